"""The sma.c seam for the clipped and per-variable task steps fused into the
elastic-averaging barrier: cbx_ea_plan_step_and_optimise_clipped_variables over
buffers the CALLER owns (include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip,
the TAIL instantiations of the three task_elastic_*_kernels.hip), on one GPU.

Expected values come from the host only: per stepping replica in id order
``tests.gradient_clip_common.decide`` and ``step(..., variables=, mults=)``
(clipping on: gradients whose S is exact in any order, scale exactly 0.5) or
``tests.test_optimise_plan.per_variable_step`` (rates only), then
``tests.averaging_common.elastic_average``.  Every comparison is bit for bit over
z and ``w``, ``last``, ``s`` and ``g`` of every replica and over every slot's
record.  Each device buffer is the first n floats of a larger allocation whose
other GUARD floats hold a sentinel pattern that must come back untouched.  The
guarded buffers are tests/test_gpu_seam_step_and_optimise.py's.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact
from tests.test_gpu_seam_step_and_optimise import ALPHA, DISCARD, _rates
from tests.test_gpu_seam_step_and_optimise_elastic import CONFIGS, ElasticBuffers, ElasticData
from tests.test_gpu_step_and_synchronise_clipped import ZERO, gradient
from tests.test_optimise_plan import per_variable_step

pytestmark = pytest.mark.gpu

POLICIES = ("variables", "clipped", "clipped_variables")
KINDS = ("unclipped", "clipped", "skipped")


def clips(policy):
    return policy in ("clipped", "clipped_variables")


def per_variable(policy):
    return policy in ("variables", "clipped_variables")


def layout(n):
    """Three variables whose boundaries lie inside float4s, multipliers no power of two."""
    if n < 3:
        return (n,), (3.0,)
    a = n // 3
    return (a, a + 1, n - 2 * a - 1), (3.0, 0.75, 1.7)


class PolicyData(ElasticData):
    """tests/test_gpu_seam_step_and_optimise_elastic.py's mirror with the policy's step."""

    def __init__(self, policy, n, R, rmom, kinds=None):
        super().__init__(n, R, rmom)
        self.policy = policy
        self.variables, self.mults = layout(n)
        self.max_norm = C.exact_gradient(n)[2]
        self.decision = {}
        if clips(policy):
            kinds = kinds or [KINDS[i % 3] for i in range(R)]
            self.g = [gradient(n, k, i) for i, k in enumerate(kinds)]

    def step(self, steps, rates, wd, keep=True):
        st, pv = self.st, per_variable(self.policy)
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        self.decision = {}
        with np.errstate(all="ignore"):
            for i in range(self.R):
                if not steps[i]:
                    continue
                bufs = [st.w[i], self.g[i], self.last[i], st.s[i]]
                if clips(self.policy):
                    S, K = C.exact_sum_sq(self.g[i])
                    scale, flags = C.decide(S, K, self.max_norm, True)
                    self.decision[i] = (S, K, float(scale), flags)
                    C.step(bufs, scale, flags, self.rmom, wd, lr=rates[i], variables=self.variables if pv else None,
                           mults=self.mults if pv else None)
                else:
                    per_variable_step(rates[i], self.mults, self.rmom, wd, *bufs, variables=self.variables)
            AV.elastic_average(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g


class PolicyBuffers(ElasticBuffers):
    def call(self, plan, steps, rates, wd, flags=0, slots="own", use_variables=None, max_norm=None, skip=True, **nulls):
        d = self.d
        if slots == "own":
            slots = list(range(d.R)) if clips(d.policy) else None
        return plan.elastic_step_and_optimise_clipped_variables(
            [self.stream.cuda_stream], [self.z.ptr], self.replicas(steps, rates, **nulls), ALPHA, d.rmom, wd,
            d.st.first, flags, slots=slots, max_norm=d.max_norm if max_norm is None else max_norm, skip_nonfinite=skip,
            use_variables=per_variable(d.policy) if use_variables is None else use_variables)

    def check_records(self, plan, counts, what=""):
        """counts[i] = (steps, clipped_steps, skipped_steps) of slot i so far."""
        for i in range(self.d.R):
            rec = plan.clip_stats(0, i, self.stream.cuda_stream)
            assert (rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == tuple(counts[i]), (what, i, rec)
            if i in self.d.decision:
                S, K, scale, flags = self.d.decision[i]
                assert (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"]) == (S, K, scale, flags), (what, i, rec)


def _count(counts, d):
    for i, (_, _, _, flags) in d.decision.items():
        counts[i][0] += 1
        counts[i][1] += 1 if flags & C.CLIPPED else 0
        counts[i][2] += 1 if flags & C.SKIPPED else 0


def _plan(policy, n):
    from crossbow_amd.seam import SmaPlan
    plan = SmaPlan([0], n)
    if per_variable(policy):
        variables, mults = layout(n)
        plan.set_variables(list(variables), list(mults))
    return plan


def _run(policy, n, R, config, flags, steps=None, first=0, held=(), s_null=()):
    rmom, wd = CONFIGS[config]
    d = PolicyData(policy, n, R, rmom)
    d.st.first = first
    for i in held:
        d.st.locked[i] = 0
    steps = [i >= first and i not in held for i in range(R)] if steps is None else steps
    rates = _rates(R)
    buf = PolicyBuffers(d)
    with _plan(policy, n) as plan:
        buf.call(plan, steps, rates, wd, flags, s_null=s_null)
        d.step(steps, rates, wd, keep=flags == 0)
        buf.check()
        if clips(policy):
            counts = [[0, 0, 0] for _ in range(R)]
            _count(counts, d)
            buf.check_records(plan, counts)
    return buf


# elements: one float, the tail alone; 771, an empty bulk under the quantum of 1,024 floats; 2,051, a bulk
# of 512 float4s and three floats behind it; 70,001, ragged over several waves.  R: unrolled, and the first
# second chunk.  The two one-sided configurations take the tail-only and the ragged size.
SHAPES = [(n, R, config) for n in (1, 771, 2_051, 70_001) for R in (2, 9) for config in CONFIGS
          if config in ("mom-wd", "plain") or n in (771, 70_001)]


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n,R,config", SHAPES)
@pytest.mark.parametrize("policy", POLICIES)
def test_every_buffer_and_record_bitexact(policy, n, R, config, flags):
    _run(policy, n, R, config, flags)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [771, 2_051, 70_001])
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_mask_first_and_held(policy, n, flags):
    # of 9: replica 0 below `first`, 4 held by a task, 1, 5 and 8 stepping (clipped, skipped, skipped), the
    # others only joining: their g and last are never read, their slots never touched
    _run(policy, n, 9, "mom-wd", flags, steps=[i in (1, 5, 8) for i in range(9)], first=1, held=(4,))


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("policy", POLICIES)
def test_a_null_s_g_and_last_where_allowed(policy, flags):
    # s: the joiners' always, the stepping ones' under discard; g and last of a replica that only joins
    n, R, steps = 2_051, 4, [True, False, True, False]
    rmom, wd = CONFIGS["mom-wd"]
    d = PolicyData(policy, n, R, rmom)
    rates = _rates(R)
    buf = PolicyBuffers(d)
    with _plan(policy, n) as plan:
        buf.call(plan, steps, rates, wd, flags, s_null=(1, 3) if flags == 0 else (0, 1, 2, 3), g_null=(1, 3),
                 rlast_null=(1, 3))
        d.step(steps, rates, wd, keep=flags == 0)
        buf.check()


@pytest.mark.parametrize("policy", POLICIES)
def test_records_and_buffers_equal_the_sequences(policy):
    # the per-replica step of the header's table on a second set of buffers and slots, then cbx_ea_plan_step
    from crossbow_amd.seam import optimise_buffers
    n, R = 2_051, 3
    rmom, wd = CONFIGS["mom-wd"]
    rates = _rates(R)
    fused, seq = PolicyBuffers(PolicyData(policy, n, R, rmom)), PolicyBuffers(PolicyData(policy, n, R, rmom))
    with _plan(policy, n) as plan:
        for clock in range(2):
            fused.call(plan, [True] * R, rates, wd)
            st = seq.stream.cuda_stream
            for i in range(R):
                args = (seq.w[i].ptr, seq.g[i].ptr, seq.last[i].ptr, seq.s[i].ptr)
                if clips(policy):
                    plan.optimise_clipped(0, R + i, st, *args, rates[i], rmom, wd, seq.d.max_norm, True,
                                          per_variable(policy))
                elif per_variable(policy):
                    plan.optimise_variables(0, st, *args, rates[i], rmom, wd, 0, len(seq.d.variables))
                else:
                    optimise_buffers(st, *args, n, rates[i], rmom, wd)
            plan.elastic_step([st], [seq.z.ptr], [(0, seq.w[i].ptr, None, 1) for i in range(R)], ALPHA)
            fused.stream.synchronize()
            seq.stream.synchronize()
            pairs = [(fused.z, seq.z, "z")]
            for i in range(R):
                pairs += [(fused.w[i], seq.w[i], f"w[{i}]"), (fused.s[i], seq.s[i], f"s[{i}]"),
                          (fused.g[i], seq.g[i], f"g[{i}]"), (fused.last[i], seq.last[i], f"last[{i}]")]
            for a, b, name in pairs:
                assert_bitexact(a.t.cpu().numpy(), b.t.cpu().numpy(), f"clock {clock}: {name} against the sequence")
            if clips(policy):
                for i in range(R):
                    assert plan.clip_stats(0, i, fused.stream.cuda_stream) == plan.clip_stats(0, R + i, st), (clock, i)
                    assert plan.clip_stats(0, i, st)["steps"] == clock + 1


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_with_both_off_it_is_the_plain_call(flags):
    n, R = 2_051, 3
    rmom, wd = CONFIGS["mom-wd"]
    rates = _rates(R)
    from crossbow_amd.seam import SmaPlan
    a, b = PolicyBuffers(PolicyData("variables", n, R, rmom)), ElasticBuffers(ElasticData(n, R, rmom))
    with SmaPlan([0], n) as plan:
        a.call(plan, [True] * R, rates, wd, flags, slots=None, use_variables=False)
        b.call(plan, [True] * R, rates, wd, flags)
        b.d.step([True] * R, rates, wd, keep=flags == 0)
        b.check()
        a.stream.synchronize()
        for x, y, name in [(a.z, b.z, "z")] + [(getattr(a, k)[i], getattr(b, k)[i], f"{k}[{i}]")
                                               for k in ("w", "s", "g", "last") for i in range(R)]:
            assert_bitexact(x.t.cpu().numpy(), y.t.cpu().numpy(), name)


@pytest.mark.parametrize("policy", ["clipped", "clipped_variables"])
def test_nobody_steps_touches_no_record_and_max_norm_zero_still_counts(policy):
    n, R = 2_051, 3
    rmom, wd = CONFIGS["mom-wd"]
    rates = _rates(R)
    d = PolicyData(policy, n, R, rmom, kinds=["clipped"] * R)
    buf = PolicyBuffers(d)
    with _plan(policy, n) as plan:
        buf.call(plan, [False] * R, rates, wd, s_null=(0, 1, 2), g_null=(0, 1, 2), rlast_null=(0, 1, 2))
        d.step([False] * R, rates, wd)
        buf.check()
        # a slot nobody has used reads as zeros once it exists
        plan.gradient_norm(0, 40, buf.stream.cuda_stream, buf.g[0].ptr)
        assert plan.clip_stats(0, 40, buf.stream.cuda_stream)["steps"] == 1
        # max_norm == 0 and no skip: the norm is reduced and the step counted, nothing is clipped
        buf.call(plan, [True] * R, rates, wd, max_norm=0.0, skip=False)
        d.max_norm = 0.0
        st = d.st
        for i in range(R):
            S, K = C.exact_sum_sq(d.g[i])
            C.step([st.w[i], d.g[i], d.last[i], st.s[i]], np.float32(1.0), 0, rmom, wd, lr=rates[i],
                   variables=d.variables if per_variable(policy) else None,
                   mults=d.mults if per_variable(policy) else None)
            rec = plan.clip_stats(0, i, buf.stream.cuda_stream)
            assert (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"]) == (S, K, 1.0, 0), rec
            assert (rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == (1, 0, 0), rec
        AV.elastic_average(st)
        buf.check("max_norm 0:")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("policy", POLICIES)
def test_then_elastic_and_sma_steps_on_the_same_plan(policy, flags):
    """The calls share the plan's scratch and the caller's stream order: the
    plan's state is not disturbed."""
    from crossbow_amd.seam import optimise_buffers
    n, R = 2_051, 3
    rmom, wd = CONFIGS["mom-wd"]
    d = PolicyData(policy, n, R, rmom)
    buf = PolicyBuffers(d)
    rates = _rates(R)
    st = d.st
    with _plan(policy, n) as plan:
        for clock in range(2):
            buf.call(plan, [True] * R, rates, wd, flags)
            d.step([True] * R, rates, wd, keep=flags == 0)
            buf.check(f"clock {clock}:")
        plan.elastic_step([buf.stream.cuda_stream], [buf.z.ptr], [(0, buf.w[i].ptr, None, 1) for i in range(R)], ALPHA)
        AV.elastic_average(st)
        buf.check("after cbx_ea_plan_step:")
        # a plain task step of the finite replicas first, so that s is the sequence's before the SMA barrier reads it
        for i in range(R):
            if np.isfinite(d.g[i]).all():
                optimise_buffers(buf.stream.cuda_stream, buf.w[i].ptr, buf.g[i].ptr, buf.last[i].ptr, buf.s[i].ptr, n,
                                 rates[i], rmom, wd)
                O.sma_optimise(np.float32(-rates[i]), rmom, wd, st.w[i], d.g[i], d.last[i], st.s[i])
        if flags == 0:  # every s was written: the SMA barrier reads them
            reps = [(0, buf.w[i].ptr, buf.s[i].ptr, 1, 0) for i in range(R)]
            plan.step([buf.stream.cuda_stream], [buf.z.ptr], None, reps, ALPHA, 0.0)
            O.sma_step(st)
            buf.check("after cbx_sma_plan_step:")
        buf.call(plan, [True] * R, rates, wd, flags)
        d.step([True] * R, rates, wd, keep=flags == 0)
        buf.check("the fused call again:")


# name: (error code name, keyword arguments of the call)
REFUSED = {
    "flag_bit_2": ("CBX_ERR_INVALID", dict(flags=2)),
    "stepping_unlocked": ("CBX_ERR_INVALID", dict(held=(1,), steps=[True, True, True])),
    "stepping_below_first": ("CBX_ERR_INVALID", dict(first=1, steps=[True, True, True])),
    "null_g_of_a_stepping_replica": ("CBX_ERR_INVALID", dict(g_null=(2,))),
    "null_rlast_with_replica_momentum": ("CBX_ERR_INVALID", dict(rlast_null=(0,))),
    "null_s_of_a_stepping_replica_kept": ("CBX_ERR_INVALID", dict(s_null=(1,))),
    "slot_out_of_range": ("CBX_ERR_INVALID", dict(slots=[0, 64, 2])),
    "slot_negative": ("CBX_ERR_INVALID", dict(slots=[0, -1, 2])),
    "slot_named_twice": ("CBX_ERR_INVALID", dict(slots=[5, 1, 5])),
    "max_norm_negative": ("CBX_ERR_INVALID", dict(max_norm=-1.0)),
    "max_norm_nan": ("CBX_ERR_INVALID", dict(max_norm=float("nan"))),
    "max_norm_infinite": ("CBX_ERR_INVALID", dict(max_norm=float("inf"))),
    "use_variables_without_a_table": ("CBX_ERR_STATE", dict(table=False)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_calls_write_nothing_and_bump_no_counter(name):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    code, kw = REFUSED[name]
    kw = dict(kw)
    n, R, wd = 4_099, 3, 5e-4
    d = PolicyData("clipped_variables", n, R, 0.9, kinds=["clipped"] * R)
    d.st.first = kw.pop("first", 0)
    for i in kw.pop("held", ()):
        d.st.locked[i] = 0
    steps, table = kw.pop("steps", [True] * R), kw.pop("table", True)
    buf = PolicyBuffers(d)
    rates = _rates(R)
    with (_plan("clipped_variables", n) if table else SmaPlan([0], n)) as plan:
        for i in (0, 1, 2, 5):  # the slots exist and have counted one norm each
            plan.gradient_norm(0, i, buf.stream.cuda_stream, buf.g[0].ptr, d.max_norm, True)
        records = [plan.clip_stats(0, i, buf.stream.cuda_stream) for i in (0, 1, 2, 5)]
        assert all(r["steps"] == 1 for r in records)
        with pytest.raises(CbxError) as e:
            buf.call(plan, steps, rates, wd, **kw)
        assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_ea_plan_step_and_optimise_clipped_variables" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")  # the host mirror never stepped
        assert [plan.clip_stats(0, i, buf.stream.cuda_stream) for i in (0, 1, 2, 5)] == records, "no counter was bumped"
        if table:  # and the plan still works
            d.st.first = 0
            d.st.locked[:] = 1
            buf.call(plan, [True] * R, rates, wd)
            d.step([True] * R, rates, wd)
            buf.check("after a good call:")


def test_use_variables_is_0_or_1_and_a_null_plan_is_invalid():
    from crossbow_amd import _lib
    lib = _lib.load()
    rc = lib.cbx_ea_plan_step_and_optimise_clipped_variables(None, None, None, 0, None, None, None, None, None, None,
                                                             None, None, None, 1.0, 0, 2, 0.1, 0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    from crossbow_amd.seam import SmaPlan
    n, R = 1_027, 2
    d = PolicyData("variables", n, R, 0.0)
    buf = PolicyBuffers(d)
    with SmaPlan([0], n) as plan:
        import ctypes

        from crossbow_amd.seam import _ints, _ptrs
        reps = buf.replicas([True] * R, _rates(R))
        rc = plan.lib.cbx_ea_plan_step_and_optimise_clipped_variables(
            plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), R, _ints([r[0] for r in reps]),
            _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]), _ptrs([r[3] for r in reps]),
            _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]), _ints([r[6] for r in reps]),
            (ctypes.c_float * R)(*_rates(R)), None, 0.0, 0, 2, ALPHA, 0.0, 0.0, 0, 0)
        assert rc == _lib.CBX_ERR_INVALID and "use_variables" in _lib.last_error()
        buf.check()


def test_more_than_64_participating_replicas_is_unsupported():
    import torch

    from crossbow_amd import CbxError, _lib
    n, R, wd = 1_027, 2, 0.0
    d = PolicyData("variables", n, R, 0.0)
    buf = PolicyBuffers(d)
    reps = buf.replicas([True] * R, _rates(R))
    with _plan("variables", n) as plan:
        with pytest.raises(CbxError) as e:
            plan.elastic_step_and_optimise_clipped_variables(
                [buf.stream.cuda_stream], [buf.z.ptr], [reps[i % R] for i in range(65)], ALPHA, 0.0, wd,
                use_variables=True)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        buf.check()
