"""The sma.c seam for the fused task steps with gradient clipping and a
learning rate per variable: cbx_sma_plan_step_and_optimise_clipped_variables
over buffers the CALLER owns (include/crossbow_sma.h,
crossbow_amd/csrc/sma_seam.hip, the TAIL instantiations of
task_barrier_clipped_variables_kernels.hip), on one GPU.

Expected values come from the host only: per stepping replica in id order
``tests.gradient_clip_common.decide`` and ``step(..., variables=, mults=)`` over
gradients whose S is exact in any order and that are non-zero in every variable
(tests/clipped_variables_common.py), then ``O.sma_step``.  Every comparison is
bit for bit over z, the base ``last``, and ``w``, ``last``, ``s`` and ``g`` of
every replica; each device buffer holds exactly n floats in front of 1,088
sentinel floats that must come back untouched (tests/helpers.py, Guarded).  The
records are compared with those a second plan holds after
``cbx_sma_plan_optimise_clipped(..., use_variables = 1)`` per stepping replica
followed by ``cbx_sma_plan_step``.

Sizes: 1 (one tail float), 771 (an empty bulk, three variables, one of them
empty), 1,029 (one chunk and 5 tail floats; once with a boundary inside a
chunk of the table, once split exactly at float 512) and 21,523 (``V``: 21
chunks, 19 tail floats, six norm tiles).
"""
from __future__ import annotations

import ctypes

import pytest

from oracle import oracle as O
from tests import clipped_variables_common as CV
from tests import gradient_clip_common as C
from tests.helpers import GUARD
from tests.test_gpu_seam_step_and_optimise import ALPHA, CONFIGS, DISCARD, Buffers, Data, _rates
from tests.test_gpu_seam_step_and_optimise_clipped import BAD_SLOTS, KINDS
from tests.test_optimise_plan import M, V

pytestmark = pytest.mark.gpu

assert GUARD == 1088
# name: (variables, multipliers)
MODELS = {
    "tail-only-1": ((1,), (3.0,)),
    "empty-bulk-771": ((300, 0, 471), (2.0, 7.0, 0.5)),
    "boundary-in-chunk-1029": ((1000, 29), (2.0, 0.25)),
    "split-at-512-1029": ((512, 517), (0.5, 2.0)),
    "V-21523": (V, M),
}
CONFIGS = dict(CONFIGS, **{"mom-only": (0.9, 0.0, 0.9)})


class BothData(Data):
    def __init__(self, model, kinds, rmom, bmom):
        self.variables, self.mults = MODELS[model]
        super().__init__(sum(self.variables), len(kinds), rmom, bmom)
        self.kinds = kinds
        self.g = [CV.gradient(self.n, k if k != "join" else "unclipped", i, self.variables)
                  for i, k in enumerate(kinds)]
        self.max_norm = CV.dense_gradient(self.n)[2]
        self.slots = [5 + 7 * i for i in range(self.R)]  # < 64 for R <= 9, all different
        self.steps = [k != "join" for k in kinds]

    def step(self, steps, rates, wd, keep=True, c=None, skip=True):
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        self.decision = {}
        for i in range(self.R):
            if steps[i]:
                S, K = C.exact_sum_sq(self.g[i])
                scale, flags = C.decide(S, K, self.max_norm if c is None else c, skip)
                self.decision[i] = {"sum_sq": S, "nonfinite": K, "scale": float(scale), "flags": flags}
                C.step([st.w[i], self.g[i], self.last[i], st.s[i]], scale, flags, self.rmom, wd, lr=rates[i],
                       variables=self.variables, mults=self.mults)
        copies = O.sma_step(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g
        return 1 if copies > 0 else 0


class BothBuffers(Buffers):
    def call(self, plan, steps, rates, wd, flags=0, slots="own", c=None, skip=True, **nulls):
        st, d = self.d.st, self.d
        return plan.step_and_optimise_clipped_variables(
            [self.stream.cuda_stream], [self.z.ptr], [self.blast.ptr] if self.blast is not None else None,
            self.replicas(steps, rates, **nulls), ALPHA, st.momentum, d.rmom, wd, st.first, flags,
            slots=d.slots if slots == "own" else slots, max_norm=d.max_norm if c is None else c, skip_nonfinite=skip)

    def sequence(self, plan, steps, rates, wd):
        """The two-call sequence of the header on these buffers."""
        d, st = self.d, self.d.st
        for i in range(d.R):
            if steps[i]:
                plan.optimise_clipped(0, d.slots[i], self.stream.cuda_stream, self.w[i].ptr, self.g[i].ptr,
                                      self.last[i].ptr if self.last[i] is not None else None, self.s[i].ptr, rates[i],
                                      d.rmom, wd, d.max_norm, True, use_variables=True)
        reps = [(0, self.w[i].ptr, self.s[i].ptr, int(st.locked[i]), int(st.copy[i])) for i in range(d.R)]
        return plan.step([self.stream.cuda_stream], [self.z.ptr], [self.blast.ptr] if self.blast is not None else None,
                         reps, ALPHA, st.momentum, st.first)


def _records(plan, buf, d):
    return [plan.clip_stats(0, d.slots[i], buf.stream.cuda_stream) for i in range(d.R)]


def _plan(d):
    from crossbow_amd.seam import SmaPlan
    plan = SmaPlan([0], d.n)
    plan.set_variables(list(d.variables), list(d.mults))
    return plan


def _run(model, R, config, flags, copies=()):
    rmom, wd, bmom = CONFIGS[config]
    kinds = KINDS[R]
    d, twin = BothData(model, kinds, rmom, bmom), BothData(model, kinds, rmom, bmom)
    for i in copies:
        d.st.copy[i] = twin.st.copy[i] = 1
    rates = _rates(R)
    buf, seq = BothBuffers(d), BothBuffers(twin)
    with _plan(d) as plan, _plan(d) as second:
        got = buf.call(plan, d.steps, rates, wd, flags)
        want = d.step(d.steps, rates, wd, keep=flags == 0)
        buf.check()
        assert got == want, (got, want)
        # the records: the host's decisions, and every byte of the sequence's on a second plan
        seq.sequence(second, d.steps, rates, wd)
        records, theirs = _records(plan, buf, d), _records(second, seq, twin)
        assert records == theirs
        for i in range(R):
            if d.steps[i]:
                flags_i = d.decision[i]["flags"]
                assert records[i] == dict(d.decision[i], steps=1, clipped_steps=flags_i & 1, skipped_steps=flags_i >> 1), i
        if flags == 0:
            twin.step(d.steps, rates, wd)
            seq.check("the sequence:")
    return buf, got


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("model", [m for m in MODELS if len(MODELS[m][0]) > 1])
def test_the_multipliers_show_on_the_host(model, config):
    rmom, wd, _ = CONFIGS[config]
    CV.multipliers_show(*MODELS[model], rmom, wd)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("R", [1, 4, 8, 9])
@pytest.mark.parametrize("model", list(MODELS))
def test_every_buffer_and_record_bitexact(model, R, config, flags):
    _run(model, R, config, flags)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("model", ["tail-only-1", "split-at-512-1029", "V-21523"])
def test_phase_d_beside_a_skipped_replica(model, flags):
    from tests.helpers import assert_bitexact
    R = 4  # a copy flag on the skipped replica (1) and on the one that only joins (3)
    buf, got = _run(model, R, "mom-wd", flags, copies=(1, 3))
    assert got == 1
    n = buf.d.n
    z = buf.z.t.cpu().numpy()[:n]
    for i in range(R):
        assert_bitexact(buf.w[i].t.cpu().numpy()[:n], z, f"w[{i}] == the new z, tail included")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_when_nobody_steps_it_is_the_per_variable_call(flags):
    # no norm, no record touched (no slot list is needed), and the buffers are the barrier's
    rmom, wd, bmom = CONFIGS["mom-wd"]
    d = BothData("boundary-in-chunk-1029", ["join"] * 3, rmom, bmom)
    buf = BothBuffers(d)
    with _plan(d) as plan:
        zero = _records(plan, buf, d)
        assert all(not any(rec.values()) for rec in zero)
        got = buf.call(plan, d.steps, _rates(3), wd, flags, slots=None)
        want = d.step(d.steps, _rates(3), wd, keep=flags == 0)
        buf.check()
        assert got == want and _records(plan, buf, d) == zero


# ---- refusals ----------------------------------------------------------------------------------------
def test_before_set_variables_it_is_a_state_error_and_writes_nothing():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    rmom, wd, bmom = CONFIGS["mom-wd"]
    d = BothData("boundary-in-chunk-1029", ["clipped", "skipped", "unclipped"], rmom, bmom)
    rates = _rates(3)
    buf = BothBuffers(d)
    with SmaPlan([0], d.n) as plan:
        zero = _records(plan, buf, d)
        with pytest.raises(CbxError) as e:
            buf.call(plan, d.steps, rates, wd)
        assert e.value.code == _lib.CBX_ERR_STATE, str(e.value)
        assert "cbx_sma_plan_step_and_optimise_clipped_variables" in _lib.last_error()
        with pytest.raises(CbxError) as e:  # before the clip arguments are looked at
            buf.call(plan, d.steps, rates, wd, slots=None)
        assert e.value.code == _lib.CBX_ERR_STATE, str(e.value)
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        assert _records(plan, buf, d) == zero
        plan.set_variables(list(d.variables), list(d.mults))  # and the plan works once it has one
        buf.call(plan, d.steps, rates, wd)
        d.step(d.steps, rates, wd)
        buf.check("after a good call:")


@pytest.mark.parametrize("name", list(BAD_SLOTS))
def test_slot_refusals_write_nothing_and_bump_no_counter(name):
    import torch

    from crossbow_amd import CbxError, _lib
    rmom, wd, bmom = CONFIGS["mom-wd"]
    d = BothData("boundary-in-chunk-1029", ["clipped", "skipped", "unclipped"], rmom, bmom)
    d.slots = [0, 1, 2]
    rates = _rates(3)
    buf = BothBuffers(d)
    with _plan(d) as plan:
        zero = _records(plan, buf, d)  # allocates the three slots: all zeros
        assert all(not any(rec.values()) for rec in zero)
        with pytest.raises(CbxError) as e:
            buf.call(plan, d.steps, rates, wd, slots=BAD_SLOTS[name])
        assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        assert "cbx_sma_plan_step_and_optimise_clipped_variables" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        assert _records(plan, buf, d) == zero
        # a replica that does not step needs no slot, and may name one that another uses
        d.steps = [True, True, False]
        buf.call(plan, d.steps, rates, wd, slots=[0, 1, 77])
        d.step(d.steps, rates, wd)
        buf.check("after a good call:")


@pytest.mark.parametrize("what", ["max_norm_negative", "max_norm_nan", "max_norm_inf", "skip_2"])
def test_bad_clip_arguments_are_refused(what):
    import torch

    from crossbow_amd import _lib
    from crossbow_amd.seam import _ints, _ptrs
    rmom, wd, bmom = CONFIGS["mom-wd"]
    d = BothData("empty-bulk-771", ["clipped", "skipped"], rmom, bmom)
    R = d.R
    buf = BothBuffers(d)
    reps = buf.replicas(d.steps, _rates(R))
    c = {"max_norm_negative": -1.0, "max_norm_nan": float("nan"), "max_norm_inf": float("inf")}.get(what, 1.0)
    with _plan(d) as plan:
        rc = plan.lib.cbx_sma_plan_step_and_optimise_clipped_variables(
            plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), _ptrs([buf.blast.ptr]), R,
            _ints([r[0] for r in reps]), _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]),
            _ptrs([r[3] for r in reps]), _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]),
            _ints([r[6] for r in reps]), _ints([r[7] for r in reps]), (ctypes.c_float * R)(*_rates(R)),
            _ints(d.slots), ctypes.c_float(c), 2 if what == "skip_2" else 1, ALPHA, 0.9, rmom, wd, 0, 0)
        assert rc == _lib.CBX_ERR_INVALID, _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        assert all(not any(rec.values()) for rec in _records(plan, buf, d))
