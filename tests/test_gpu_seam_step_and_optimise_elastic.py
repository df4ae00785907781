"""The sma.c seam for the task steps fused into the elastic-averaging barrier:
cbx_ea_plan_step_and_optimise over buffers the CALLER owns
(include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip, the TAIL
instantiations of task_elastic_kernels.hip), on one GPU.

Expected values come from the oracle only: ``O.sma_optimise`` for every
stepping replica in id order, then ``tests.averaging_common.elastic_average``.
Every comparison is bit for bit over z and ``w``, ``last``, ``s`` and ``g`` of
every replica.  Each device buffer is the first n floats of a larger allocation
whose other GUARD floats hold a sentinel pattern that must come back untouched:
a bulk or tail store past ``elements`` would break it.  The mirror and the
guarded buffers are tests/test_gpu_seam_step_and_optimise.py's.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests.helpers import assert_bitexact
from tests.test_gpu_seam_step_and_optimise import ALPHA, DISCARD, Buffers, Data, _rates

pytestmark = pytest.mark.gpu

# (replica momentum, weight decay)
CONFIGS = {"mom-wd": (0.9, 5e-4), "plain": (0.0, 0.0), "mom": (0.9, 0.0), "wd": (0.0, 5e-4)}


class ElasticData(Data):
    def __init__(self, n, R, rmom, seed=0):
        super().__init__(n, R, rmom, 0.0, seed)  # no base momentum: st.last is None

    def step(self, steps, rates, wd, keep=True):
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        for i in range(self.R):
            if steps[i]:
                O.sma_optimise(np.float32(-rates[i]), self.rmom, wd, st.w[i], self.g[i], self.last[i], st.s[i])
        AV.elastic_average(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g


class ElasticBuffers(Buffers):
    def replicas(self, steps, rates, s_null=(), g_null=(), rlast_null=()):
        st = self.d.st
        return [(0, self.w[i].ptr, None if i in s_null else self.s[i].ptr, None if i in g_null else self.g[i].ptr,
                 None if self.last[i] is None or i in rlast_null else self.last[i].ptr, int(st.locked[i]),
                 int(bool(steps[i])), rates[i]) for i in range(self.d.R)]

    def call(self, plan, steps, rates, wd, flags=0, **nulls):
        return plan.elastic_step_and_optimise([self.stream.cuda_stream], [self.z.ptr],
                                              self.replicas(steps, rates, **nulls), ALPHA, self.d.rmom, wd,
                                              self.d.st.first, flags)


def _run(n, R, config, flags, steps=None, first=0, held=(), s_null=()):
    from crossbow_amd.seam import SmaPlan
    rmom, wd = CONFIGS[config]
    d = ElasticData(n, R, rmom)
    d.st.first = first
    for i in held:
        d.st.locked[i] = 0
    steps = [i >= first and i not in held for i in range(R)] if steps is None else steps
    rates = _rates(R)
    buf = ElasticBuffers(d)
    with SmaPlan([0], n) as plan:
        buf.call(plan, steps, rates, wd, flags, s_null=s_null)
        d.step(steps, rates, wd, keep=flags == 0)
        buf.check()
    return buf


# elements: one float, the tail alone; 771, an empty bulk under the quantum of 1,024 floats; 2,051, a bulk
# of 512 float4s and three floats behind it; 70,001, ragged over several waves.  R: unrolled, and the first
# second chunk.  The two one-sided configurations take the tail-only and the ragged size.
SHAPES = [(n, R, config) for n in (1, 771, 2_051, 70_001) for R in (2, 9) for config in CONFIGS
          if config in ("mom-wd", "plain") or n in (771, 70_001)]


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n,R,config", SHAPES)
def test_every_buffer_bitexact(n, R, config, flags):
    _run(n, R, config, flags)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [771, 2_051, 70_001])
def test_mixed_mask_first_and_held(n, flags):
    # of 9: replica 0 below `first`, 4 held by a task, 1, 5 and 8 stepping, the others only joining
    _run(n, 9, "mom-wd", flags, steps=[i in (1, 5, 8) for i in range(9)], first=1, held=(4,))


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [771, 70_001])
def test_a_null_s_for_joiners_and_under_discard(n, flags):
    R, steps = 4, [True, False, True, False]
    s_null = (1, 3) if flags == 0 else (0, 1, 2, 3)  # the joiners' always; the stepping ones' under discard
    buf = _run(n, R, "mom-wd", flags, steps=steps, s_null=s_null)
    fresh = ElasticData(n, R, 0.9)
    for i in range(R):  # s and g are rewritten by a stepping replica whose outputs are kept, and by nobody else
        changed = steps[i] and flags == 0
        assert np.any(buf.s[i].t.cpu().numpy()[:n] != fresh.st.s[i]) == changed, f"s[{i}]"
        assert np.any(buf.g[i].t.cpu().numpy()[:n] != fresh.g[i]) == changed, f"g[{i}]"


@pytest.mark.parametrize("n", [771, 70_001])
def test_nobody_steps_is_the_plain_elastic_step(n):
    from crossbow_amd.seam import SmaPlan
    R = 9
    buf = _run(n, R, "mom-wd", 0, steps=[False] * R, s_null=tuple(range(R)))
    plain = ElasticBuffers(ElasticData(n, R, 0.9))
    with SmaPlan([0], n) as plan:
        plan.elastic_step([plain.stream.cuda_stream], [plain.z.ptr], [(0, plain.w[i].ptr, None, 1) for i in range(R)],
                          ALPHA)
        plain.stream.synchronize()
    for a, b, name in [(buf.z, plain.z, "z")] + [(buf.w[i], plain.w[i], f"w[{i}]") for i in range(R)]:
        assert_bitexact(a.t.cpu().numpy(), b.t.cpu().numpy(), name)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_then_elastic_and_sma_steps_on_the_same_plan(flags):
    """The calls share the plan's scratch and the caller's stream order: the
    plan's state is not disturbed."""
    from crossbow_amd.seam import SmaPlan, optimise_buffers
    n, R, wd = 2_051, 3, 5e-4
    d = ElasticData(n, R, 0.9)
    buf = ElasticBuffers(d)
    rates = _rates(R)
    st = d.st
    with SmaPlan([0], n) as plan:
        for clock in range(2):
            buf.call(plan, [True] * R, rates, wd, flags)
            d.step([True] * R, rates, wd, keep=flags == 0)
            buf.check(f"clock {clock}:")
        plan.elastic_step([buf.stream.cuda_stream], [buf.z.ptr], [(0, buf.w[i].ptr, None, 1) for i in range(R)], ALPHA)
        AV.elastic_average(st)
        buf.check("after cbx_ea_plan_step:")
        # a plain task step first, so that s is the sequence's before the SMA barrier reads it
        for i in range(R):
            optimise_buffers(buf.stream.cuda_stream, buf.w[i].ptr, buf.g[i].ptr, buf.last[i].ptr, buf.s[i].ptr, n,
                             rates[i], 0.9, wd)
            O.sma_optimise(np.float32(-rates[i]), 0.9, wd, st.w[i], d.g[i], d.last[i], st.s[i])
        reps = [(0, buf.w[i].ptr, buf.s[i].ptr, 1, 0) for i in range(R)]
        plan.step([buf.stream.cuda_stream], [buf.z.ptr], None, reps, ALPHA, 0.0)
        O.sma_step(st)
        buf.check("after cbx_sma_plan_step:")
        buf.call(plan, [True] * R, rates, wd, flags)
        d.step([True] * R, rates, wd, keep=flags == 0)
        buf.check("the fused call again:")


def test_each_call_adds_one_timing_entry():
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 4099, 3, 5e-4
    d = ElasticData(n, R, 0.9)
    buf = ElasticBuffers(d)
    rates = _rates(R)
    with SmaPlan([0], n) as plan:
        plan.set_timing(True)
        assert plan.timing_history(4) == []
        for flags in (0, DISCARD):
            buf.call(plan, [True] * R, rates, wd, flags)
            d.step([True] * R, rates, wd, keep=flags == 0)
        t = plan.timing_history(8)
        assert len(t) == 2 and all(0.0 < x < 100.0 for x in t), t
        buf.check()


# name: (what is wrong, keyword arguments of the call)
INVALID = {
    "flag_bit_2": dict(flags=2),
    "stepping_unlocked": dict(held=(1,), steps=[True, True, True]),
    "stepping_below_first": dict(first=1, steps=[True, True, True]),
    "null_g_of_a_stepping_replica": dict(g_null=(2,)),
    "null_rlast_with_replica_momentum": dict(rlast_null=(0,)),
    "null_s_of_a_stepping_replica_kept": dict(s_null=(1,)),
    "null_g_array": dict(null_array=7),
    "null_step_array": dict(null_array=10),
    "null_rate_array": dict(null_array=11),
}


@pytest.mark.parametrize("name", list(INVALID))
def test_invalid_calls_write_nothing(name):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan, _ints, _ptrs
    kw = dict(INVALID[name])
    n, R, wd = 4099, 3, 5e-4
    d = ElasticData(n, R, 0.9)
    d.st.first = kw.pop("first", 0)
    for i in kw.pop("held", ()):
        d.st.locked[i] = 0
    steps, flags, null_array = kw.pop("steps", [True] * R), kw.pop("flags", 0), kw.pop("null_array", None)
    buf = ElasticBuffers(d)
    rates = _rates(R)
    with SmaPlan([0], n) as plan:
        if null_array is None:
            with pytest.raises(CbxError) as e:
                buf.call(plan, steps, rates, wd, flags, **kw)
            assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        else:
            reps = buf.replicas(steps, rates)
            args = [plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), R, _ints([r[0] for r in reps]),
                    _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]), _ptrs([r[3] for r in reps]),
                    _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]), _ints([r[6] for r in reps]),
                    (ctypes.c_float * R)(*rates), ALPHA, 0.9, wd, 0, 0]
            args[null_array] = None
            assert plan.lib.cbx_ea_plan_step_and_optimise(*args) == _lib.CBX_ERR_INVALID
        assert "cbx_ea_plan_step_and_optimise" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")  # the host mirror never stepped
        d.st.first = 0
        d.st.locked[:] = 1
        buf.call(plan, [True] * R, rates, wd)  # and the plan still works
        d.step([True] * R, rates, wd)
        buf.check("after a good call:")


def test_more_than_64_participating_replicas_is_unsupported():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 1027, 2, 0.0
    d = ElasticData(n, R, 0.0)
    buf = ElasticBuffers(d)
    reps = buf.replicas([True] * R, _rates(R))
    with SmaPlan([0], n) as plan:
        with pytest.raises(CbxError) as e:
            plan.elastic_step_and_optimise([buf.stream.cuda_stream], [buf.z.ptr], [reps[i % R] for i in range(65)],
                                           ALPHA, 0.0, wd)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        buf.check()
