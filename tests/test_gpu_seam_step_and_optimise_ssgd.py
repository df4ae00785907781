"""The sma.c seam for the task steps fused into the synchronous-SGD barrier:
cbx_ssgd_plan_step_and_optimise over buffers the CALLER owns
(include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip, the TAIL
instantiations of task_ssgd_kernels.hip), on one GPU.

Expected values come from the oracle only: ``O.ssgd_worker`` for every stepping
replica in id order, then ``O.ssgd_sync``.  Every comparison is bit for bit over
z, the base ``last``, the accumulator (all +0 afterwards) and ``w`` and ``g`` of
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
from tests.helpers import Guarded, assert_bitexact
from tests.test_gpu_seam_step_and_optimise import ALPHA, DISCARD, Buffers, Data, _rates

pytestmark = pytest.mark.gpu

# (base momentum, weight decay)
CONFIGS = {"mom-wd": (0.9, 5e-4), "plain": (0.0, 0.0), "mom": (0.9, 0.0), "wd": (0.0, 5e-4)}


class SsgdData(Data):
    def __init__(self, n, R, bmom, wpc=None, acc_seed=None, seed=0):
        super().__init__(n, R, 0.0, bmom, seed)  # no replica momentum under WORKER: no replica `last`
        self.wpc = R if wpc is None else wpc
        # the accumulator as the call finds it: zero, or what earlier task steps left
        self.acc = np.zeros(n, np.float32) if acc_seed is None else O.fill_normal(n, acc_seed, 0.01)

    def step(self, steps, rates, wd, keep=True):
        st = self.st
        kept = {i: self.g[i].copy() for i in range(self.R) if steps[i] and not keep}
        for i in range(self.R):  # ascending id: the accumulator depends on the order
            if steps[i]:
                O.ssgd_worker(np.float32(-rates[i]), wd, st.w[i], self.g[i], self.acc)
        O.ssgd_sync(st, [self.acc], self.wpc)
        for i, g in kept.items():
            self.g[i] = g


class SsgdBuffers(Buffers):
    def __init__(self, d):
        super().__init__(d)
        self.acc = Guarded(d.acc, 3)

    def replicas(self, steps, rates, g_null=()):
        st = self.d.st
        return [(0, self.w[i].ptr, None if i in g_null else self.g[i].ptr, int(st.locked[i]), int(bool(steps[i])),
                 rates[i]) for i in range(self.d.R)]

    def call(self, plan, steps, rates, wd, flags=0, **nulls):
        st = self.d.st
        return plan.ssgd_step_and_optimise([self.stream.cuda_stream], [self.z.ptr],
                                           [self.blast.ptr] if self.blast is not None else None, [self.acc.ptr],
                                           self.replicas(steps, rates, **nulls), st.momentum, wd, self.d.wpc, st.first,
                                           flags)

    def check(self, what=""):
        super().check(what)  # z, the base last, w, g and the untouched s of every replica
        assert not self.d.acc.any() and not np.signbit(self.d.acc).any()
        self.acc.check(self.d.acc, f"{what} acc")


def _run(n, R, config, flags, steps=None, first=0, held=(), g_null=(), wpc=None, acc_seed=None):
    from crossbow_amd.seam import SmaPlan
    bmom, wd = CONFIGS[config]
    d = SsgdData(n, R, bmom, wpc, acc_seed)
    d.st.first = first
    for i in held:
        d.st.locked[i] = 0
    steps = [i >= first and i not in held for i in range(R)] if steps is None else steps
    rates = _rates(R)
    buf = SsgdBuffers(d)
    with SmaPlan([0], n) as plan:
        buf.call(plan, steps, rates, wd, flags, g_null=g_null)
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
def test_an_accumulator_that_is_not_zero_and_another_work_per_clock(n, flags):
    _run(n, 9, "mom-wd", flags, wpc=3, acc_seed=7777)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [771, 2_051, 70_001])
def test_mixed_lists_first_and_held_with_null_g_for_joiners(n, flags):
    # of 9: replica 0 below `first`, 4 held by a task, 1, 5 and 8 stepping, the others only joining
    stepping = (1, 5, 8)
    _run(n, 9, "mom-wd", flags, steps=[i in stepping for i in range(9)], first=1, held=(4,),
         g_null=tuple(i for i in range(9) if i not in stepping), acc_seed=7778)


@pytest.mark.parametrize("n", [771, 70_001])
def test_nobody_steps_is_the_plain_ssgd_step(n):
    from crossbow_amd.seam import SmaPlan
    R = 9
    buf = _run(n, R, "mom-wd", 0, steps=[False] * R, g_null=tuple(range(R)), acc_seed=7779)
    plain = SsgdBuffers(SsgdData(n, R, 0.9, acc_seed=7779))
    with SmaPlan([0], n) as plan:
        plan.ssgd_step([plain.stream.cuda_stream], [plain.z.ptr], [plain.blast.ptr], [plain.acc.ptr],
                       [(0, plain.w[i].ptr, 1) for i in range(R)], 0.9, R)
        plain.stream.synchronize()
    pairs = [(buf.z, plain.z, "z"), (buf.blast, plain.blast, "last"), (buf.acc, plain.acc, "acc")]
    for a, b, name in pairs + [(buf.w[i], plain.w[i], f"w[{i}]") for i in range(R)]:
        assert_bitexact(a.t.cpu().numpy(), b.t.cpu().numpy(), name)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_then_ssgd_and_sma_steps_on_the_same_plan(flags):
    """The calls share the plan's scratch and the caller's stream order: the
    plan's state is not disturbed."""
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 2_051, 3, 5e-4
    d = SsgdData(n, R, 0.9)
    buf = SsgdBuffers(d)
    rates = _rates(R)
    st = d.st
    with SmaPlan([0], n) as plan:
        for clock in range(2):
            buf.call(plan, [True] * R, rates, wd, flags)
            d.step([True] * R, rates, wd, keep=flags == 0)
            buf.check(f"clock {clock}:")
        plan.ssgd_step([buf.stream.cuda_stream], [buf.z.ptr], [buf.blast.ptr], [buf.acc.ptr],
                       [(0, buf.w[i].ptr, 1) for i in range(R)], 0.9, R)
        O.ssgd_sync(st, [d.acc], R)
        buf.check("after cbx_ssgd_plan_step:")
        reps = [(0, buf.w[i].ptr, buf.s[i].ptr, 1, 0) for i in range(R)]
        plan.step([buf.stream.cuda_stream], [buf.z.ptr], [buf.blast.ptr], reps, ALPHA, 0.9)
        O.sma_step(st)
        buf.check("after cbx_sma_plan_step:")
        buf.call(plan, [True] * R, rates, wd, flags)
        d.step([True] * R, rates, wd, keep=flags == 0)
        buf.check("the fused call again:")


def test_each_call_adds_one_timing_entry():
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 4099, 3, 5e-4
    d = SsgdData(n, R, 0.9)
    buf = SsgdBuffers(d)
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


# name: keyword arguments of the call, or the position of an array argument passed as NULL
INVALID = {
    "flag_bit_2": dict(flags=2),
    "no_work_per_clock": dict(wpc=0),
    "stepping_unlocked": dict(held=(1,), steps=[True, True, True]),
    "stepping_below_first": dict(first=1, steps=[True, True, True]),
    "null_g_of_a_stepping_replica": dict(g_null=(2,)),
    "null_last_with_base_momentum": dict(null_array=3),
    "null_acc_array": dict(null_array=4),
    "null_g_array": dict(null_array=8),
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
    d = SsgdData(n, R, 0.9, acc_seed=7780)
    d.st.first = kw.pop("first", 0)
    for i in kw.pop("held", ()):
        d.st.locked[i] = 0
    steps, flags, null_array = kw.pop("steps", [True] * R), kw.pop("flags", 0), kw.pop("null_array", None)
    if "wpc" in kw:
        d.wpc = kw.pop("wpc")
    buf = SsgdBuffers(d)
    rates = _rates(R)
    with SmaPlan([0], n) as plan:
        if null_array is None:
            with pytest.raises(CbxError) as e:
                buf.call(plan, steps, rates, wd, flags, **kw)
            assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        else:
            reps = buf.replicas(steps, rates)
            args = [plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), _ptrs([buf.blast.ptr]),
                    _ptrs([buf.acc.ptr]), R, _ints([r[0] for r in reps]), _ptrs([r[1] for r in reps]),
                    _ptrs([r[2] for r in reps]), _ints([r[3] for r in reps]), _ints([r[4] for r in reps]),
                    (ctypes.c_float * R)(*rates), 0.9, wd, R, 0, 0]
            args[null_array] = None
            assert plan.lib.cbx_ssgd_plan_step_and_optimise(*args) == _lib.CBX_ERR_INVALID
        assert "cbx_ssgd_plan_step_and_optimise" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        Buffers.check(buf, "after the refused call:")  # the host mirror never stepped
        buf.acc.check(d.acc, "acc after the refused call")
        d.st.first = 0
        d.st.locked[:] = 1
        d.wpc = R
        buf.call(plan, [True] * R, rates, wd)  # and the plan still works
        d.step([True] * R, rates, wd)
        buf.check("after a good call:")


def test_more_than_64_participating_replicas_is_unsupported():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 1027, 2, 0.0
    d = SsgdData(n, R, 0.0, acc_seed=7781)
    buf = SsgdBuffers(d)
    reps = buf.replicas([True] * R, _rates(R))
    with SmaPlan([0], n) as plan:
        with pytest.raises(CbxError) as e:
            plan.ssgd_step_and_optimise([buf.stream.cuda_stream], [buf.z.ptr], None, [buf.acc.ptr],
                                        [reps[i % R] for i in range(65)], 0.0, wd, R)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        Buffers.check(buf)
        buf.acc.check(d.acc, "acc")
