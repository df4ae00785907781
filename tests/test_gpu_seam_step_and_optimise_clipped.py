"""The sma.c seam for the fused task steps with gradient clipping:
cbx_sma_plan_step_and_optimise_clipped over buffers the CALLER owns
(include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip, the TAIL
instantiations of task_barrier_clipped_kernels.hip), on one GPU.

Expected values come from the host only: per stepping replica in id order
``tests.gradient_clip_common.decide`` and ``step`` over gradients whose S is
exact in any order (tests/test_gpu_step_and_synchronise_clipped.py's), then
``O.sma_step``.  Every comparison is bit for bit over z, the base ``last``, and
``w``, ``last``, ``s`` and ``g`` of every replica; each device buffer holds
exactly n floats in front of 1,088 sentinel floats that must come back
untouched (tests/helpers.py, Guarded).  The records are compared with those a
second plan holds after the two-call sequence.

Sizes: 1 (one tail float), 771 (an empty bulk), 1,029 (one chunk and 5 tail
floats), 9,095 (8 chunks, 903 tail floats, three norm tiles) and 21,523 (21
chunks, 19 tail floats).  The exact gradients spread their values over the whole
buffer, so the clipped and the skipped replica have work in the bulk and in
the tail.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.helpers import GUARD
from tests.test_gpu_seam_step_and_optimise import ALPHA, CONFIGS, DISCARD, Buffers, Data, _rates
from tests.test_gpu_step_and_synchronise_clipped import gradient

pytestmark = pytest.mark.gpu

assert GUARD == 1088
SIZES = [1, 771, 1_029, 9_095, 21_523]
CONFIGS = dict(CONFIGS, **{"mom-only": (0.9, 0.0, 0.9)})
KINDS = {1: ["clipped"], 4: ["clipped", "skipped", "unclipped", "join"],
         8: ["unclipped", "clipped", "skipped"] * 2 + ["clipped", "skipped"],
         9: ["unclipped", "join", "skipped", "clipped"] * 2 + ["skipped"]}


class ClipData(Data):
    def __init__(self, n, kinds, rmom, bmom):
        super().__init__(n, len(kinds), rmom, bmom)
        self.kinds = kinds
        self.g = [gradient(n, k if k != "join" else "unclipped", i) for i, k in enumerate(kinds)]
        self.max_norm = C.exact_gradient(n)[2]
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
                C.step([st.w[i], self.g[i], self.last[i], st.s[i]], scale, flags, self.rmom, wd, lr=rates[i])
        copies = O.sma_step(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g
        return 1 if copies > 0 else 0


class ClipBuffers(Buffers):
    def call(self, plan, steps, rates, wd, flags=0, slots="own", c=None, skip=True, **nulls):
        st, d = self.d.st, self.d
        return plan.step_and_optimise_clipped([self.stream.cuda_stream], [self.z.ptr],
                                              [self.blast.ptr] if self.blast is not None else None,
                                              self.replicas(steps, rates, **nulls), ALPHA, st.momentum, d.rmom, wd,
                                              st.first, flags, slots=d.slots if slots == "own" else slots,
                                              max_norm=d.max_norm if c is None else c, skip_nonfinite=skip)

    def sequence(self, plan, steps, rates, wd, c=None, skip=True):
        """The two-call sequence of the header on these buffers."""
        d, st = self.d, self.d.st
        for i in range(d.R):
            if steps[i]:
                plan.optimise_clipped(0, d.slots[i], self.stream.cuda_stream, self.w[i].ptr, self.g[i].ptr,
                                      self.last[i].ptr if self.last[i] is not None else None, self.s[i].ptr, rates[i],
                                      d.rmom, wd, d.max_norm if c is None else c, skip)
        reps = [(0, self.w[i].ptr, self.s[i].ptr, int(st.locked[i]), int(st.copy[i])) for i in range(d.R)]
        return plan.step([self.stream.cuda_stream], [self.z.ptr], [self.blast.ptr] if self.blast is not None else None,
                         reps, ALPHA, st.momentum, st.first)


def _records(plan, buf, d):
    return [plan.clip_stats(0, d.slots[i], buf.stream.cuda_stream) for i in range(d.R)]


def _run(n, R, config, flags, copies=()):
    from crossbow_amd.seam import SmaPlan
    rmom, wd, bmom = CONFIGS[config]
    kinds = KINDS[R]
    d, twin = ClipData(n, kinds, rmom, bmom), ClipData(n, kinds, rmom, bmom)
    for i in copies:
        d.st.copy[i] = twin.st.copy[i] = 1
    rates = _rates(R)
    buf, seq = ClipBuffers(d), ClipBuffers(twin)
    with SmaPlan([0], n) as plan, SmaPlan([0], n) as second:
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


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("R", [1, 4, 8, 9])
@pytest.mark.parametrize("n", SIZES)
def test_every_buffer_and_record_bitexact(n, R, config, flags):
    _run(n, R, config, flags)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [1, 1_029, 9_095])
def test_phase_d_beside_a_skipped_replica(n, flags):
    from tests.helpers import assert_bitexact
    R = 4  # a copy flag on the skipped replica (1) and on the one that only joins (3)
    buf, got = _run(n, R, "mom-wd", flags, copies=(1, 3))
    assert got == 1
    z = buf.z.t.cpu().numpy()[:n]
    for i in range(R):
        assert_bitexact(buf.w[i].t.cpu().numpy()[:n], z, f"w[{i}] == the new z, tail included")


@pytest.mark.parametrize("c,skip", [(0.0, False), (0.0, True), (1e30, False)])
def test_a_max_norm_of_zero_and_no_skip_still_reduce_and_count(c, skip):
    from crossbow_amd.seam import SmaPlan
    n, R, (rmom, wd, bmom) = 1_029, 3, CONFIGS["mom-wd"]
    d = ClipData(n, ["clipped", "unclipped", "clipped"], rmom, bmom)  # finite gradients: nothing to skip
    rates = _rates(R)
    buf = ClipBuffers(d)
    with SmaPlan([0], n) as plan:
        for clock in (1, 2):
            buf.call(plan, d.steps, rates, wd, c=c, skip=skip)
            d.step(d.steps, rates, wd, c=c, skip=skip)
            buf.check(f"clock {clock}:")
            for i, rec in enumerate(_records(plan, buf, d)):
                want = dict(d.decision[i], steps=clock, clipped_steps=0, skipped_steps=0)
                if clock == 2:  # g is the first step's output now: its S is exact in one order only
                    assert abs(rec["sum_sq"] - want["sum_sq"]) <= 2 * n * 2.0 ** -53 * want["sum_sq"]
                    want["sum_sq"] = rec["sum_sq"]
                assert rec == want, (clock, i, rec)
                assert rec["scale"] == 1.0 and rec["flags"] == 0


# ---- refusals ----------------------------------------------------------------------------------------
BAD_SLOTS = {
    "null_slots_with_a_stepping_replica": None,
    "slot_minus_1": [0, -1, 2],
    "slot_64": [0, 1, 64],
    "two_stepping_replicas_share_a_slot": [3, 9, 3],
}


@pytest.mark.parametrize("name", list(BAD_SLOTS))
def test_slot_refusals_write_nothing_and_bump_no_counter(name):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n, R, (rmom, wd, bmom) = 1_029, 3, CONFIGS["mom-wd"]
    d = ClipData(n, ["clipped", "skipped", "unclipped"], rmom, bmom)
    d.slots = [0, 1, 2]
    rates = _rates(R)
    buf = ClipBuffers(d)
    with SmaPlan([0], n) as plan:
        zero = _records(plan, buf, d)  # allocates the three slots: all zeros
        assert all(not any(rec.values()) for rec in zero)
        with pytest.raises(CbxError) as e:
            buf.call(plan, d.steps, rates, wd, slots=BAD_SLOTS[name])
        assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        assert "cbx_sma_plan_step_and_optimise_clipped" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        assert _records(plan, buf, d) == zero
        # a replica that does not step needs no slot, and may name one that another uses
        d.kinds = ["clipped", "skipped", "join"]
        d.steps = [True, True, False]
        buf.call(plan, d.steps, rates, wd, slots=[0, 1, 77])
        d.step(d.steps, rates, wd)
        buf.check("after a good call:")


@pytest.mark.parametrize("what", ["max_norm_negative", "max_norm_nan", "max_norm_inf", "skip_2"])
def test_bad_clip_arguments_are_refused(what):
    import torch

    from crossbow_amd import _lib
    from crossbow_amd.seam import SmaPlan, _ints, _ptrs
    n, R, (rmom, wd, bmom) = 771, 2, CONFIGS["mom-wd"]
    d = ClipData(n, ["clipped", "skipped"], rmom, bmom)
    buf = ClipBuffers(d)
    reps = buf.replicas(d.steps, _rates(R))
    c = {"max_norm_negative": -1.0, "max_norm_nan": float("nan"), "max_norm_inf": float("inf")}.get(what, 1.0)
    with SmaPlan([0], n) as plan:
        rc = plan.lib.cbx_sma_plan_step_and_optimise_clipped(
            plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), _ptrs([buf.blast.ptr]), R,
            _ints([r[0] for r in reps]), _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]),
            _ptrs([r[3] for r in reps]), _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]),
            _ints([r[6] for r in reps]), _ints([r[7] for r in reps]), (ctypes.c_float * R)(*_rates(R)),
            _ints(d.slots), ctypes.c_float(c), 2 if what == "skip_2" else 1, ALPHA, 0.9, rmom, wd, 0, 0)
        assert rc == _lib.CBX_ERR_INVALID, _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")
        assert all(not any(rec.values()) for rec in _records(plan, buf, d))
