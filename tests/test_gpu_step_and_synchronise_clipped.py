"""GPU parity of ``cbx_step_and_synchronise_clipped``: the replicas' pending
task steps, clipped by global L2 norm or skipped over a non-finite gradient,
fused into the one-GPU SMA barrier (task_barrier_clipped_kernels.hip).

Expectations come from the host: per stepping replica
``tests.gradient_clip_common.decide`` and ``step``, then ``O.sma_step``.  The
gradients have an exact S in any summation order (small integers and halves on
a few elements, ``exact_gradient``), so S, K, the scale and the flags are known
without the device; the device's own S enters an expectation only in the
normal-data test, after it has passed the reordering bound.  Every comparison is
bit for bit, a NaN only having to be a NaN where the oracle has one.

n = 9,095 = 2 * 4,096 + 903: three norm tiles, the last partial, padded to
12,288 floats; n = 8: one tile, and the norm's last float4 bulk is empty.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact
from tests.test_gpu_step_and_synchronise import ALPHA, DISCARD, REFUSALS, Case, _exp, _gpu, _rates, _snapshot
from tests.test_gpu_step_and_synchronise_variables import SHAPES

pytestmark = pytest.mark.gpu

N = 9_095
PADDED = 12_288
ZERO = {"sum_sq": 0.0, "nonfinite": 0, "scale": 0.0, "flags": 0, "steps": 0, "clipped_steps": 0, "skipped_steps": 0}
_, _, MAX_NORM = C.exact_gradient(N)  # every exact gradient below is made for this max_norm


def gradient(n, kind, i):
    """A gradient whose S is exact in any order, for a context clipping at
    ``exact_gradient(n)``'s max_norm: "clipped" has scale exactly 0.5,
    "unclipped" a quarter of those values (S = c^2 / 4: scale 1), "skipped" the
    clipped one with a NaN and an infinity in it.  Replica i's is rolled by 3 i."""
    g, S, c = C.exact_gradient(n)
    g = np.roll(g, 3 * i)
    if kind == "unclipped":
        g = g * np.float32(0.25)
    elif kind == "skipped":
        for p, v in zip(C.nonfinite_positions(n), (np.nan, np.inf, -np.inf)):
            g[p] = v
    return np.ascontiguousarray(g, np.float32)


class ClipCase(Case):
    """tests/test_gpu_step_and_synchronise.py's mirror with the clipped step."""

    def set_gradients(self, kinds):
        self.g = [gradient(self.n, k if k != "join" else "unclipped", i) for i, k in enumerate(kinds)]

    def step(self, tasks, rates, wd, c, skip, keep=True, sums=None):
        """The two-call sequence.  sums[i] = (S, K) where the host's exact pair is not to be used."""
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if tasks[i] >= 0 and not keep}
        self.decision = {}
        for i in range(self.R):
            if tasks[i] < 0:
                continue
            S, K = sums[i] if sums else C.exact_sum_sq(self.g[i])
            scale, flags = C.decide(S, K, c, skip)
            self.decision[i] = (S, K, float(scale), flags)
            C.step([st.w[i], self.g[i], self.last[i], st.s[i]], scale, flags, self.momentum, wd, lr=rates[i])
        with np.errstate(all="ignore"):
            O.sma_step(st)
        for i, (s, g) in kept.items():  # the device left them alone: so does the mirror, for the clocks to come
            st.s[i], self.g[i] = s, g
        self.dev_s, self.dev_g = st.s, self.g

    def check(self, gpu, what=""):
        from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
        st, same = self.st, C.assert_same_with_nans
        same(gpu.base_read(0, BUF_DATA), st.z[0], f"{what} z")
        if st.last is not None:
            same(gpu.base_read(0, BUF_LAST), st.last[0], f"{what} base last")
        for i in range(self.R):
            same(gpu.replica_read(i, BUF_DATA), st.w[i], f"{what} w[{i}]")
            same(gpu.replica_read(i, BUF_DIFF), self.dev_s[i], f"{what} s[{i}]")
            same(gpu.replica_read(i, BUF_GRADIENT), self.dev_g[i], f"{what} g[{i}]")
            if self.last[i] is not None:
                same(gpu.replica_read(i, BUF_LAST), self.last[i], f"{what} last[{i}]")
        for a in (st.z[0], *st.w):
            assert np.count_nonzero(np.isnan(a)) * 4 <= a.size  # at most a quarter of a compared array is NaN

    def check_records(self, gpu, counts, what=""):
        """counts[i] = (steps, clipped_steps, skipped_steps) expected so far."""
        for i in range(self.R):
            rec = gpu.replica_clip_stats(i)
            assert (rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == tuple(counts[i]), (what, i, rec)
            if i in self.decision:
                S, K, scale, flags = self.decision[i]
                assert (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"]) == (S, K, scale, flags), (what, i, rec)


def _clipped(gpu, first, clock, tasks, streams=None, flags=0):
    gpu.lockAny()
    gpu.step_and_synchronise_clipped(first, clock, 0, tasks, streams, flags)
    gpu.unlockAny()


def _count(counts, case):
    for i, (_, _, _, flags) in case.decision.items():
        counts[i][0] += 1
        counts[i][1] += 1 if flags & C.CLIPPED else 0
        counts[i][2] += 1 if flags & C.SKIPPED else 0


def _mixes(R):
    """Lists of outcomes per replica: all of them stepping (the unrolled and the
    chunked all-step kernels), and some only joining (the mixed kernel).  At
    R = 9 replica 8, the second chunk's, is skipped in both."""
    if R == 1:
        return [["clipped"], ["skipped"], ["unclipped"]]
    every = [("unclipped", "clipped", "skipped")[i % 3] for i in range(R)]
    some = [("join", "clipped", "skipped", "unclipped")[i % 4] for i in range(R)]
    if R == 9:
        some[8] = "skipped"
    assert "skipped" in every and "join" in some and "skipped" in some and (R != 9 or every[8] == "skipped")
    return [every, some]


# ---- the matrix ----------------------------------------------------------------
# One context per (R, momentum, weight decay); the launch shapes, the flags and
# the outcome mixes run on it one after the other, each from freshly uploaded buffers.
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [1, 3, 8, 9])
def test_outcome_mix(R, momentum, wd):
    all_tasks = [3 + 2 * i for i in range(R)]
    all_rates = _rates(_exp, R, all_tasks, momentum)
    gpu = _gpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        clock, counts = 0, [[0, 0, 0] for _ in range(R)]
        for shape in SHAPES:
            gpu.set_task_barrier_kernel_config(*shape)
            for flags in (0, DISCARD):
                for kinds in _mixes(R):
                    tasks = [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]
                    case = ClipCase(N, R, momentum)
                    case.set_gradients(kinds)
                    case.upload(gpu)
                    clock += 1
                    _clipped(gpu, 0, clock, tasks, None, flags)
                    gpu.wait()
                    case.step(tasks, all_rates, wd, MAX_NORM, True, keep=flags == 0)
                    what = f"shape {shape} flags {flags} {kinds}:"
                    for i, k in enumerate(kinds):  # the host's decisions are the outcomes the mix names
                        if k == "skipped":
                            assert case.decision[i][3] == C.CLIPPED | C.SKIPPED, (what, i, case.decision[i])
                        elif k != "join":
                            want = (1.0, 0) if k == "unclipped" else (0.5, C.CLIPPED)
                            assert case.decision[i][2:] == want, (what, i, case.decision[i])
                    case.check(gpu, what)
                    _count(counts, case)
                    case.check_records(gpu, counts, what)
                    assert [gpu.replica_clock(i) for i in range(R)] == [clock] * R
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("kinds", [["unclipped", "clipped", "skipped"], ["join", "skipped", "clipped"],
                                   ["skipped", "skipped", "skipped"], ["join", "join", "join"]])
def test_one_tile_and_an_empty_float4_bulk_in_the_norm(kinds, flags):
    n, R, momentum, wd = 8, 3, 0.9, 1e-4
    _, _, c = C.exact_gradient(n)
    all_tasks = [3, 5, 7]
    rates = _rates(_exp, R, all_tasks, momentum)
    tasks = [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]
    case = ClipCase(n, R, momentum)
    case.set_gradients(kinds)
    gpu = _gpu(n, R, momentum, wd)
    try:
        gpu.set_gradient_clip(c, True)
        case.upload(gpu)
        _clipped(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, c, True, keep=flags == 0)
        case.check(gpu)
        counts = [[0, 0, 0] for _ in range(R)]
        _count(counts, case)
        case.check_records(gpu, counts)
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("kinds", [["skipped"] * 3, ["join"] * 3])
def test_all_skipped_and_all_join(kinds, flags):
    R, momentum, wd = 3, 0.9, 1e-4
    all_tasks = [3, 5, 7]
    rates = _rates(_exp, R, all_tasks, momentum)
    tasks = [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]
    case = ClipCase(N, R, momentum)
    case.set_gradients(kinds)
    gpu = _gpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        case.upload(gpu)
        before = _snapshot(gpu, R, momentum)[0]
        _clipped(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, MAX_NORM, True, keep=flags == 0)
        case.check(gpu)
        counts = [[0, 0, 0] for _ in range(R)]
        _count(counts, case)
        case.check_records(gpu, counts)
        if kinds[0] == "join":
            assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R  # no norm was launched
        else:  # the steps moved nothing: g and last keep every bit, NaN and infinity included
            after = _snapshot(gpu, R, momentum)[0]
            for i in range(R):
                for name in ("g", "last"):
                    assert np.array_equal(after[f"{name}[{i}]"].view(np.uint32), before[f"{name}[{i}]"].view(np.uint32)), (name, i)
    finally:
        gpu.free()


# ---- the records against the sequence's, all 48 bytes ---------------------------------
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_records_equal_the_sequences_over_three_clocks(momentum):
    from crossbow_amd import BUF_GRADIENT
    R, wd = 4, 1e-4
    gpu, twin = _gpu(N, R, momentum, wd), _gpu(N, R, momentum, wd)
    plan = [(["clipped", "skipped", "unclipped", "join"], [0, 1, 2, -1]),
            (["skipped", "join", "clipped", "clipped"], [4, -1, 5, 6]),
            (["unclipped", "clipped", "skipped", "skipped"], [7, 8, 9, 10])]
    try:
        for g in (gpu, twin):
            g.set_gradient_clip(MAX_NORM, True)
        case = ClipCase(N, R, momentum)
        case.upload(gpu)
        case.upload(twin)
        steps = [[0, 0, 0] for _ in range(R)]
        for clock, (kinds, tasks) in enumerate(plan, 1):
            case.set_gradients(kinds)
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            _clipped(gpu, 0, clock, tasks)
            for i in range(R):
                if tasks[i] >= 0:
                    twin.replica_optimise(i, tasks[i])
            twin.lockAny()
            twin.synchronise(0, clock, 0, False)
            twin.unlockAny()
            gpu.wait()
            twin.wait()
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                assert np.array_equal(a[0][key].view(np.uint32), b[0][key].view(np.uint32)), f"clock {clock}: {key}"
            assert a[1:] == b[1:]
            for i, k in enumerate(kinds):
                if k != "join":
                    steps[i][0] += 1
                    steps[i][1] += k != "unclipped"
                    steps[i][2] += k == "skipped"
            for i in range(R):
                rec = gpu.replica_clip_stats(i)
                assert rec == twin.replica_clip_stats(i), (clock, i)
                assert [rec["steps"], rec["clipped_steps"], rec["skipped_steps"]] == steps[i], (clock, i, rec)
    finally:
        gpu.free()
        twin.free()


# ---- normal data; a non-finite gradient with the skip off --------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("nonfinite", [False, True])
def test_normal_data_and_a_nonfinite_gradient_with_the_skip_off(nonfinite, flags):
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    case = ClipCase(N, R, momentum)  # gradients of normal data, sigma 0.01
    c = float(np.float32(0.25 * np.sqrt(C.exact_sum_sq(case.g[0])[0])))  # clips to about a quarter of the norm
    gpu = _gpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(c, False)
        case.upload(gpu)
        for clock, tasks in ((1, [3, 5, 7]), (2, [4, 6, 8])):
            rates = _rates(_exp, R, tasks, momentum)
            if clock == 2:  # every replica steps again, on a fresh finite gradient
                for i in range(R):
                    case.g[i] = O.fill_normal(N, 7000 + i, 0.01)
                    gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            elif nonfinite:
                for p, v in zip(C.nonfinite_positions(N), (np.nan, np.inf, -np.inf)):
                    case.g[1][p] = v
                gpu.replica_write(1, BUF_GRADIENT, case.g[1])
            exact = [C.exact_sum_sq(g) for g in case.g]
            _clipped(gpu, 0, clock, tasks, None, flags)
            gpu.wait()
            sums = []
            for i in range(R):
                rec = gpu.replica_clip_stats(i)
                S_ref, K = exact[i]
                assert rec["nonfinite"] == K == (3 if nonfinite and i == 1 and clock == 1 else 0)
                # the reordering bound of a sum of n non-negative terms in fp64, then the device's S may be used
                assert abs(rec["sum_sq"] - S_ref) <= 2 * N * 2.0 ** -53 * S_ref, (i, rec["sum_sq"], S_ref)
                sums.append((rec["sum_sq"], K))
            case.step(tasks, rates, wd, c, False, keep=flags == 0, sums=sums)
            assert all(d[3] == C.CLIPPED for d in case.decision.values())
            if nonfinite:
                # S and K are taken over the finite values and the step is not skipped: the NaN is in
                # w[1] after the first clock, and through s = w in z after the second
                assert np.isnan(case.st.w[1][0]) and not np.isnan(case.st.w[0][0])
                assert np.isnan(case.st.z[0][0]) == (clock == 2)
            case.check(gpu, f"clock {clock}:")
            case.check_records(gpu, [[clock, clock, 0]] * R)
    finally:
        gpu.free()


# ---- clipping off: the plain call ----------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
def test_with_clipping_off_it_is_the_plain_call(flags):
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    gpu, twin = _gpu(N, R, momentum, wd), _gpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(1.0, True)
        gpu.set_gradient_clip(0.0, False)  # on, then off again
        for g in (gpu, twin):
            g.set_timing(True)
        case = Case(N, R, momentum)
        case.upload(gpu)
        case.upload(twin)
        for k in range(2):
            tasks = [3 * k, 3 * k + 1, 3 * k + 2]
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            _clipped(gpu, 0, k + 1, tasks, None, flags)
            twin.lockAny()
            twin.step_and_synchronise(0, k + 1, 0, tasks, None, flags)
            twin.unlockAny()
            gpu.wait()
            twin.wait()
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                assert_bitexact(a[0][key], b[0][key], f"{key} against cbx_step_and_synchronise")
            assert a[1:] == b[1:]
            assert len(gpu.timing_history()) == k + 1  # one timing entry per call
            assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
    finally:
        gpu.free()
        twin.free()


# ---- Phase D beside a skipped replica ---------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("how", ["set_beforehand", "raised_by_this_call"])
def test_phase_d(how, flags):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST
    R, momentum, wd = 3, 0.9, 1e-4
    kinds = ["clipped", "unclipped", "skipped"]
    if how == "set_beforehand":
        policy, tasks = _exp, [4, 6, 8]
    else:  # replica 1 crosses the boundary at the task that is passed: (task + 1) >= 3
        def policy(g):
            g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
        tasks = [0, 2, 1]
    case = ClipCase(N, R, momentum)
    case.set_gradients(kinds)
    gpu = _gpu(N, R, momentum, wd, policy)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        case.upload(gpu)
        if how == "set_beforehand":
            gpu.set_replica_copy(1, True)
        rates = _rates(policy, R, tasks, momentum)
        if how == "raised_by_this_call":
            assert rates == pytest.approx([0.1, 0.05, 0.1])
            assert [gpu.replica_copy(i) for i in range(R)] == [0, 0, 0]
        case.st.copy[1] = 1
        g2, last2 = case.g[2].copy(), case.last[2].copy()
        _clipped(gpu, 0, 7, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, MAX_NORM, True, keep=flags == 0)
        case.check(gpu)
        z = gpu.base_read(0, BUF_DATA)
        for i in range(R):  # the skipped replica's w becomes z as well
            assert_bitexact(gpu.replica_read(i, BUF_DATA), z, f"w[{i}] == the new z")
        assert np.array_equal(gpu.replica_read(2, BUF_GRADIENT).view(np.uint32), g2.view(np.uint32)), "g of the skipped replica"
        assert_bitexact(gpu.replica_read(2, BUF_LAST), last2, "last of the skipped replica")
        assert [gpu.replica_copy(i) for i in range(R)] == [0] * R
        assert [gpu.replica_clock(i) for i in range(R)] == [7] * R
    finally:
        gpu.free()


# ---- task streams ------------------------------------------------------------------------------
def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    return hip


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_gradients_and_norms_on_two_caller_streams(flags):
    # The gradients arrive on two caller streams; the norm passes go on those
    # streams and the launch behind them.  Until then g holds another gradient.
    import torch
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    kinds, tasks = ["clipped", "skipped", "unclipped"], [2, 4, 6]
    rates = _rates(_exp, R, tasks, momentum)
    gpu, same = _gpu(N, R, momentum, wd), _gpu(N, R, momentum, wd)
    hip = _hip()
    try:
        case = ClipCase(N, R, momentum)
        case.set_gradients(kinds)
        fresh = [torch.from_numpy(g).cuda() for g in case.g]
        for g in (gpu, same):
            g.set_gradient_clip(MAX_NORM, True)
            case.upload(g)
        stale = np.full(N, 3.0, np.float32)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, stale)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for i in range(R):
            assert hip.hipMemcpyAsync(gpu.replica_buffer(i, BUF_GRADIENT), fresh[i].data_ptr(), 4 * N, 3,
                                      streams[i % 2].cuda_stream) == 0  # device to device
        _clipped(gpu, 0, 1, tasks, [streams[i % 2].cuda_stream for i in range(R)], flags)
        _clipped(same, 0, 1, tasks, None, flags)
        gpu.wait()
        same.wait()
        torch.cuda.synchronize()
        a, b = _snapshot(gpu, R, momentum), _snapshot(same, R, momentum)
        for key in a[0]:
            assert np.array_equal(a[0][key].view(np.uint32), b[0][key].view(np.uint32)), f"{key} against the same-stream run"
        assert [gpu.replica_clip_stats(i) for i in range(R)] == [same.replica_clip_stats(i) for i in range(R)]
        case.step(tasks, rates, wd, MAX_NORM, True, keep=flags == 0)
        case.check(gpu)
        case.check_records(gpu, [[1, 1, 0], [1, 1, 1], [1, 0, 0]])
    finally:
        torch.cuda.synchronize()
        gpu.free()
        same.free()


# ---- the pad ---------------------------------------------------------------------------------------
def test_the_pad_of_the_gradient_is_never_read():
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 2, 0.9, 1e-4
    tasks = [3, 5]
    rates = _rates(_exp, R, tasks, momentum)
    gpu, clean = _gpu(N, R, momentum, wd), _gpu(N, R, momentum, wd)
    hip = _hip()
    try:
        case = ClipCase(N, R, momentum)  # normal data: a pad of 1e30 in the sum would move S by 1e60
        exact = [C.exact_sum_sq(g) for g in case.g]
        c = float(np.float32(0.25 * np.sqrt(exact[0][0])))
        for g in (gpu, clean):
            g.set_gradient_clip(c, True)
            case.upload(g)
        pad = np.full(PADDED - N, 1e30, np.float32)
        assert pad.size == 3_193
        for i in range(R):
            assert hip.hipMemcpy(gpu.replica_buffer(i, BUF_GRADIENT) + 4 * N, pad.ctypes.data, pad.nbytes, 1) == 0
        _clipped(gpu, 0, 1, tasks)
        _clipped(clean, 0, 1, tasks)
        gpu.wait()
        clean.wait()
        sums = []
        for i in range(R):
            rec = gpu.replica_clip_stats(i)
            assert rec == clean.replica_clip_stats(i), i  # the S bits are the zero pad's
            assert abs(rec["sum_sq"] - exact[i][0]) <= 2 * N * 2.0 ** -53 * exact[i][0]
            sums.append((rec["sum_sq"], 0))
        case.step(tasks, rates, wd, c, True, sums=sums)
        case.check(gpu)  # [0, n) is the oracle's
    finally:
        gpu.free()  # the pad no longer holds zeros: the context ends here
        clean.free()


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in REFUSALS if k != "clipping"])
def test_refusals_change_nothing(name):
    # the plain call's table but its clipping entry, with clipping on; "variable_rates" is the
    # per-variable refusal, which this call keeps
    from crossbow_amd import CbxError, TheGPU, _lib
    from tests.test_gpu_step_and_synchronise import _two_variables
    code, kw, after, call = REFUSALS[name]
    n, R, momentum, wd, wpc = 4_099, 3, 0.9, 5e-4, 3
    update_type = kw.get("update_type", 7)
    gpu = TheGPU()
    gpu.init([0])
    try:
        if kw.get("two_variables"):
            _two_variables(gpu, n)
        else:
            gpu.setModel(1, 4 * n)
            gpu.setModelVariable(0, 1, [n], 4 * n)
        gpu.setModelWorkPerClock(wpc)
        gpu.setUpdateModelType(update_type)
        if kw.get("elastic"):
            gpu.setElasticAverage(True)
        gpu.setEamsgdAlpha(ALPHA)
        gpu.setMomentum(momentum, kw.get("method", 0))
        gpu.setWeightDecay(wd)
        _exp(gpu)
        gpu.setModelManager(R, kw.get("sync", 0))
        gpu.set_gradient_clip(1.0, True)
        if after:
            after(gpu)
        case = Case(n, R, momentum)
        case.upload(gpu)
        if update_type in (3, 7) and not kw.get("method") and not kw.get("two_variables"):
            gpu.replica_optimise(1, 0)  # a record that is not all zeros: one clipped step behind replica 1
            gpu.wait()
        gpu.set_replica_copy(0, True)  # a flag the refused call must leave raised
        before = _snapshot(gpu, R, momentum)
        records = [gpu.replica_clip_stats(i) for i in range(R)]
        hold = kw.get("hold")
        if hold is not None:
            gpu.replica_lock(hold)
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise_clipped(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_clipped(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_step_and_synchronise_clipped" in _lib.last_error(), _lib.last_error()
        if name == "variable_rates":  # the reason names the two-call sequence
            assert "cbx_replica_optimise and cbx_synchronise" in _lib.last_error(), _lib.last_error()
        gpu.wait()
        after_call = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after_call[0][key], before[0][key], f"{key} after the refused call")
        assert after_call[1:] == before[1:], "copy flags and clocks after the refused call"
        assert [gpu.replica_clip_stats(i) for i in range(R)] == records, "no counter was bumped"
        gpu.unlockAny()
        if hold is not None:
            gpu.replica_unlock(hold)
    finally:
        gpu.free()


def test_the_plain_calls_still_refuse_clipping():
    from crossbow_amd import CbxError, _lib
    gpu = _gpu(N, 3, 0.9, 1e-4)
    try:
        gpu.set_gradient_clip(1.0, False)
        gpu.lockAny()
        for call in (gpu.step_and_synchronise, gpu.step_and_synchronise_variables):
            with pytest.raises(CbxError) as e:
                call(0, 1, 0, [3, 4, 5], None, 0)
            assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
        gpu.unlockAny()
    finally:
        gpu.free()
