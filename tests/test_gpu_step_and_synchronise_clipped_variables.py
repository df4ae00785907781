"""GPU parity of ``cbx_step_and_synchronise_clipped_variables``: the replicas'
pending task steps, clipped by global L2 norm (or skipped over a non-finite
gradient) and with a learning rate per variable, fused into the one-GPU SMA
barrier (task_barrier_clipped_variables_kernels.hip).

Expectations come from the host, never from a device result: per stepping
replica ``tests.gradient_clip_common.decide`` and ``step(..., variables=,
mults=)``, then ``O.sma_step``.  The gradients have an exact S in any summation
order and are non-zero in every variable (tests/clipped_variables_common.py),
so S, K, the scale and the flags are known without the device and every
variable sees its multiplier in every (momentum, weight decay) cell.  Every
comparison is bit for bit, a NaN only having to be a NaN where the oracle has
one, and at most a quarter of a compared array is NaN.

The model is ``V``, ``M`` of tests/test_optimise_plan.py: n = 21,523 = 5 * 4,096
+ 1,043 (six norm tiles, the last partial) padded to 24,576, boundaries inside
float4s and inside chunks; and n = 8 as two variables (3, 5): one norm tile, an
empty float4 bulk in the norm, a boundary inside a float4.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import clipped_variables_common as CV
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact
from tests.test_gpu_step_and_synchronise import DISCARD, REFUSALS, _exp, _rates, _snapshot
from tests.test_gpu_step_and_synchronise_clipped import ZERO, ClipCase, _count, _mixes
from tests.test_gpu_step_and_synchronise_variables import PADDED, SHAPES, _gpu
from tests.test_optimise_plan import M, V

pytestmark = pytest.mark.gpu

N = CV.N
MAX_NORM = CV.MAX_NORM
V8, M8 = (3, 5), (2.0, 0.5)


class Both(ClipCase):
    """tests/test_gpu_step_and_synchronise_clipped.py's mirror, stepping per variable."""

    def __init__(self, R, momentum, variables=V, mults=M):
        super().__init__(sum(variables), R, momentum)
        self.variables, self.mults = variables, mults

    def set_gradients(self, kinds):
        self.g = [CV.gradient(self.n, k if k != "join" else "unclipped", i, self.variables)
                  for i, k in enumerate(kinds)]

    def step(self, tasks, rates, wd, c, skip, keep=True, mults=None):
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if tasks[i] >= 0 and not keep}
        self.decision = {}
        for i in range(self.R):
            if tasks[i] < 0:
                continue
            S, K = C.exact_sum_sq(self.g[i])
            scale, flags = C.decide(S, K, c, skip)
            self.decision[i] = (S, K, float(scale), flags)
            C.step([st.w[i], self.g[i], self.last[i], st.s[i]], scale, flags, self.momentum, wd, lr=rates[i],
                   variables=self.variables, mults=mults or self.mults)
        with np.errstate(all="ignore"):
            O.sma_step(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g
        self.dev_s, self.dev_g = st.s, self.g


def _both(gpu, first, clock, tasks, streams=None, flags=0):
    gpu.lockAny()
    gpu.step_and_synchronise_clipped_variables(first, clock, 0, tasks, streams, flags)
    gpu.unlockAny()


def _clipping(R, momentum, wd, c=MAX_NORM, skip=True, **kw):
    gpu = _gpu(R, momentum, wd, **kw)
    gpu.set_gradient_clip(c, skip)
    return gpu


def _check_outcomes(case, kinds, what):
    for i, k in enumerate(kinds):  # the host's decisions are the outcomes the mix names
        if k == "skipped":
            assert case.decision[i][3] == C.CLIPPED | C.SKIPPED, (what, i, case.decision[i])
        elif k != "join":
            want = (1.0, 0) if k == "unclipped" else (0.5, C.CLIPPED)
            assert case.decision[i][2:] == want, (what, i, case.decision[i])


# ---- the host-only guard --------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_the_multipliers_show_in_every_variable_on_the_host(momentum, wd):
    # with every multiplier forced to 1 the expected w differs in every variable of V whose multiplier is
    # not 1 (V's variables 1 and 4 have multiplier 1 and must not differ): the matrix below is no test of the
    # clipped kernel alone
    CV.multipliers_show(V, M, momentum, wd)
    CV.multipliers_show(V8, M8, momentum, wd)


# ---- the matrix ----------------------------------------------------------------
# One context per (R, momentum, weight decay); the launch shapes, the flags and
# the outcome mixes run on it one after the other, each from freshly uploaded buffers.
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [1, 3, 8, 9])
def test_outcome_mix(R, momentum, wd):
    all_tasks = [3 + 2 * i for i in range(R)]
    all_rates = _rates(_exp, R, all_tasks, momentum)
    gpu = _clipping(R, momentum, wd)
    try:
        clock, counts = 0, [[0, 0, 0] for _ in range(R)]
        for shape in SHAPES:
            gpu.set_task_barrier_kernel_config(*shape)
            for flags in (0, DISCARD):
                for kinds in _mixes(R):
                    tasks = [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]
                    case = Both(R, momentum)
                    case.set_gradients(kinds)
                    case.upload(gpu)
                    clock += 1
                    _both(gpu, 0, clock, tasks, None, flags)
                    gpu.wait()
                    case.step(tasks, all_rates, wd, MAX_NORM, True, keep=flags == 0)
                    what = f"shape {shape} flags {flags} {kinds}:"
                    _check_outcomes(case, kinds, what)
                    case.check(gpu, what)
                    _count(counts, case)
                    case.check_records(gpu, counts, what)
                    assert [gpu.replica_clock(i) for i in range(R)] == [clock] * R
    finally:
        gpu.free()


def test_the_result_differs_from_the_clipped_calls_expectation():
    # the same call held to the expectation of cbx_step_and_synchronise_clipped (every multiplier 1) fails
    R, momentum, wd = 3, 0.0, 0.0
    kinds, tasks = ["unclipped", "clipped", "skipped"], [3, 5, 7]
    rates = _rates(_exp, R, tasks, momentum)
    gpu = _clipping(R, momentum, wd)
    try:
        case = Both(R, momentum)
        case.set_gradients(kinds)
        case.upload(gpu)
        _both(gpu, 0, 1, tasks)
        gpu.wait()
        case.step(tasks, rates, wd, MAX_NORM, True, mults=(1.0,) * len(V))
        with pytest.raises(AssertionError):
            case.check(gpu)
        from crossbow_amd import BUF_DATA
        for i in (0, 1):
            got, lo = gpu.replica_read(i, BUF_DATA), 0
            for v, count in enumerate(V):
                same = np.array_equal(got[lo:lo + count].view(np.uint32), case.st.w[i][lo:lo + count].view(np.uint32))
                assert same == (M[v] == 1.0), (i, v)
                lo += count
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("kinds", [["unclipped", "clipped", "skipped"], ["join", "skipped", "clipped"],
                                   ["skipped", "skipped", "skipped"], ["join", "join", "join"]])
def test_eight_floats_as_two_variables(kinds, flags):
    R, momentum, wd = 3, 0.9, 1e-4
    _, _, c = CV.dense_gradient(8)
    all_tasks = [3, 5, 7]
    rates = _rates(_exp, R, all_tasks, momentum)
    tasks = [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]
    case = Both(R, momentum, V8, M8)
    case.set_gradients(kinds)
    gpu = _clipping(R, momentum, wd, c, variables=V8, mults=M8)
    try:
        case.upload(gpu)
        _both(gpu, 0, 1, tasks, None, flags)
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
    case = Both(R, momentum)
    case.set_gradients(kinds)
    gpu = _clipping(R, momentum, wd)
    try:
        case.upload(gpu)
        before = _snapshot(gpu, R, momentum)[0]
        _both(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, MAX_NORM, True, keep=flags == 0)
        case.check(gpu)
        counts = [[0, 0, 0] for _ in range(R)]
        _count(counts, case)
        case.check_records(gpu, counts)
        if kinds[0] == "join":
            assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R  # no norm, no record touched
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
    gpu, twin = _clipping(R, momentum, wd), _clipping(R, momentum, wd)
    plan = [(["clipped", "skipped", "unclipped", "join"], [0, 1, 2, -1]),
            (["skipped", "join", "clipped", "clipped"], [4, -1, 5, 6]),
            (["unclipped", "clipped", "skipped", "skipped"], [7, 8, 9, 10])]
    try:
        case = Both(R, momentum)
        case.upload(gpu)
        case.upload(twin)
        steps = [[0, 0, 0] for _ in range(R)]
        for clock, (kinds, tasks) in enumerate(plan, 1):
            if clock == 2:  # a multiplier changes between two clocks: variable 4, 17 chunks, 15 of them uniform
                for g in (gpu, twin):
                    g.setModelVariableLearningRateMultiplier(4, 1, 3.0)
            case.set_gradients(kinds)
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            _both(gpu, 0, clock, tasks)
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


# ---- the degenerate rows: each is bit for bit the call it names -----------------------------
def _against(row, flags, make_gpu, make_twin, twin_call, kinds, tasks, records="same"):
    """records: "same" (the twin clips too: all 48 bytes equal) or "zero" (no norm ran, no record was touched)."""
    from crossbow_amd import BUF_GRADIENT
    R, momentum = 3, 0.9
    gpu, twin = make_gpu(), make_twin()
    try:
        for g in (gpu, twin):
            g.set_timing(True)
        case = Both(R, momentum)
        case.upload(gpu)
        case.upload(twin)
        for k in range(2):
            case.set_gradients(kinds)
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            tk = [t + 3 * k if t >= 0 else -1 for t in tasks]
            _both(gpu, 0, k + 1, tk, None, flags)
            twin.lockAny()
            getattr(twin, twin_call)(0, k + 1, 0, tk, None, flags)
            twin.unlockAny()
            gpu.wait()
            twin.wait()
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                assert np.array_equal(a[0][key].view(np.uint32), b[0][key].view(np.uint32)), f"{row}: {key} against {twin_call}"
            assert a[1:] == b[1:]
            if records == "same":
                assert [gpu.replica_clip_stats(i) for i in range(R)] == [twin.replica_clip_stats(i) for i in range(R)]
            else:
                assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
            assert len(gpu.timing_history()) == k + 1  # one timing entry per call
    finally:
        gpu.free()
        twin.free()


def _on_then_off(gpu):
    gpu.set_gradient_clip(1.0, True)  # the scratch exists, its records all zeros
    gpu.set_gradient_clip(0.0, False)
    return gpu


FINITE, STEPS = ["unclipped", "clipped", "clipped"], [0, 1, 2]
ONES = (1.0,) * len(V)


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("row", ["multipliers_all_1", "switch_off", "clipping_off", "both_off", "nobody_steps",
                                 "nobody_steps_multipliers_all_1"])
def test_each_degenerate_row_is_the_call_it_names(row, flags):
    wd = 1e-4
    mixed = ["unclipped", "clipped", "skipped"]
    if row == "multipliers_all_1":  # clipping on, no irregular multiplier: what _clipped launches
        _against(row, flags, lambda: _clipping(3, 0.9, wd, mults=ONES), lambda: _clipping(3, 0.9, wd, mults=ONES),
                 "step_and_synchronise_clipped", mixed, STEPS)
    elif row == "switch_off":
        _against(row, flags, lambda: _clipping(3, 0.9, wd, switch=False), lambda: _clipping(3, 0.9, wd, switch=False),
                 "step_and_synchronise_clipped", mixed, STEPS)
    elif row == "clipping_off":  # what _variables launches; the gradients stay finite, nothing is skipped
        _against(row, flags, lambda: _on_then_off(_gpu(3, 0.9, wd)), lambda: _gpu(3, 0.9, wd),
                 "step_and_synchronise_variables", FINITE, STEPS, "zero")
    elif row == "both_off":  # the plain kernel
        _against(row, flags, lambda: _on_then_off(_gpu(3, 0.9, wd, switch=False)),
                 lambda: _gpu(3, 0.9, wd, switch=False), "step_and_synchronise", FINITE, STEPS, "zero")
    elif row == "nobody_steps":  # clipping on, nobody steps: the kernel _variables launches, no record touched
        _against(row, flags, lambda: _clipping(3, 0.9, wd), lambda: _gpu(3, 0.9, wd),
                 "step_and_synchronise_variables", ["join"] * 3, [-1] * 3, "zero")
    else:
        _against(row, flags, lambda: _clipping(3, 0.9, wd, mults=ONES), lambda: _gpu(3, 0.9, wd, switch=False),
                 "step_and_synchronise", ["join"] * 3, [-1] * 3, "zero")


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
    case = Both(R, momentum)
    case.set_gradients(kinds)
    gpu = _clipping(R, momentum, wd, policy=policy)
    try:
        case.upload(gpu)
        if how == "set_beforehand":
            gpu.set_replica_copy(1, True)
        rates = _rates(policy, R, tasks, momentum)
        if how == "raised_by_this_call":
            assert rates == pytest.approx([0.1, 0.05, 0.1])
            assert [gpu.replica_copy(i) for i in range(R)] == [0, 0, 0]
        case.st.copy[1] = 1
        g2, last2 = case.g[2].copy(), case.last[2].copy()
        _both(gpu, 0, 7, tasks, None, flags)
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
    gpu, same = _clipping(R, momentum, wd), _clipping(R, momentum, wd)
    hip = _hip()
    try:
        case = Both(R, momentum)
        case.set_gradients(kinds)
        fresh = [torch.from_numpy(g).cuda() for g in case.g]
        for g in (gpu, same):
            case.upload(g)
        stale = np.full(N, 3.0, np.float32)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, stale)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for i in range(R):
            assert hip.hipMemcpyAsync(gpu.replica_buffer(i, BUF_GRADIENT), fresh[i].data_ptr(), 4 * N, 3,
                                      streams[i % 2].cuda_stream) == 0  # device to device
        _both(gpu, 0, 1, tasks, [streams[i % 2].cuda_stream for i in range(R)], flags)
        _both(same, 0, 1, tasks, None, flags)
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
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_a_pad_of_1e30_stays_untouched_and_unread(shape):
    # Were the pad of g read by the norm, each float would move S by 1e60: the records hold the exact S of
    # [0, n).  [0, n) of every buffer is the oracle's: no variable's multiplier and no pad float leaks into
    # it from the last partial chunk.
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    kinds, tasks = ["clipped", "unclipped", "skipped"], [3, 4, 5]
    rates = _rates(_exp, R, tasks, momentum)
    gpu = _clipping(R, momentum, wd)
    hip = _hip()
    try:
        gpu.set_task_barrier_kernel_config(*shape)
        case = Both(R, momentum)
        case.set_gradients(kinds)
        case.upload(gpu)
        pad = np.full(PADDED - N, 1e30, np.float32)
        assert pad.size == 3_053
        for i in range(R):
            assert hip.hipMemcpy(gpu.replica_buffer(i, BUF_GRADIENT) + 4 * N, pad.ctypes.data, pad.nbytes, 1) == 0
        _both(gpu, 0, 1, tasks)
        gpu.wait()
        case.step(tasks, rates, wd, MAX_NORM, True)
        case.check(gpu)  # [0, n) is the oracle's
        case.check_records(gpu, [[1, 1, 0], [1, 0, 0], [1, 1, 1]])  # S is that of [0, n), exactly
        # the skipped replica's pad keeps every bit (a stepping one's steps as the pseudo-variable of
        # multiplier 1, as in cbx_step_and_synchronise_variables)
        got = np.empty_like(pad)
        assert hip.hipMemcpy(got.ctypes.data, gpu.replica_buffer(2, BUF_GRADIENT) + 4 * N, got.nbytes, 2) == 0
        assert np.array_equal(got.view(np.uint32), pad.view(np.uint32)), "the pad of the skipped replica's g"
    finally:
        gpu.free()  # the pad no longer holds zeros: the context ends here


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in REFUSALS if k not in ("clipping", "variable_rates")])
def test_refusals_change_nothing(name):
    # the plain call's table without the two rows this call honours, with both features on
    from crossbow_amd import CbxError, _lib
    from tests.test_gpu_step_and_synchronise_variables import Case as VariablesCase
    code, kw, after, call = REFUSALS[name]
    n, R, momentum, wd = 4_099, 3, 0.9, 5e-4
    variables, mults = (n // 2, n - n // 2), (1.0, 2.0)
    update_type = kw.get("update_type", 7)
    gpu = _gpu(R, momentum, wd, variables=variables, mults=mults, sync=kw.get("sync", 0), update_type=update_type,
               method=kw.get("method", 0), elastic=kw.get("elastic", False), wpc=3)
    try:
        gpu.set_gradient_clip(1.0, True)
        if after:
            after(gpu)
        case = VariablesCase(R, momentum, variables, mults)
        case.upload(gpu)
        if update_type in (3, 7) and not kw.get("method") and not kw.get("elastic"):
            gpu.replica_optimise(1, 0)  # a record that is not all zeros: one clipped step behind replica 1
            gpu.wait()
            assert gpu.replica_clip_stats(1)["steps"] == 1
        gpu.set_replica_copy(0, True)  # a flag the refused call must leave raised
        before = _snapshot(gpu, R, momentum)
        records = [gpu.replica_clip_stats(i) for i in range(R)]
        hold = kw.get("hold")
        if hold is not None:
            gpu.replica_lock(hold)
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise_clipped_variables(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_clipped_variables(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_step_and_synchronise_clipped_variables" in _lib.last_error(), _lib.last_error()
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


def test_the_other_three_calls_still_refuse_what_they_refused():
    from crossbow_amd import CbxError, _lib
    gpu = _clipping(3, 0.9, 1e-4)  # both on
    try:
        gpu.lockAny()
        for call in (gpu.step_and_synchronise, gpu.step_and_synchronise_variables, gpu.step_and_synchronise_clipped):
            with pytest.raises(CbxError) as e:
                call(0, 1, 0, [3, 4, 5], None, 0)
            assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
            assert "cbx_step_and_synchronise_clipped_variables" in _lib.last_error()  # the reason names the call to take
        gpu.unlockAny()
        gpu.set_gradient_clip(0.0, False)  # clipping off, variable rates on
        gpu.lockAny()
        for call in (gpu.step_and_synchronise, gpu.step_and_synchronise_clipped):
            with pytest.raises(CbxError) as e:
                call(0, 1, 0, [3, 4, 5], None, 0)
            assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
        gpu.unlockAny()
        gpu.set_gradient_clip(1.0, False)  # clipping on, variable rates off
        gpu.set_variable_learning_rates(False)
        gpu.lockAny()
        for call in (gpu.step_and_synchronise, gpu.step_and_synchronise_variables):
            with pytest.raises(CbxError) as e:
                call(0, 1, 0, [3, 4, 5], None, 0)
            assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
        gpu.unlockAny()
        assert [gpu.replica_clip_stats(i) for i in range(3)] == [ZERO] * 3
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_each_call_adds_one_timing_entry(flags):
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 2, 0.9, 1e-4
    case = Both(R, momentum)
    case.set_gradients(["clipped", "skipped"])
    gpu = _clipping(R, momentum, wd)
    try:
        gpu.set_timing(True)
        case.upload(gpu)
        assert len(gpu.timing_history()) == 0
        for k in range(3):
            for i in range(R):
                gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            _both(gpu, 0, k + 1, [2 * k, 2 * k + 1], None, flags)
            gpu.wait()
            history = gpu.timing_history()
            assert len(history) == k + 1, history  # the norm launches add none
            assert history[-1] > 0.0
    finally:
        gpu.free()
