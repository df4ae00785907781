"""GPU parity of ``cbx_step_and_synchronise_variables``: the replicas' pending
task steps with a learning rate per variable, fused into the one-GPU SMA
barrier (task_barrier_variables_kernels.hip).

The reference is always the oracle, never a device result:
``tests.test_optimise_plan.per_variable_step`` for every stepping replica, then
``O.sma_step``.  Every comparison is bit for bit, over z, the base ``last`` and
every replica's ``w``, ``s``, ``g`` and ``last``.

The model is the variable list ``V`` of tests/test_optimise_plan.py with its
multipliers ``M``: n = 21,523 floats padded to 24,576; a float4 over two
variables at float 1; boundaries inside float4s and inside chunks (1, 4, 39,
4,132, 8,228, 9,228); uniform chunks; a last partial chunk; 3,053 pad floats.
None of V's boundaries falls exactly on a chunk boundary, so
``test_two_variables`` adds a model split at float 512 beside the one split
mid-float4.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact
from tests.test_gpu_step_and_synchronise import ALPHA, DISCARD, REFUSALS, _snapshot
from tests.test_optimise_plan import M, V, per_variable_step

pytestmark = pytest.mark.gpu

N = sum(V)
PADDED = 24_576
SHAPES = [(64, 1, -1), (64, 2, 2), (256, 1, 4), (256, 2, 0)]  # (block, unroll, waves per CU); -1: the auto cap


def _exp(g):
    g.setLearningRateDecayPolicyExp(0.05, 0.97)


def _inv(g):
    g.setLearningRateDecayPolicyInv(0.05, 0.01, 0.75)


def _gpu(R, momentum, wd, policy=_exp, variables=V, mults=M, switch=True, sync=0, update_type=7, method=0,
         elastic=False, wpc=None):
    """One operator per variable, multipliers in that order, the switch on."""
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(len(variables), 4 * sum(variables))
    for v, count in enumerate(variables):
        g.setModelVariable(v, 1, [count], 4 * count)
    for v, m in enumerate(mults):
        g.setModelVariableLearningRateMultiplier(v, 1, m)
    if wpc:
        g.setModelWorkPerClock(wpc)
    g.setUpdateModelType(update_type)
    if elastic:
        g.setElasticAverage(True)
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, method)
    g.setWeightDecay(wd)
    policy(g)
    g.setModelManager(R, sync)
    g.set_variable_learning_rates(switch)
    return g


class Case:
    """The device's buffers mirrored on the host (tests/test_gpu_step_and_synchronise.py's,
    with the per-variable step)."""

    def __init__(self, R, momentum, variables=V, mults=M, seed=0):
        self.n = n = sum(variables)
        self.R, self.momentum, self.variables, self.mults = R, momentum, variables, mults
        self.st = O.make_state(n, 1, R, ALPHA, momentum)
        self.g = [O.fill_normal(n, 5000 + seed + i, 0.01) for i in range(R)]
        self.last = [O.fill_normal(n, 5100 + seed + i, 0.001) if momentum > 0 else None for i in range(R)]

    def upload(self, gpu):
        from crossbow_amd import BUF_GRADIENT, BUF_LAST
        from tests.helpers import upload
        upload(gpu, self.st)
        for i in range(self.R):
            gpu.replica_write(i, BUF_GRADIENT, self.g[i])
            if self.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, self.last[i])

    def task_step(self, i, rate, wd):
        st = self.st
        per_variable_step(rate, self.mults, self.momentum, wd, st.w[i], self.g[i], self.last[i], st.s[i],
                          variables=self.variables)

    def step(self, tasks, rates, wd, keep=True):
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if tasks[i] >= 0 and not keep}
        for i in range(self.R):
            if tasks[i] >= 0:
                self.task_step(i, rates[i], wd)
        O.sma_step(st)
        self.dev_s = [kept[i][0] if i in kept else st.s[i] for i in range(self.R)]
        self.dev_g = [kept[i][1] if i in kept else self.g[i] for i in range(self.R)]

    def check(self, gpu, what=""):
        from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
        st = self.st
        assert_bitexact(gpu.base_read(0, BUF_DATA), st.z[0], f"{what} z")
        if st.last is not None:
            assert_bitexact(gpu.base_read(0, BUF_LAST), st.last[0], f"{what} base last")
        for i in range(self.R):
            assert_bitexact(gpu.replica_read(i, BUF_DATA), st.w[i], f"{what} w[{i}]")
            assert_bitexact(gpu.replica_read(i, BUF_DIFF), self.dev_s[i], f"{what} s[{i}]")
            assert_bitexact(gpu.replica_read(i, BUF_GRADIENT), self.dev_g[i], f"{what} g[{i}]")
            if self.last[i] is not None:
                assert_bitexact(gpu.replica_read(i, BUF_LAST), self.last[i], f"{what} last[{i}]")


def _rates(gpu, tasks):
    """Each stepping replica's rate from the context's own configuration (a
    query may raise a copy flag: callers that mind use a twin)."""
    return [gpu.replica_learning_rate(i, t) if t >= 0 else 0.0 for i, t in enumerate(tasks)]


def _twin_rates(policy, R, tasks, momentum):
    twin = _gpu(R, momentum, 0.0, policy, variables=(4,), mults=(1.0,), switch=False)
    try:
        return _rates(twin, tasks)
    finally:
        twin.free()


def _fused(gpu, first, clock, tasks, flags=0, variables=True):
    gpu.lockAny()
    (gpu.step_and_synchronise_variables if variables else gpu.step_and_synchronise)(first, clock, 0, tasks, None, flags)
    gpu.unlockAny()


# ---- the matrix ----------------------------------------------------------------
# One context per (R, momentum, weight decay); the launch shapes and the flags
# run on it one after the other, each from freshly uploaded buffers.
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [1, 3, 8, 9])
def test_every_buffer_bitexact(R, momentum, wd):
    tasks = [3 + 2 * i for i in range(R)]
    rates = _twin_rates(_exp, R, tasks, momentum)
    assert R == 1 or len(set(rates)) == R, rates
    gpu = _gpu(R, momentum, wd)
    try:
        clock = 0
        for shape in SHAPES:
            for flags in (0, DISCARD):
                gpu.set_task_barrier_kernel_config(*shape)
                case = Case(R, momentum)
                case.upload(gpu)
                clock += 1
                _fused(gpu, 0, clock, tasks, flags)
                gpu.wait()
                case.step(tasks, rates, wd, keep=flags == 0)
                case.check(gpu, f"shape {shape} flags {flags}:")
                assert [gpu.replica_clock(i) for i in range(R)] == [clock] * R
    finally:
        gpu.free()


def test_the_multipliers_matter():
    # the oracle with one rate differs from the per-variable one where M is not 1: the test above can fail
    w, g = O.fill_normal(N, 1, 0.05), O.fill_normal(N, 2, 0.01)
    a, b = w.copy(), w.copy()
    per_variable_step(0.05, M, 0.0, 0.0, a, g.copy(), None, np.zeros(N, np.float32))
    O.sma_optimise(np.float32(-0.05), 0.0, 0.0, b, g.copy(), None, np.zeros(N, np.float32))
    assert not np.array_equal(a[:1], b[:1]) and not np.array_equal(a[9228:], b[9228:])
    assert_bitexact(a[1:4], b[1:4], "multiplier 1")


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("first,tasks", [(0, [5, -1, 7]), (1, [-1, 5, 7]), (1, [-1, -1, 4]), (0, [-1, -1, -1])])
def test_mixed_participation(first, tasks, flags):
    R, momentum, wd = 3, 0.9, 5e-4
    rates = _twin_rates(_inv, R, tasks, momentum)
    case = Case(R, momentum)
    case.st.first = first
    gpu = _gpu(R, momentum, wd, _inv)
    try:
        case.upload(gpu)
        _fused(gpu, first, 2, tasks, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("how", ["set_beforehand", "raised_by_this_call"])
def test_phase_d(how, flags):
    R, momentum, wd = 3, 0.9, 5e-4
    if how == "set_beforehand":
        policy, tasks = _exp, [4, 6, 8]
    else:  # replica 1 crosses the boundary at the task that is passed: (task + 1) >= 3
        def policy(g):
            g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
        tasks = [0, 2, 1]
    case = Case(R, momentum)
    gpu = _gpu(R, momentum, wd, policy)
    try:
        case.upload(gpu)
        if how == "set_beforehand":
            gpu.set_replica_copy(1, True)
        rates = _twin_rates(policy, R, tasks, momentum)
        if how == "raised_by_this_call":
            assert rates == pytest.approx([0.1, 0.05, 0.1])
            assert [gpu.replica_copy(i) for i in range(R)] == [0, 0, 0]
        case.st.copy[1] = 1
        _fused(gpu, 0, 7, tasks, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        from crossbow_amd import BUF_DATA
        z = gpu.base_read(0, BUF_DATA)
        for i in range(R):
            assert_bitexact(gpu.replica_read(i, BUF_DATA), z, f"w[{i}] == the new z")
        assert [gpu.replica_copy(i) for i in range(R)] == [0] * R
        assert [gpu.replica_clock(i) for i in range(R)] == [7] * R
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("split", [4_099 // 2, 512])  # mid-float4; exactly on a chunk boundary
def test_two_variables(split, flags):
    n, R, momentum, wd = 4_099, 3, 0.9, 5e-4
    variables, mults = (split, n - split), (1.0, 2.0)
    assert (4_099 // 2) % 4 != 0 and 512 % 256 == 0
    tasks = [3, 4, 5]
    rates = _twin_rates(_exp, R, tasks, momentum)
    case = Case(R, momentum, variables, mults)
    gpu = _gpu(R, momentum, wd, variables=variables, mults=mults)
    try:
        case.upload(gpu)
        _fused(gpu, 0, 1, tasks, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("how", ["all_ones_switch_on", "switch_off"])
def test_without_irregular_rates_it_is_the_plain_call(how, flags):
    # the existing kernel, the same bits: a twin context through cbx_step_and_synchronise, and the oracle
    R, momentum, wd = 3, 0.9, 5e-4
    mults = (1.0,) * len(V) if how == "all_ones_switch_on" else M
    switch = how == "all_ones_switch_on"
    tasks = [3, 4, 5]
    rates = _twin_rates(_exp, R, tasks, momentum)
    case = Case(R, momentum, V, (1.0,) * len(V))  # the switch off ignores the multipliers
    gpu = _gpu(R, momentum, wd, mults=mults, switch=switch)
    twin = _gpu(R, momentum, wd, mults=(1.0,) * len(V), switch=False)
    try:
        case.upload(gpu)
        case.upload(twin)
        _fused(gpu, 0, 1, tasks, flags)
        _fused(twin, 0, 1, tasks, flags, variables=False)
        gpu.wait()
        twin.wait()
        a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
        for key in a[0]:
            assert_bitexact(a[0][key], b[0][key], f"{key} against cbx_step_and_synchronise")
        assert a[1:] == b[1:]
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        gpu.free()
        twin.free()


def test_a_multiplier_changed_between_two_clocks():
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 5e-4
    case = Case(R, momentum)
    gpu = _gpu(R, momentum, wd)
    try:
        case.upload(gpu)
        for clock, tasks in ((1, [0, 1, 2]), (2, [3, 4, 5])):
            rates = _twin_rates(_exp, R, tasks, momentum)
            if clock == 2:
                gpu.setModelVariableLearningRateMultiplier(4, 1, 3.0)  # variable 4: 17 chunks, 15 of them uniform
                case.mults = M[:4] + (3.0,) + M[5:]
                for i in range(R):
                    case.g[i] = O.fill_normal(N, 7000 + i, 0.01)
                    gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            _fused(gpu, 0, clock, tasks)
            gpu.wait()
            case.step(tasks, rates, wd)
            case.check(gpu, f"clock {clock}:")
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_clock_loop_bitexact(flags):
    # 3 clocks of 2 tasks per replica: the first through cbx_replica_optimise
    # (variable rates on), the last fused into the barrier.
    from crossbow_amd import BUF_GRADIENT
    R, clocks, wpc, momentum, wd = 3, 3, 2, 0.9, 1e-4
    twin = _gpu(R, momentum, 0.0, variables=(4,), mults=(1.0,), switch=False)
    case = Case(R, momentum)
    gpu = _gpu(R, momentum, wd)
    try:
        case.upload(gpu)
        task = 0
        for clock in range(1, clocks + 1):
            last_tasks = [-1] * R
            for k in range(wpc):
                for i in range(R):
                    case.g[i] = O.fill_normal(N, 6000 + task, 0.01)
                    gpu.replica_write(i, BUF_GRADIENT, case.g[i])
                    if k < wpc - 1:
                        gpu.replica_optimise(i, task)
                        case.task_step(i, twin.replica_learning_rate(i, task), wd)
                    else:
                        last_tasks[i] = task
                    task += 1
            rates = _rates(twin, last_tasks)
            _fused(gpu, 0, clock, last_tasks, flags)
            case.step(last_tasks, rates, wd, keep=flags == 0)
        gpu.wait()
        case.check(gpu, "after the loop:")
        assert [gpu.replica_clock(i) for i in range(R)] == [clocks] * R
    finally:
        gpu.free()
        twin.free()


# ---- the pad ---------------------------------------------------------------------
def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    return hip


def _buffers(gpu, R, momentum):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    out = {"z": gpu.base_buffer(0, BUF_DATA)}
    if momentum > 0:
        out["base last"] = gpu.base_buffer(0, BUF_LAST)
    for i in range(R):
        for name, kind in (("w", BUF_DATA), ("s", BUF_DIFF), ("g", BUF_GRADIENT)) + ((("last", BUF_LAST),) if momentum > 0 else ()):
            out[f"{name}[{i}]"] = gpu.replica_buffer(i, kind)
    return out


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
@pytest.mark.parametrize("fill", ["zero_pad", "pad_of_1e30"])
def test_the_pad(fill, shape):
    # M's last multiplier is 0.1 and M holds a 0: were the pad floats stepped
    # with a variable's multiplier nothing would show on zeros, so the second
    # run fills the pad with 1e30 and holds [0, n) to the oracle.
    R, momentum, wd = 3, 0.9, 5e-4
    tasks = [3, 4, 5]
    rates = _twin_rates(_exp, R, tasks, momentum)
    case = Case(R, momentum)
    gpu = _gpu(R, momentum, wd)
    hip = _hip()
    try:
        gpu.set_task_barrier_kernel_config(*shape)
        case.upload(gpu)
        bufs = _buffers(gpu, R, momentum)
        pad = np.zeros(PADDED - N, np.float32)
        assert pad.size == 3_053
        if fill == "pad_of_1e30":
            pad[:] = 1e30
            for name, p in bufs.items():
                assert hip.hipMemcpy(p + 4 * N, pad.ctypes.data, pad.nbytes, 1) == 0, name
        else:
            for name, p in bufs.items():  # the arena's pad starts as zeros
                got = np.empty_like(pad)
                assert hip.hipMemcpy(got.ctypes.data, p + 4 * N, got.nbytes, 2) == 0
                assert not got.view(np.uint32).any(), f"the pad of {name} before the call"
        _fused(gpu, 0, 1, tasks)
        gpu.wait()
        case.step(tasks, rates, wd)
        case.check(gpu)  # [0, n): a last partial chunk still takes its own variables' multipliers
        if fill == "zero_pad":
            for name, p in bufs.items():
                got = np.empty_like(pad)
                assert hip.hipMemcpy(got.ctypes.data, p + 4 * N, got.nbytes, 2) == 0
                assert not got.view(np.uint32).any(), f"the pad of {name} is not all zero bits after the call"
    finally:
        gpu.free()


# ---- refusals ----------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in REFUSALS if k != "variable_rates"])
def test_refusals_change_nothing(name):
    from crossbow_amd import CbxError, _lib
    code, kw, after, call = REFUSALS[name]
    n, R, momentum, wd = 4_099, 3, 0.9, 5e-4
    variables, mults = (n // 2, n - n // 2), (1.0, 2.0)
    gpu = _gpu(R, momentum, wd, variables=variables, mults=mults, sync=kw.get("sync", 0),
               update_type=kw.get("update_type", 7), method=kw.get("method", 0), elastic=kw.get("elastic", False), wpc=3)
    try:
        if after:
            after(gpu)
        case = Case(R, momentum, variables, mults)
        case.upload(gpu)
        gpu.set_replica_copy(0, True)  # a flag the refused call must leave raised
        before = _snapshot(gpu, R, momentum)
        hold = kw.get("hold")
        if hold is not None:
            gpu.replica_lock(hold)
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise_variables(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_variables(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_step_and_synchronise_variables" in _lib.last_error(), _lib.last_error()
        gpu.wait()
        after_call = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after_call[0][key], before[0][key], f"{key} after the refused call")
        assert after_call[1:] == before[1:], "copy flags and clocks after the refused call"
        gpu.unlockAny()
        if hold is not None:
            gpu.replica_unlock(hold)
    finally:
        gpu.free()


def test_the_plain_call_still_refuses_variable_rates():
    from crossbow_amd import CbxError, _lib
    gpu = _gpu(3, 0.9, 5e-4)
    try:
        gpu.lockAny()
        with pytest.raises(CbxError) as e:
            gpu.step_and_synchronise(0, 1, 0, [3, 4, 5], None, 0)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
        gpu.unlockAny()
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_each_call_adds_one_timing_entry(flags):
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 2, 0.9, 5e-4
    case = Case(R, momentum)
    gpu = _gpu(R, momentum, wd)
    try:
        gpu.set_timing(True)
        case.upload(gpu)
        assert len(gpu.timing_history()) == 0
        for k in range(3):
            for i in range(R):
                gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            _fused(gpu, 0, k + 1, [2 * k, 2 * k + 1], flags)
            gpu.wait()
            history = gpu.timing_history()
            assert len(history) == k + 1, history
            assert history[-1] > 0.0
    finally:
        gpu.free()
