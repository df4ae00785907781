"""GPU parity of ``cbx_step_and_synchronise``: the replicas' pending task steps
fused into the one-GPU SMA barrier (task_barrier_kernels.hip).

Expected values always come from the oracle: ``O.sma_optimise`` for every
stepping replica, then ``O.sma_step``.  A twin context that runs the two-call
sequence stands beside it only to read each replica's rate
(``replica_learning_rate``) and to compare host state (copy flags, clocks).
Every comparison is bit for bit, over every buffer: z, the base ``last``, and
``w``, ``last``, ``s`` and ``g`` of every replica.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact

pytestmark = pytest.mark.gpu

ALPHA = 0.1
DISCARD = 1  # CBX_STEP_DISCARD_TASK_OUTPUTS


def _exp(g):
    g.setLearningRateDecayPolicyExp(0.05, 0.97)


def _inv(g):
    g.setLearningRateDecayPolicyInv(0.05, 0.01, 0.75)


def _gpu(n, R, momentum, wd, policy=_exp, sync=0, update_type=7, method=0, before_manager=None):
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(1, 4 * n)
    g.setModelVariable(0, 1, [n], 4 * n)
    g.setUpdateModelType(update_type)
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, method)
    g.setWeightDecay(wd)
    policy(g)
    if before_manager:
        before_manager(g)
    g.setModelManager(R, sync)
    return g


class Case:
    """The device's buffers mirrored on the host: the oracle's state plus the
    replicas' gradients and momenta."""

    def __init__(self, n, R, momentum, seed=0):
        self.n, self.R, self.momentum = n, R, momentum
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

    def step(self, tasks, rates, wd, keep=True):
        """The oracle's two-call sequence.  Without `keep` the device leaves
        s and g of the stepping replicas alone: the mirror keeps them aside."""
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if tasks[i] >= 0 and not keep}
        for i in range(self.R):
            if tasks[i] >= 0:
                O.sma_optimise(np.float32(-rates[i]), self.momentum, wd, st.w[i], self.g[i], self.last[i], st.s[i])
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


def _rates(policy, R, tasks, momentum=0.0):
    """Each stepping replica's rate, read from a twin context's own configuration."""
    twin = _gpu(4, R, momentum, 0.0, policy)
    try:
        return [twin.replica_learning_rate(i, tasks[i]) if tasks[i] >= 0 else 0.0 for i in range(R)]
    finally:
        twin.free()


def _fused(gpu, first, clock, tasks, streams=None, flags=0):
    gpu.lockAny()
    gpu.step_and_synchronise(first, clock, 0, tasks, streams, flags)
    gpu.unlockAny()


def _run_bitexact(n, R, momentum, wd, policy, flags, config=None):
    tasks = [3 + 2 * i for i in range(R)]  # a task number, hence a rate, per replica
    rates = _rates(policy, R, tasks, momentum)
    assert R == 1 or len(set(rates)) == R, rates
    case = Case(n, R, momentum)
    gpu = _gpu(n, R, momentum, wd, policy)
    try:
        if config:
            gpu.set_task_barrier_kernel_config(*config)
        case.upload(gpu)
        _fused(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        assert [gpu.replica_clock(i) for i in range(R)] == [1] * R
    finally:
        gpu.free()


# n: one element; one float past a pad quantum; a ragged size of several waves.
# R: the largest unrolled count (8) and the first that needs a second chunk (9).
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("n,R,momentum,wd,policy", [
    (1, 1, 0.0, 0.0, _exp),
    (4_097, 2, 0.9, 5e-4, _inv),
    (70_001, 8, 0.9, 0.0, _exp),
    (70_001, 9, 0.0, 5e-4, _inv),
    (4_097, 9, 0.9, 5e-4, _exp),
    (1, 8, 0.0, 0.0, _inv),
    (70_001, 2, 0.0, 5e-4, _exp),
])
def test_every_buffer_bitexact(n, R, momentum, wd, policy, flags):
    _run_bitexact(n, R, momentum, wd, policy, flags)


# one and two float4s per lane, 64 and 256 threads, with and without a cap
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("config", [(64, 1, 0), (64, 2, 2), (256, 1, 4), (256, 2, 0)])
def test_forced_launch_shapes_bitexact(config, flags):
    _run_bitexact(70_001, 3, 0.9, 5e-4, _exp, flags, config)


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_grid_stride_shape_bitexact(flags):
    # The default configuration on a launch too small to fill the chip 16 waves
    # per CU over (small_launch_shape): one float4 per lane, 8 blocks per CU.
    # 800,001 floats are 200,704 float4s = 3,136 waves on at most 2,048 blocks,
    # so some blocks take a second trip.
    _run_bitexact(800_001, 2, 0.9, 5e-4, _exp, flags)


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_default_shape_with_the_occupancy_cap_bitexact(flags):
    # Nothing forced: 2,100,001 floats are 525,312 float4s = 4,104 two-float4
    # waves, past the 16 waves per CU (4,096 on 256 CUs) from which the default
    # configuration reserves LDS to cap the occupancy.
    _run_bitexact(2_100_001, 2, 0.9, 5e-4, _exp, flags)


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("how", ["set_beforehand", "raised_by_this_call"])
def test_phase_d(how, flags):
    n, R, momentum, wd = 70_001, 3, 0.9, 5e-4
    if how == "set_beforehand":
        policy, tasks = _exp, [4, 6, 8]
    else:  # replica 1 crosses the boundary at the task that is passed: (task + 1) >= 3
        def policy(g):
            g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
        tasks = [0, 2, 1]
    case = Case(n, R, momentum)
    gpu = _gpu(n, R, momentum, wd, policy)
    twin = _gpu(n, R, momentum, wd, policy)  # the two-call sequence: host state and rates only
    try:
        case.upload(gpu)
        case.upload(twin)
        if how == "set_beforehand":
            gpu.set_replica_copy(1, True)
            twin.set_replica_copy(1, True)
            case.st.copy[1] = 1
        rates = _rates(policy, R, tasks, momentum)
        for i in range(R):
            twin.replica_optimise(i, tasks[i])
        if how == "raised_by_this_call":
            assert [twin.replica_copy(i) for i in range(R)] == [0, 1, 0]
            assert rates == pytest.approx([0.1, 0.05, 0.1])
            case.st.copy[1] = 1
        twin.lockAny()
        twin.synchronise(0, 7, 0, False)
        twin.unlockAny()
        _fused(gpu, 0, 7, tasks, None, flags)
        gpu.wait()
        twin.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        from crossbow_amd import BUF_DATA
        z = gpu.base_read(0, BUF_DATA)
        for i in range(R):
            assert_bitexact(gpu.replica_read(i, BUF_DATA), z, f"w[{i}] == the new z")
        assert [gpu.replica_copy(i) for i in range(R)] == [twin.replica_copy(i) for i in range(R)] == [0] * R
        assert [gpu.replica_clock(i) for i in range(R)] == [twin.replica_clock(i) for i in range(R)] == [7] * R
    finally:
        gpu.free()
        twin.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("first,tasks", [(0, [5, -1, 7]), (1, [-1, 5, 7]), (1, [-1, -1, 4]), (0, [-1, -1, -1])])
def test_mixed_participation(first, tasks, flags):
    n, R, momentum, wd = 70_001, 3, 0.9, 5e-4
    rates = _rates(_inv, R, tasks, momentum)
    case = Case(n, R, momentum)
    case.st.first = first
    gpu = _gpu(n, R, momentum, wd, _inv)
    try:
        case.upload(gpu)
        _fused(gpu, first, 2, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        gpu.free()


def _hip():
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    return hip


def _busy(torch, stream, ms=2.0):
    """Hold `stream` for about `ms` milliseconds before whatever is queued next."""
    with torch.cuda.stream(stream):
        try:
            torch.cuda._sleep(int(ms * 2.1e6))  # ~2.1 GHz shader clock
        except (AttributeError, RuntimeError):
            a = torch.randn(2048, 2048, device="cuda")
            for _ in range(8):
                a = a @ a * 1e-3


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_launch_is_ordered_behind_the_gradient_streams(flags):
    # Each replica's gradient arrives on a task stream of its own, behind ~2 ms
    # of other work, and the fused call is enqueued at once: it must wait for
    # the streams it was given.  Until then the buffers hold another gradient.
    # (With the library's deferred waits switched off, $CBX_FAULT_SKIP_TASK_WAIT,
    # this came out wrong in every element of a replica's w whenever the task
    # stream did not happen to share the sync stream's hardware queue.)
    import torch

    from crossbow_amd import BUF_GRADIENT
    n, R, momentum, wd = 1 << 18, 3, 0.9, 5e-4
    tasks = [2, 4, 6]
    rates = _rates(_exp, R, tasks, momentum)
    case = Case(n, R, momentum)
    gpu = _gpu(n, R, momentum, wd, _exp)
    hip = _hip()
    try:
        case.upload(gpu)
        stale = O.fill_normal(n, 5999, 0.01)
        fresh = [torch.from_numpy(case.g[i]).cuda() for i in range(R)]
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, stale)
        streams = [torch.cuda.Stream() for _ in range(R)]
        torch.cuda.synchronize()
        for i in range(R):
            _busy(torch, streams[i])
            assert hip.hipMemcpyAsync(gpu.replica_buffer(i, BUF_GRADIENT), fresh[i].data_ptr(), 4 * n, 3,
                                      streams[i].cuda_stream) == 0  # device to device
        _fused(gpu, 0, 1, tasks, [s.cuda_stream for s in streams], flags)
        gpu.wait()
        torch.cuda.synchronize()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        torch.cuda.synchronize()
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_clock_loop_bitexact(flags):
    # 3 clocks of 2 tasks per replica: the first through cbx_replica_optimise,
    # the last fused into the barrier.  Every stepping replica steps again
    # before its s or g is read, so the discard flag's promise holds here.
    from crossbow_amd import BUF_GRADIENT
    n, R, clocks, wpc, momentum, wd = 33_333, 3, 3, 2, 0.9, 1e-4
    twin = _gpu(4, R, momentum, 0.0, _exp)
    case = Case(n, R, momentum)
    gpu = _gpu(n, R, momentum, wd, _exp)
    try:
        case.upload(gpu)
        task = 0
        for clock in range(1, clocks + 1):
            last_tasks = [-1] * R
            for k in range(wpc):
                for i in range(R):
                    case.g[i] = O.fill_normal(n, 6000 + task, 0.01)
                    gpu.replica_write(i, BUF_GRADIENT, case.g[i])
                    if k < wpc - 1:
                        gpu.replica_optimise(i, task)
                        O.sma_optimise(np.float32(-twin.replica_learning_rate(i, task)), momentum, wd, case.st.w[i],
                                       case.g[i], case.last[i], case.st.s[i])
                    else:
                        last_tasks[i] = task
                    task += 1
            rates = [twin.replica_learning_rate(i, last_tasks[i]) for i in range(R)]
            _fused(gpu, 0, clock, last_tasks, None, flags)
            case.step(last_tasks, rates, wd, keep=flags == 0)
        gpu.wait()
        case.check(gpu, "after the loop:")
        assert [gpu.replica_clock(i) for i in range(R)] == [clocks] * R
    finally:
        gpu.free()
        twin.free()


def _snapshot(gpu, R, momentum):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    bufs = {"z": gpu.base_read(0, BUF_DATA)}
    if momentum > 0:
        bufs["base last"] = gpu.base_read(0, BUF_LAST)
    for i in range(R):
        bufs[f"w[{i}]"] = gpu.replica_read(i, BUF_DATA)
        bufs[f"s[{i}]"] = gpu.replica_read(i, BUF_DIFF)
        bufs[f"g[{i}]"] = gpu.replica_read(i, BUF_GRADIENT)
        if momentum > 0:
            bufs[f"last[{i}]"] = gpu.replica_read(i, BUF_LAST)
    return bufs, [gpu.replica_copy(i) for i in range(R)], [gpu.replica_clock(i) for i in range(R)]


def _two_variables(g, n):
    g.setModel(1, 4 * n)
    g.setModelVariable(0, 1, [n // 2], 4 * (n // 2))
    g.setModelVariable(0, 2, [n - n // 2], 4 * (n - n // 2))
    g.setModelVariableLearningRateMultiplier(0, 2, 2.0)


REFUSALS = {
    # name: (error code name, keyword arguments of the context, set-up after the manager, call arguments)
    "force_split": ("CBX_ERR_UNSUPPORTED", {}, lambda g: g.set_force_split(True), {}),
    "clipping": ("CBX_ERR_UNSUPPORTED", {}, lambda g: g.set_gradient_clip(1.0, False), {}),
    "variable_rates": ("CBX_ERR_UNSUPPORTED", {"two_variables": True}, lambda g: g.set_variable_learning_rates(True), {}),
    "nesterov": ("CBX_ERR_UNSUPPORTED", {"method": 1}, None, {}),
    "worker": ("CBX_ERR_UNSUPPORTED", {"update_type": 1}, None, {}),
    "default": ("CBX_ERR_UNSUPPORTED", {"update_type": 0}, None, {}),
    "polyak_ruppert": ("CBX_ERR_UNSUPPORTED", {"update_type": 6}, None, {}),
    "elastic_average": ("CBX_ERR_UNSUPPORTED", {"update_type": 3, "elastic": True}, None, {}),
    "below_first": ("CBX_ERR_INVALID", {}, None, {"first": 1, "tasks": [3, 4, 5]}),
    "unlocked": ("CBX_ERR_INVALID", {"sync": 1, "hold": 2}, None, {}),
    "task_minus_2": ("CBX_ERR_INVALID", {}, None, {"tasks": [3, -2, 5]}),
    "null_tasks": ("CBX_ERR_INVALID", {}, None, {"tasks": None}),
    "flag_bit_2": ("CBX_ERR_INVALID", {}, None, {"flags": 2}),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing(name):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, CbxError, TheGPU, _lib
    from tests import averaging_common as AV
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
        if after:
            after(gpu)
        case = Case(n, R, momentum)
        case.upload(gpu)
        gpu.set_replica_copy(0, True)  # a flag the refused call must leave raised
        case.st.copy[0] = 1
        before = _snapshot(gpu, R, momentum)
        hold = kw.get("hold")
        if hold is not None:  # SSP: a task thread holds the replica, the barrier goes on without it
            gpu.replica_lock(hold)
            case.st.locked[hold] = 0
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_step_and_synchronise" in _lib.last_error(), _lib.last_error()  # the message names its cause
        gpu.wait()
        after_call = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after_call[0][key], before[0][key], f"{key} after the refused call")
        assert after_call[1:] == before[1:], "copy flags and clocks after the refused call"
        # a plain barrier right after it is still the oracle's
        gpu.synchronise(0, 2, 0, False)
        gpu.unlockAny()
        if hold is not None:
            gpu.replica_unlock(hold)
        gpu.wait()
        st = case.st
        if update_type == 1:
            O.ssgd_sync(st, [np.zeros(n, np.float32)], wpc)
        elif update_type == 0:
            O.default_sync(st)
        elif update_type == 6 or kw.get("elastic"):
            AV.step(st, update_type == 6, 2)
        else:
            O.sma_step(st)
        assert_bitexact(gpu.base_read(0, BUF_DATA), st.z[0], "z after the plain barrier")
        if update_type != 0 and not kw.get("elastic"):
            assert_bitexact(gpu.base_read(0, BUF_LAST), st.last[0], "base last after the plain barrier")
        for i in range(R):
            assert_bitexact(gpu.replica_read(i, BUF_DATA), st.w[i], f"w[{i}] after the plain barrier")
            assert_bitexact(gpu.replica_read(i, BUF_GRADIENT), case.g[i], f"g[{i}] after the plain barrier")
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_each_call_adds_one_timing_entry(flags):
    from crossbow_amd import BUF_GRADIENT
    n, R, momentum, wd = 70_001, 2, 0.9, 5e-4
    case = Case(n, R, momentum)
    gpu = _gpu(n, R, momentum, wd, _exp)
    try:
        gpu.set_timing(True)
        case.upload(gpu)
        assert len(gpu.timing_history()) == 0
        for k in range(3):
            for i in range(R):
                gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            _fused(gpu, 0, k + 1, [2 * k, 2 * k + 1], None, flags)
            gpu.wait()
            history = gpu.timing_history()
            assert len(history) == k + 1, history
            assert history[-1] > 0.0
    finally:
        gpu.free()
