"""GPU parity of ``cbx_step_and_synchronise_ssgd``: the replicas' pending task
steps fused into the one-GPU synchronous-SGD barrier (task_ssgd_kernels.hip),
under update model WORKER.

Expected values always come from the oracle: ``O.ssgd_worker`` for every
stepping replica in ascending id, then ``O.ssgd_sync``.  A twin context stands
beside it only to read each replica's rate (``replica_learning_rate``) and to
compare host state (copy flags, clocks); no device result enters an
expectation.  Every comparison is bit for bit, over every buffer: z, the base
``last``, the base gradient (all +0 afterwards), and ``w``, ``g``, ``s`` and
``last`` of every replica, the last two untouched.  The mirror, the policies
and the stream helpers are tests/test_gpu_step_and_synchronise.py's.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact
from tests.test_gpu_step_and_synchronise import ALPHA, DISCARD, Case, _busy, _exp, _gpu, _hip, _inv, _rates, _snapshot

pytestmark = pytest.mark.gpu

WORKER = 1  # CBX_UPDATE_WORKER


def _sgpu(n, R, momentum, wd, policy=_exp, sync=0, wpc=None):
    wpc = R if wpc is None else wpc
    return _gpu(n, R, momentum, wd, policy, sync=sync, update_type=WORKER,
                before_manager=lambda g: g.setModelWorkPerClock(wpc))


class SsgdCase(Case):
    """tests/test_gpu_step_and_synchronise.py's mirror with this barrier: the
    state's momentum is the base model's, `acc` the device's base gradient."""

    def __init__(self, n, R, momentum, wpc=None, seed=0):
        super().__init__(n, R, momentum, seed)
        self.wpc = R if wpc is None else wpc
        self.acc = np.zeros(n, np.float32)

    def worker(self, i, rate, wd):
        """One plain task step of replica i (cbx_replica_optimise)."""
        O.ssgd_worker(np.float32(-rate), wd, self.st.w[i], self.g[i], self.acc)

    def step(self, tasks, rates, wd, keep=True):
        st = self.st
        kept = {i: self.g[i].copy() for i in range(self.R) if tasks[i] >= 0 and not keep}
        for i in range(self.R):  # ascending id: the accumulator depends on the order
            if tasks[i] >= 0:
                self.worker(i, rates[i], wd)
        O.ssgd_sync(st, [self.acc], self.wpc)
        self.dev_s = st.s  # no step writes s, no barrier reads it
        self.dev_g = [kept.get(i, self.g[i]) for i in range(self.R)]

    def check(self, gpu, what=""):
        from crossbow_amd import BUF_GRADIENT
        super().check(gpu, what)
        assert not self.acc.any() and not np.signbit(self.acc).any()
        assert_bitexact(gpu.base_read(0, BUF_GRADIENT), self.acc, f"{what} base gradient")


def _fused(gpu, first, clock, tasks, streams=None, flags=0):
    gpu.lockAny()
    gpu.step_and_synchronise_ssgd(first, clock, 0, tasks, streams, flags)
    gpu.unlockAny()


def _run_bitexact(n, R, momentum, wd, policy, flags, config=None, load_policy=None, wpc=None, prefill=False):
    tasks = [3 + 2 * i for i in range(R)]  # a task number, hence a rate, per replica
    rates = _rates(policy, R, tasks, momentum)
    assert R == 1 or len(set(rates)) == R, rates
    case = SsgdCase(n, R, momentum, wpc)
    gpu = _sgpu(n, R, momentum, wd, policy, wpc=wpc)
    try:
        if load_policy is not None:
            gpu.set_kernel_config(64, 0, load_policy, 2)  # the load/store policy is shared by every kernel
        if config:
            gpu.set_task_barrier_kernel_config(*config)
        case.upload(gpu)
        if prefill:
            # An earlier task of the same clock, stepped by the plain call: the
            # base gradient is not zero when the fused call finds it.
            from crossbow_amd import BUF_GRADIENT
            gpu.replica_optimise(0, 1)
            case.worker(0, _rates(policy, R, [1] + [-1] * (R - 1), momentum)[0], wd)
            gpu.wait()
            assert case.acc.any()
            assert_bitexact(gpu.base_read(0, BUF_GRADIENT), case.acc, "base gradient before the fused call")
        _fused(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        assert [gpu.replica_clock(i) for i in range(R)] == [1] * R
    finally:
        gpu.free()


# n: one element; one float past a pad quantum; a ragged size of several waves.
# R: the largest unrolled count (8) and the first that needs a second chunk (9).
# Base momentum 0 / 0.9 and weight decay 0 / 5e-4 in every pairing.
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("n,R,momentum,wd,policy", [
    (1, 1, 0.0, 0.0, _exp),
    (4_097, 2, 0.9, 5e-4, _inv),
    (70_001, 8, 0.9, 0.0, _exp),
    (70_001, 9, 0.0, 5e-4, _inv),
    (4_097, 9, 0.9, 5e-4, _exp),
    (1, 8, 0.0, 0.0, _inv),
])
def test_every_buffer_bitexact(n, R, momentum, wd, policy, flags):
    _run_bitexact(n, R, momentum, wd, policy, flags)


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_work_per_clock_that_is_not_the_replica_count(flags):
    _run_bitexact(70_001, 8, 0.9, 5e-4, _exp, flags, wpc=3)


# The case that catches an accumulator started from 0.
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("n,R,momentum,wd", [(70_001, 3, 0.9, 5e-4), (4_097, 9, 0.0, 0.0)])
def test_base_gradient_that_is_not_zero_on_entry(n, R, momentum, wd, flags):
    _run_bitexact(n, R, momentum, wd, _exp, flags, prefill=True)


# one and two float4s per lane, 64 and 256 threads, with and without a cap, both load policies
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("load_policy", [0, 1])
@pytest.mark.parametrize("config", [(64, 1, 0), (64, 2, 2), (256, 1, 4), (256, 2, 0)])
def test_forced_launch_shapes_bitexact(config, load_policy, flags):
    _run_bitexact(70_001, 3, 0.9, 5e-4, _exp, flags, config, load_policy)


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_grid_stride_shape_bitexact(flags):
    # The default configuration on a launch too small to fill the chip 16 waves
    # per CU over (small_launch_shape): one float4 per lane, 8 blocks per CU.
    # 800,001 floats are 200,704 float4s = 3,136 waves on at most 2,048 blocks,
    # so some blocks take a second trip.
    _run_bitexact(800_001, 2, 0.9, 5e-4, _exp, flags)


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("first,tasks,hold", [
    (0, [5, -1, 7], None), (1, [-1, 5, 7], None), (1, [-1, -1, 4], None), (0, [-1, -1, -1], None),
    (0, [5, -1, 7], 1),  # SSP: a task thread holds replica 1, the barrier goes on without it
])
def test_mixed_participation(first, tasks, hold, flags):
    n, R, momentum, wd = 70_001, 3, 0.9, 5e-4
    rates = _rates(_inv, R, tasks, momentum)
    case = SsgdCase(n, R, momentum)
    case.st.first = first
    gpu = _sgpu(n, R, momentum, wd, _inv, sync=0 if hold is None else 1)
    try:
        case.upload(gpu)
        if hold is not None:
            gpu.replica_lock(hold)
            case.st.locked[hold] = 0
        _fused(gpu, first, 2, tasks, None, flags)
        if hold is not None:
            gpu.replica_unlock(hold)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
    finally:
        gpu.free()


def test_nobody_stepping_is_synchronise_under_worker():
    # the same inputs, a base gradient left by a plain task step, through
    # cbx_synchronise on a second context: both against the oracle
    n, R, momentum, wd = 70_001, 3, 0.9, 5e-4
    rate = _rates(_exp, R, [4, -1, -1], momentum)[0]
    for fused in (True, False):
        case = SsgdCase(n, R, momentum)
        gpu = _sgpu(n, R, momentum, wd)
        try:
            case.upload(gpu)
            gpu.replica_optimise(0, 4)
            case.worker(0, rate, wd)
            if fused:
                _fused(gpu, 0, 2, [-1] * R)
            else:
                gpu.lockAny()
                gpu.synchronise(0, 2, 0, False)
                gpu.unlockAny()
            gpu.wait()
            case.step([-1] * R, [0.0] * R, wd)
            case.check(gpu, "fused:" if fused else "cbx_synchronise:")
        finally:
            gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_launch_is_ordered_behind_the_gradient_streams(flags):
    # Each replica's gradient arrives on a task stream of its own, behind ~2 ms
    # of other work, and the fused call is enqueued at once: it must wait for
    # the streams it was given.  Until then the buffers hold another gradient.
    import torch

    from crossbow_amd import BUF_GRADIENT
    n, R, momentum, wd = 1 << 18, 3, 0.9, 5e-4
    tasks = [2, 4, 6]
    rates = _rates(_exp, R, tasks, momentum)
    case = SsgdCase(n, R, momentum)
    gpu = _sgpu(n, R, momentum, wd)
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
def test_clock_loop_alternates_with_the_two_call_sequence(flags):
    # 5 clocks on one context, gradients rewritten each clock: the odd clocks
    # through the fused call, the even ones through cbx_replica_optimise in
    # ascending id and cbx_synchronise.  Every clock rewrites g of every
    # replica, so the discard flag's promise holds.
    from crossbow_amd import BUF_GRADIENT
    n, R, clocks, momentum, wd = 33_333, 3, 5, 0.9, 1e-4
    twin = _gpu(4, R, momentum, 0.0, _exp)
    case = SsgdCase(n, R, momentum)
    gpu = _sgpu(n, R, momentum, wd)
    try:
        case.upload(gpu)
        task = 0
        for clock in range(1, clocks + 1):
            tasks = []
            for i in range(R):
                case.g[i] = O.fill_normal(n, 6000 + task, 0.01)
                gpu.replica_write(i, BUF_GRADIENT, case.g[i])
                tasks.append(task)
                task += 1
            rates = [twin.replica_learning_rate(i, tasks[i]) for i in range(R)]
            fused = clock % 2 == 1
            if fused:
                _fused(gpu, 0, clock, tasks, None, flags)
            else:
                for i in range(R):
                    gpu.replica_optimise(i, tasks[i])
                gpu.lockAny()
                gpu.synchronise(0, clock, 0, False)
                gpu.unlockAny()
            case.step(tasks, rates, wd, keep=not fused or flags == 0)
            gpu.wait()
            case.check(gpu, f"clock {clock} ({'fused' if fused else 'two calls'}):")
        assert [gpu.replica_clock(i) for i in range(R)] == [clocks] * R
    finally:
        gpu.free()
        twin.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_a_multistep_boundary_leaves_the_copy_flag_raised(flags):
    # MULTISTEP: replica 1 crosses the boundary at the task that is passed, (task + 1) >= 3, and the
    # query raises its copy flag.  The S-SGD barrier looks at no flag: it stays raised, as after the
    # two calls on the twin.
    def policy(g):
        g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
    n, R, momentum, wd = 70_001, 3, 0.9, 5e-4
    tasks = [0, 2, 1]
    case = SsgdCase(n, R, momentum)
    gpu = _sgpu(n, R, momentum, wd, policy)
    twin = _sgpu(n, R, momentum, wd, policy)  # the two-call sequence: host state and rates only
    try:
        case.upload(gpu)
        case.upload(twin)
        rates = _rates(policy, R, tasks, momentum)
        assert rates == pytest.approx([0.1, 0.05, 0.1])
        for i in range(R):
            twin.replica_optimise(i, tasks[i])
        assert [twin.replica_copy(i) for i in range(R)] == [0, 1, 0]
        twin.lockAny()
        twin.synchronise(0, 7, 0, False)
        twin.unlockAny()
        assert [gpu.replica_copy(i) for i in range(R)] == [0, 0, 0]
        _fused(gpu, 0, 7, tasks, None, flags)
        gpu.wait()
        twin.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        assert [gpu.replica_copy(i) for i in range(R)] == [twin.replica_copy(i) for i in range(R)] == [0, 1, 0]
        assert [gpu.replica_clock(i) for i in range(R)] == [twin.replica_clock(i) for i in range(R)] == [7] * R
    finally:
        gpu.free()
        twin.free()


INSTEAD = "cbx_replica_optimise and cbx_synchronise"
REFUSALS = {
    # name: (error code name, keyword arguments of the context, set-up after the manager, call arguments,
    #        what the message names)
    "force_split": ("CBX_ERR_UNSUPPORTED", {}, lambda g: g.set_force_split(True), {}, INSTEAD),
    "clipping": ("CBX_ERR_UNSUPPORTED", {}, lambda g: g.set_gradient_clip(1.0, False), {}, INSTEAD),
    "nesterov": ("CBX_ERR_UNSUPPORTED", {"method": 1}, None, {}, "cbx_replica_optimise"),
    "nesterov_without_momentum": ("CBX_ERR_UNSUPPORTED", {"method": 1, "momentum": 0.0}, None, {},
                                  "cbx_replica_optimise"),
    "default": ("CBX_ERR_UNSUPPORTED", {"update_type": 0}, None, {}, INSTEAD),
    "polyak_ruppert": ("CBX_ERR_UNSUPPORTED", {"update_type": 6}, None, {}, INSTEAD),
    "sma": ("CBX_ERR_UNSUPPORTED", {"update_type": 7}, None, {}, "the SMA barrier takes cbx_step_and_synchronise"),
    "eamsgd": ("CBX_ERR_UNSUPPORTED", {"update_type": 3}, None, {}, "the SMA barrier takes cbx_step_and_synchronise"),
    "elastic_average": ("CBX_ERR_UNSUPPORTED", {"update_type": 3, "elastic": True}, None, {},
                        "elastic averaging takes cbx_step_and_synchronise_elastic"),
    "no_work_per_clock": ("CBX_ERR_STATE", {"wpc": 0}, None, {}, "setModelWorkPerClock"),
    "step_policy_of_size_0": ("CBX_ERR_STATE", {"policy": lambda g: g.setLearningRateDecayPolicyStep(0.1, 0.5, 0)},
                              None, {}, "size 0"),
    "below_first": ("CBX_ERR_INVALID", {}, None, {"first": 1, "tasks": [3, 4, 5]}, "below the first"),
    "unlocked": ("CBX_ERR_INVALID", {"sync": 1, "hold": 2}, None, {}, "not locked"),
    "task_minus_2": ("CBX_ERR_INVALID", {}, None, {"tasks": [3, -2, 5]}, "-2"),
    "null_tasks": ("CBX_ERR_INVALID", {}, None, {"tasks": None}, "null task list"),
    "flag_bit_2": ("CBX_ERR_INVALID", {}, None, {"flags": 2}, "flag bits"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing(name):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, CbxError, TheGPU, _lib
    from tests import averaging_common as AV
    code, kw, after, call, names = REFUSALS[name]
    n, R, wd = 4_099, 3, 5e-4
    momentum, wpc = kw.get("momentum", 0.9), kw.get("wpc", 3)
    update_type = kw.get("update_type", WORKER)
    elastic = kw.get("elastic", False)
    gpu = TheGPU()
    gpu.init([0])
    try:
        gpu.setModel(1, 4 * n)
        gpu.setModelVariable(0, 1, [n], 4 * n)
        if wpc:
            gpu.setModelWorkPerClock(wpc)
        gpu.setUpdateModelType(update_type)
        if elastic:
            gpu.setElasticAverage(True)
        gpu.setEamsgdAlpha(ALPHA)
        gpu.setMomentum(momentum, kw.get("method", 0))
        gpu.setWeightDecay(wd)
        kw.get("policy", _exp)(gpu)
        gpu.setModelManager(R, kw.get("sync", 0))
        if after:
            after(gpu)
        case = SsgdCase(n, R, momentum, wpc)
        case.upload(gpu)
        # a base gradient and a flag the refused call must leave as they are
        case.acc = O.fill_normal(n, 5555, 0.01)
        gpu.base_write(0, BUF_GRADIENT, case.acc)
        gpu.set_replica_copy(0, True)
        case.st.copy[0] = 1
        before = _snapshot(gpu, R, momentum)
        hold = kw.get("hold")
        if hold is not None:  # SSP: a task thread holds the replica, the barrier goes on without it
            gpu.replica_lock(hold)
            case.st.locked[hold] = 0
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise_ssgd(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_ssgd(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert names in _lib.last_error(), _lib.last_error()  # the cause, and the call to take instead
        gpu.wait()
        after_call = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after_call[0][key], before[0][key], f"{key} after the refused call")
        assert after_call[1:] == before[1:], "copy flags and clocks after the refused call"
        assert_bitexact(gpu.base_read(0, BUF_GRADIENT), case.acc, "base gradient after the refused call")
        if not wpc:
            return  # the plain barrier needs the work per clock too
        # a plain barrier right after it is still the oracle's
        gpu.synchronise(0, 2, 0, False)
        gpu.unlockAny()
        if hold is not None:
            gpu.replica_unlock(hold)
        gpu.wait()
        st = case.st
        if update_type == WORKER:
            O.ssgd_sync(st, [case.acc], wpc)
        elif update_type == 0:
            O.default_sync(st)
        elif update_type == 6 or elastic:
            AV.step(st, update_type == 6, 2)
        else:
            O.sma_step(st)
        assert_bitexact(gpu.base_read(0, BUF_DATA), st.z[0], "z after the plain barrier")
        if update_type != 0 and momentum > 0:
            assert_bitexact(gpu.base_read(0, BUF_LAST), st.last[0], "base last after the plain barrier")
        for i in range(R):
            assert_bitexact(gpu.replica_read(i, BUF_DATA), st.w[i], f"w[{i}] after the plain barrier")
            assert_bitexact(gpu.replica_read(i, BUF_GRADIENT), case.g[i], f"g[{i}] after the plain barrier")
    finally:
        gpu.free()


# More than 64 participants cannot be reached through a context: the model manager
# refuses more than 64 replicas on a device.  The seam's test holds that refusal
# (tests/test_gpu_seam_step_and_optimise_ssgd.py).


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_each_call_adds_one_timing_entry(flags):
    from crossbow_amd import BUF_GRADIENT
    n, R, momentum, wd = 70_001, 2, 0.9, 5e-4
    case = SsgdCase(n, R, momentum)
    gpu = _sgpu(n, R, momentum, wd)
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
