"""GPU parity of the replica step with per-variable learning rates.

``cbx_set_variable_learning_rates`` makes ``cbx_replica_optimise`` step every
variable with ``rate x multiplier`` (crossbowModelGetLearningRateForVariable,
clib-multigpu/model.c:159-177); ``cbx_replica_optimise_variables`` is the
per-operator form (crossbowStreamSynchronousEamsgdModelUpdate,
stream.c:422-479).  The reference is the oracle's replica step called once per
variable on slices (tests/test_optimise_plan.py pins it to its OpenBLAS
replay); every comparison is bit for bit on w, s, g and last.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact
from tests.test_optimise_plan import LR, M, V, per_variable_step

pytestmark = pytest.mark.gpu

N = sum(V)
R = 2
AUX_CONFIGS = [None, (64, 2, 2), (256, 1, 0), (512, 1, 8)]
KINDS = ("w", "g", "last", "s")


def _gpu(momentum, wd, mults=M, update_type=7, method=0, replicas=R, layout=None, capacity_slack=0):
    """One operator per variable of V (or ``layout``: (op, order, floats) in
    registration order), multipliers ``mults`` in that order."""
    from crossbow_amd import TheGPU
    layout = layout or [(v, 1, V[v]) for v in range(len(V))]
    g = TheGPU()
    g.init([0])
    g.setModel(1 + max(op for op, _, _ in layout), 4 * sum(c for _, _, c in layout) + capacity_slack)
    for k, (op, order, count) in enumerate(layout):
        g.setModelVariable(op, order, [count], 4 * count + (capacity_slack if k == 0 else 0))
    if mults is not None:
        for (op, order, _), m in zip(layout, mults):
            g.setModelVariableLearningRateMultiplier(op, order, m)
    g.setUpdateModelType(update_type)
    g.setEamsgdAlpha(0.1)
    g.setMomentum(momentum, method)
    g.setWeightDecay(wd)
    g.setLearningRateDecayPolicyFixed(LR)
    g.setModelManager(replicas, 0)
    return g


def _host(seed, momentum, n=N, sentinel=False):
    """w, g, last, s on the host.  ``sentinel``: s holds a pattern of its own
    instead of zeros, so an unwritten float is told from a written one."""
    w = O.fill_normal(n, seed, 0.05)
    g = O.fill_normal(n, seed + 1, 0.01)
    last = O.fill_normal(n, seed + 2, 0.001) if momentum > 0 else None
    s = O.fill_normal(n, seed + 3, 7.0) if sentinel else np.zeros(n, np.float32)
    return [w, g, last, s]


def _put(gpu, i, bufs):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    for kind, a in zip((BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF), bufs):
        if a is not None:
            gpu.replica_write(i, kind, a)


def _check(gpu, i, bufs, what=""):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    for kind, name, a in zip((BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF), KINDS, bufs):
        if a is not None:
            assert_bitexact(gpu.replica_read(i, kind), a, f"{what}{name}[{i}]")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("on_torch_stream", [False, True])
@pytest.mark.parametrize("aux", AUX_CONFIGS)
def test_whole_model_step_bitexact(momentum, wd, on_torch_stream, aux):
    import torch
    gpu = _gpu(momentum, wd)
    try:
        gpu.set_variable_learning_rates(True)
        if aux:
            gpu.set_aux_kernel_config(*aux)
        stream = torch.cuda.Stream() if on_torch_stream else None
        for i in range(R):
            bufs = _host(300 + 10 * i, momentum, sentinel=True)
            _put(gpu, i, bufs)
            gpu.replica_optimise(i, task=i, stream=stream.cuda_stream if stream else None)
            gpu.wait()
            per_variable_step(LR, M, momentum, wd, *bufs)
            _check(gpu, i, bufs)
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_switch_off_ignores_the_multipliers(momentum):
    # present behaviour, kept: one rate for the whole model whatever is set
    gpu = _gpu(momentum, 5e-4)
    try:
        bufs = _host(340, momentum)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        O.sma_optimise(np.float32(-LR), momentum, 5e-4, *bufs)
        _check(gpu, 0, bufs)
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_irregular_with_every_multiplier_one_is_the_plain_step(momentum):
    gpu = _gpu(momentum, 5e-4, mults=None)
    try:
        gpu.set_variable_learning_rates(True)
        gpu.setModelVariableLearningRateMultiplier(3, 1, 2.0)  # conf.irregular = 1 from here on
        gpu.setModelVariableLearningRateMultiplier(3, 1, 1.0)
        bufs = _host(350, momentum)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        O.sma_optimise(np.float32(-LR), momentum, 5e-4, *bufs)
        _check(gpu, 0, bufs)
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("aux", [None, (64, 2, 2)])
def test_one_operator_touches_nothing_else(momentum, aux):
    gpu = _gpu(momentum, 5e-4)
    try:
        if aux:
            gpu.set_aux_kernel_config(*aux)
        bufs = _host(360, momentum, sentinel=True)
        _put(gpu, 0, bufs)
        gpu.replica_optimise_variables(0, task=0, op=3)
        gpu.wait()
        per_variable_step(LR, M, momentum, 5e-4, *bufs, only={3})
        _check(gpu, 0, bufs, "after op 3 alone: ")
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("aux", [None, (64, 2, 2)])
def test_operators_in_backward_order_on_two_streams_equal_the_whole_step(momentum, aux):
    import torch
    gpu = _gpu(momentum, 5e-4)
    try:
        if aux:
            gpu.set_aux_kernel_config(*aux)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = _host(370, momentum, sentinel=True)
        _put(gpu, 1, bufs)
        gpu.wait()
        for k, op in enumerate(reversed(range(len(V)))):
            gpu.replica_optimise_variables(1, task=5, op=op, stream=streams[k % 2].cuda_stream)
        gpu.wait()
        torch.cuda.synchronize()
        per_variable_step(LR, M, momentum, 5e-4, *bufs)
        _check(gpu, 1, bufs)
    finally:
        gpu.free()


def test_operator_with_two_separate_runs():
    # registration order: op 0 order 1, op 1 order 1, op 0 order 2; op 2 has no
    # variables at all
    layout = [(0, 1, 300), (1, 1, 7), (0, 2, 1030), (3, 1, 2)]
    mults = (3.0, 5.0, 0.25, 1.0)
    counts = [c for _, _, c in layout]
    n = sum(counts)
    gpu = _gpu(0.9, 5e-4, mults=mults, layout=layout)
    try:
        bufs = _host(380, 0.9, n=n, sentinel=True)
        _put(gpu, 0, bufs)
        gpu.replica_optimise_variables(0, task=0, op=2)  # no variables: nothing runs
        gpu.wait()
        _check(gpu, 0, bufs, "after the empty op: ")
        gpu.replica_optimise_variables(0, task=0, op=0)
        gpu.wait()
        per_variable_step(LR, mults, 0.9, 5e-4, *bufs, variables=counts, only={0, 2})
        _check(gpu, 0, bufs, "after op 0: ")
    finally:
        gpu.free()


def test_multiplier_changed_between_two_steps():
    gpu = _gpu(0.9, 5e-4)
    try:
        gpu.set_variable_learning_rates(True)
        bufs = _host(390, 0.9)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        per_variable_step(LR, M, 0.9, 5e-4, *bufs)
        m2 = list(M)
        m2[4] = 4.0
        gpu.setModelVariableLearningRateMultiplier(4, 1, 4.0)
        gpu.replica_optimise(0, task=1)
        gpu.wait()
        per_variable_step(LR, m2, 0.9, 5e-4, *bufs)
        _check(gpu, 0, bufs)
    finally:
        gpu.free()


def test_added_replica_steps_with_the_same_rates():
    gpu = _gpu(0.9, 5e-4)
    try:
        gpu.set_variable_learning_rates(True)
        gpu.addModel()  # replica R, created locked (modelmanager.c:433-435)
        gpu.unlockAny()
        assert gpu.num_replicas() == R + 1
        bufs = _host(400, 0.9, sentinel=True)
        _put(gpu, R, bufs)
        gpu.replica_optimise(R, task=0)
        gpu.replica_optimise_variables(R, task=1, op=5)
        gpu.wait()
        per_variable_step(LR, M, 0.9, 5e-4, *bufs)
        per_variable_step(LR, M, 0.9, 5e-4, *bufs, only={5})
        _check(gpu, R, bufs)
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_clock_loop_bitexact(momentum):
    # 2 clocks x 2 tasks of the per-variable step, then the barrier: the
    # snapshot the step leaves feeds the averaging.
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    from tests.helpers import compare_states, download, upload
    clocks, wpc, alpha, wd = 2, 2, 0.1, 1e-4
    gpu = _gpu(momentum, wd)
    try:
        gpu.set_variable_learning_rates(True)
        st = O.make_state(N, 1, R, alpha, momentum)
        upload(gpu, st)
        lasts = [np.zeros(N, np.float32) if momentum > 0 else None for _ in range(R)]
        task = 0
        for clock in range(1, clocks + 1):
            for i in range(R):
                for _ in range(wpc):
                    gr = O.fill_normal(N, 1000 + task, 0.01)
                    gpu.replica_write(i, BUF_GRADIENT, gr)
                    gpu.replica_optimise(i, task)
                    per_variable_step(LR, M, momentum, wd, st.w[i], gr, lasts[i], st.s[i])
                    task += 1
            gpu.lockAny()
            gpu.synchronise(0, clock, 0, False)
            gpu.unlockAny()
            O.sma_step(st)
        gpu.wait()
        compare_states(download(gpu, st), st)
        if momentum > 0:
            for i in range(R):
                assert_bitexact(gpu.replica_read(i, BUF_LAST), lasts[i], f"replica last[{i}]")
    finally:
        gpu.free()


def _refused(gpu, call, code, momentum=0.9):
    from crossbow_amd import CbxError
    bufs = _host(410, momentum, n=gpu.elements(), sentinel=True)
    _put(gpu, 0, bufs)
    with pytest.raises(CbxError) as e:
        call()
    assert e.value.code == code, e.value
    gpu.wait()
    _check(gpu, 0, bufs, "after the refusal: ")
    return str(e.value)


def test_capacity_above_the_elements_is_refused():
    from crossbow_amd import _lib
    gpu = _gpu(0.9, 5e-4, capacity_slack=16)  # variable (0, 1): 1 float in 20 bytes
    try:
        gpu.set_variable_learning_rates(True)
        msg = _refused(gpu, lambda: gpu.replica_optimise(0, 0), _lib.CBX_ERR_UNSUPPORTED)
        assert "op 0, order 1" in msg, msg
        msg = _refused(gpu, lambda: gpu.replica_optimise_variables(0, 0, 3), _lib.CBX_ERR_UNSUPPORTED)
        assert "op 0, order 1" in msg, msg
        gpu.set_variable_learning_rates(False)  # the one-rate step needs no variable ranges
        gpu.replica_optimise(0, 0)
        gpu.wait()
    finally:
        gpu.free()


@pytest.mark.parametrize("update_type", [1, 6])  # WORKER, POLYAK_RUPPERT
def test_per_operator_step_is_unsupported_under(update_type):
    from crossbow_amd import _lib
    gpu = _gpu(0.9, 5e-4, update_type=update_type)
    try:
        _refused(gpu, lambda: gpu.replica_optimise_variables(0, 0, 3), _lib.CBX_ERR_UNSUPPORTED)
    finally:
        gpu.free()


def test_nesterov_and_bad_arguments_are_refused():
    from crossbow_amd import CbxError, _lib
    gpu = _gpu(0.9, 5e-4, method=1)  # NESTEROV (utils.h:101)
    try:
        gpu.set_variable_learning_rates(True)
        _refused(gpu, lambda: gpu.replica_optimise(0, 0), _lib.CBX_ERR_UNSUPPORTED)
        _refused(gpu, lambda: gpu.replica_optimise_variables(0, 0, 3), _lib.CBX_ERR_UNSUPPORTED)
        _refused(gpu, lambda: gpu.replica_optimise_variables(0, 0, len(V)), _lib.CBX_ERR_INVALID)
        _refused(gpu, lambda: gpu.replica_optimise_variables(0, 0, -1), _lib.CBX_ERR_INVALID)
        with pytest.raises(CbxError) as e:
            gpu.set_variable_learning_rates(2)
        assert e.value.code == _lib.CBX_ERR_INVALID
    finally:
        gpu.free()
