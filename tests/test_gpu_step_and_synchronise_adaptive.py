"""GPU parity of the task steps with layer-wise adaptive rates fused into the one-GPU SMA barrier
(``cbx_step_and_synchronise_adaptive``; task_barrier_adaptive_kernels.hip).  The reference is the one of
tests/test_gpu_adaptive_rate.py per stepping replica (``math.fsum`` of exact products, rule 2 in float64,
the oracle's replica step per variable with ``(-lr * m_v) * t_v``), then the oracle's SMA barrier.  The
data of w and g is in that file's exact regime, so no device value enters an expectation.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import oracle as O
from tests.edge_values import assert_edge_equal
from tests.helpers import upload
from tests.test_gpu_adaptive_rate import EPS, RAGGED, SHAPES, _check_records, _data, _mults, _trust
from tests.test_gpu_step_and_synchronise import _exp

pytestmark = pytest.mark.gpu

ALPHA, ETA, DISCARD = 0.1, 0.05, 1
# momentum, weight decay, mode, multipliers, flags, (unroll, policy): every value of each with each path
CASES = [(0.0, 0.0, 0, False, 0, (1, 1)), (0.9, 1e-4, 1, True, DISCARD, (2, 0)),
         (0.9, 0.0, 1, False, DISCARD, (1, 0)), (0.0, 1e-4, 0, True, 0, (2, 1))]
# variables, tasks: 2 stepping (unrolled), 2 of 3 stepping (MIXED), 9 stepping (runtime-chunked, second column load)
PATHS = [(v, t) for v in ("ragged", "ragged0", "one") for t in ([3, 5], [3, -1, 7])] + [("one", list(range(3, 21, 2)))]


def _context(variables, enable, R, momentum, wd, mults, policy=_exp, update_type=7):
    from crossbow_amd import TheGPU
    gpu = TheGPU()
    gpu.init([0])
    gpu.setModel(len(variables), 4 * sum(variables))
    for v, count in enumerate(variables):
        gpu.setModelVariable(v, 1, [count], 4 * count)
        if mults[v] != 1.0:
            gpu.setModelVariableLearningRateMultiplier(v, 1, mults[v])
        if not enable[v]:
            gpu.set_model_variable_adaptive_rate(v, 1, False)
    gpu.setUpdateModelType(update_type)
    gpu.setEamsgdAlpha(ALPHA)
    gpu.setMomentum(momentum, 0)
    gpu.setWeightDecay(wd)
    policy(gpu)
    gpu.setModelManager(R, 0)
    return gpu


class State:
    """The device's buffers on the host: every replica its own data and, through its task, its own rate."""

    def __init__(self, variables, R, momentum, exact=True):
        data = [_data(variables, exact, momentum, seed=7 + 10 * i) for i in range(R)]
        self.variables, self.R, self.enable = variables, R, data[0][1]
        self.st = O.make_state(sum(variables), 1, R, ALPHA, momentum)
        for i, (bufs, _) in enumerate(data):
            self.st.w[i], self.st.s[i] = bufs[0], bufs[3]
        self.g, self.last = [b[1] for b, _ in data], [b[2] for b, _ in data]

    def upload(self, gpu):
        from crossbow_amd import BUF_GRADIENT, BUF_LAST
        upload(gpu, self.st)
        for i in range(self.R):
            gpu.replica_write(i, BUF_GRADIENT, self.g[i])
            if self.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, self.last[i])

    def step(self, tasks, rates, mults, wd, mode, keep):
        """The two-call sequence; returns the stepping replicas' expected records."""
        st, recs, kept = self.st, {}, {}
        for i in [i for i in range(self.R) if tasks[i] >= 0]:
            w, g, last, s = st.w[i], self.g[i], self.last[i], st.s[i]
            kept[i], lo, recs[i] = (s.copy(), g.copy()), 0, []
            for v, count in enumerate(self.variables):
                sl = slice(lo, lo + count)
                W, G = (math.fsum(float(x) * float(x) for x in a[sl][np.isfinite(a[sl])]) for a in (w, g))
                K = int(np.sum(~np.isfinite(w[sl])) + np.sum(~np.isfinite(g[sl])))
                t, flags = _trust(W, G, K, count, self.enable[v], ETA, wd, mode)
                recs[i].append((W, G, K, t, flags))
                if count:
                    rate = (np.float32(-rates[i]) * np.float32(mults[v])) * t
                    O.sma_optimise(rate, st.momentum, wd, w[sl], g[sl], last[sl] if last is not None else None, s[sl])
                lo += count
        O.sma_step(st)
        if not keep:  # the device leaves s and g of a stepping replica alone
            for i, (s, g) in kept.items():
                st.s[i][:], self.g[i][:] = s, g
        return recs

    def read(self, gpu):
        """Every buffer of want(), from the device."""
        from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "last": BUF_LAST}
        return {key: gpu.replica_read(int(key[-2]), kinds[key[:-3]]) if key[-1] == "]" else
                gpu.base_read(0, BUF_DATA if key == "z" else BUF_LAST) for key in self.want()}

    def want(self):
        out = {"z": self.st.z[0], "base last": self.st.last[0] if self.st.last is not None else None}
        for i in range(self.R):
            out.update({f"w[{i}]": self.st.w[i], f"s[{i}]": self.st.s[i], f"g[{i}]": self.g[i], f"last[{i}]": self.last[i]})
        return {key: a for key, a in out.items() if a is not None}


def _rates(make, tasks):
    twin = make()  # the rates, read from a twin context's own configuration
    try:
        return [twin.replica_learning_rate(i, t) if t >= 0 else 0.0 for i, t in enumerate(tasks)]
    finally:
        twin.free()


def _fused(gpu, tasks, flags=0, clock=1):
    gpu.lockAny()
    gpu.step_and_synchronise_adaptive(0, clock, 0, tasks, None, flags)
    gpu.unlockAny()
    gpu.wait()


@pytest.mark.parametrize("momentum, wd, mode, multipliers, flags, shape", CASES)
@pytest.mark.parametrize("variables, tasks", PATHS)
def test_every_buffer_and_record_in_the_exact_regime(variables, tasks, momentum, wd, mode, multipliers, flags, shape):
    variables, R = SHAPES[variables], len(tasks)
    state, mults = State(variables, R, momentum), _mults(variables, multipliers)
    make = lambda: _context(variables, state.enable, R, momentum, wd, mults)
    rates = _rates(make, tasks)
    stepping = [r for r, t in zip(rates, tasks) if t >= 0]
    assert len(set(stepping)) == len(stepping), rates  # a swapped matrix column shows
    gpu = make()
    try:
        gpu.set_variable_learning_rates(multipliers)
        gpu.set_task_barrier_kernel_config(64, shape[0], -1)
        gpu.set_kernel_config(policy=shape[1])
        gpu.set_adaptive_rate(ETA, EPS, mode)
        state.upload(gpu)
        _fused(gpu, tasks, flags)
        recs = state.step(tasks, rates, mults, wd, mode, keep=flags == 0)
        got, want = state.read(gpu), state.want()
        for name in want:
            assert_edge_equal(got[name], want[name], name)
        for i, t in enumerate(tasks):
            dev = gpu.replica_adaptive_stats(i, len(variables))
            if t >= 0:
                _check_records(dev, recs[i])
            else:
                assert not dev.view(np.uint8).any(), f"replica {i} only joins"
    finally:
        gpu.free()


def _both_doors(variables, tasks, momentum, wd, policy, adaptive, multipliers=True):
    """The fused call and the device's own sequence (with the rates off: the other fused call) from the same
    state in two contexts: for each, every buffer's and every record's bytes and the host state."""
    R, out = len(tasks), []
    state, mults = State(variables, R, momentum, exact=False), _mults(variables, multipliers)
    for fused in (True, False):
        gpu = _context(variables, state.enable, R, momentum, wd, mults, policy)
        try:
            gpu.set_variable_learning_rates(multipliers)
            if adaptive:
                gpu.set_adaptive_rate(0.002, EPS, 1)
            state.upload(gpu)
            if fused:
                _fused(gpu, tasks, clock=7)
            else:
                for i in [i for i in range(R) if tasks[i] >= 0 and adaptive]:
                    gpu.replica_optimise(i, tasks[i])
                gpu.lockAny()
                if adaptive:
                    gpu.synchronise(0, 7, 0, False)
                else:  # with the rates off: the fused call that the multipliers ask for
                    gpu.step_and_synchronise_variables(0, 7, 0, tasks)
                gpu.unlockAny()
                gpu.wait()
            bufs = {k: v.tobytes() for k, v in state.read(gpu).items()}
            recs = [gpu.replica_adaptive_stats(i, len(variables)).tobytes() for i in range(R)]
            out.append((bufs, recs, [(gpu.replica_copy(i), gpu.replica_clock(i)) for i in range(R)]))
        finally:
            gpu.free()
    return out


def test_the_fused_call_is_the_sequence_on_normal_data():
    fused, sequence = _both_doors(RAGGED, [3, -1, 7], 0.9, 1e-4, _exp, True)
    assert fused == sequence
    assert any(fused[1][0]) and not any(fused[1][1])  # records for the stepping replica, none for the joiner


def test_phase_d_raised_by_a_rate_query_of_this_call():
    def policy(g):  # replica 1 crosses the boundary at the task that is passed
        g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
    fused, sequence = _both_doors(RAGGED, [0, 2, 1], 0.9, 1e-4, policy, True)
    assert fused == sequence
    bufs = fused[0]
    assert bufs["w[0]"] == bufs["w[1]"] == bufs["w[2]"] == bufs["z"]
    assert fused[2] == [(0, 7)] * 3


def test_with_adaptive_rates_off_it_is_the_other_fused_calls():
    fused, other = _both_doors(RAGGED, [3, 5], 0.9, 1e-4, _exp, False)
    assert fused[0] == other[0] and not any(any(r) for r in fused[1])


REFUSALS = {
    "clipping": (7, lambda g: g.set_gradient_clip(1.0), "UNSUPPORTED", "cbx_set_gradient_clip"),
    "elastic": (3, lambda g: g.setElasticAverage(True), "UNSUPPORTED", "cbx_synchronise"),
    "worker": (1, lambda g: None, "UNSUPPORTED", "cbx_set_adaptive_rate"),
    "not locked": (7, lambda g: g.unlockAny(), "INVALID", "not locked"),
    "the other fused calls": (7, lambda g: None, "UNSUPPORTED", "cbx_step_and_synchronise_adaptive"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing_and_name_the_call_to_take(name):
    from crossbow_amd import _lib
    update_type, prepare, code, names = REFUSALS[name]
    state, mults = State(RAGGED, 2, 0.9), _mults(RAGGED, False)
    gpu = _context(RAGGED, state.enable, 2, 0.9, 1e-4, mults, update_type=update_type)
    try:
        gpu.set_adaptive_rate(ETA, EPS, 0)
        state.upload(gpu)
        gpu.lockAny()
        prepare(gpu)
        call = gpu.step_and_synchronise_variables if name == "the other fused calls" else gpu.step_and_synchronise_adaptive
        with pytest.raises(_lib.CbxError) as e:
            call(0, 1, 0, [3, 5])
        assert e.value.code == getattr(_lib, "CBX_ERR_" + code) and names in str(e.value), str(e.value)
        got, want = state.read(gpu), state.want()
        for key in want:
            assert_edge_equal(got[key], want[key], f"{name}: {key}")
        assert not any(gpu.replica_adaptive_stats(i, len(RAGGED)).view(np.uint8).any() for i in range(2))
        assert [(gpu.replica_copy(i), gpu.replica_clock(i)) for i in range(2)] == [(0, 0)] * 2
    finally:
        gpu.free()


def test_a_model_without_variable_ranges_is_refused():
    from crossbow_amd import TheGPU, _lib
    gpu = TheGPU()
    gpu.init([0])
    try:
        gpu.setModel(1, 4 * 771)  # registered as raw bytes
        gpu.setUpdateModelType(7)
        _exp(gpu)
        gpu.setModelManager(1, 0)
        gpu.set_adaptive_rate(ETA, EPS, 0)
        gpu.lockAny()
        with pytest.raises(_lib.CbxError) as e:
            gpu.step_and_synchronise_adaptive(0, 1, 0, [0])
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED and "no variables" in str(e.value)
    finally:
        gpu.free()
