"""GPU parity of ``cbx_step_and_synchronise_ssgd_adaptive`` (task_ssgd_adaptive_kernels.hip): layer-wise adaptive
rates in the one-GPU synchronous-SGD barrier.  The reference: acc by ``O.ssgd_worker`` per stepping replica, Gs by
numpy fp32 adds in id order, the norms by ``math.fsum`` over exact products, t_v by tests/test_gpu_adaptive_rate.py's
``_trust``, the apply by ``O.ssgd_sync`` per variable on ``np.float32(t_v) * acc``.  In the exact regime (integers
|k| <= 2^10 times one power of two per buffer, wpc a power of two) no device value enters an expectation; on normal
data Z_v and G_v are held to the reordering bound 2 m 2^-53 sum and t_v and the step are restated from them.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests.edge_values import assert_edge_equal
from tests.test_gpu_adaptive_rate import EPS, LR, RAGGED, SHAPES, _check_records, _data, _mults, _trust
from tests.test_gpu_step_and_synchronise import _exp
from tests.test_gpu_step_and_synchronise_adaptive import CASES, ETA, State, _context, _rates

pytestmark = pytest.mark.gpu

WORKER = 1  # CBX_UPDATE_WORKER
# tasks, first, wpc: one stepping replica; three plus one that only joins, replica 0 below `first`; kChunk + 1
SETS = {"one": ([3], 0, 1), "joiner": ([-1, 3, 5, 7, -1], 1, 4), "chunked": (list(range(3, 21, 2)), 0, 8)}
PATHS = [(v, s) for v in ("ragged", "ragged0", "one") for s in ("one", "joiner", "chunked")]


def context(variables, enable, R, momentum, wd, mults, wpc, update_type=WORKER):
    return _context(variables, enable, R, momentum, wd, mults, lambda g: (_exp(g), g.setModelWorkPerClock(wpc)),
                    update_type)


class SsgdState(State):
    """State with the base model z from the same data builder (so the special variables are z's), the base
    gradient, and this barrier behind the steps."""

    def __init__(self, variables, R, momentum, wpc, first=0, exact=True):
        super().__init__(variables, R, momentum, exact)
        self.st.z[0] = _data(variables, exact, momentum, seed=1000)[0][0]
        self.st.first, self.wpc, self.acc = first, wpc, np.zeros(sum(variables), np.float32)

    def step(self, tasks, rates, wd, mode, keep, on=True, device=None, eta=ETA):
        """The issue's sequence in place; returns the expected records (none when the call is the plain one).
        ``device``: the device's records, whose sums stand in for Z_v and G_v once they are within the bound."""
        st, ids, recs, lo = self.st, [i for i, t in enumerate(tasks) if t >= 0], [], 0
        kept = {i: self.g[i].copy() for i in ids}
        Gs = np.zeros(st.n, np.float32)
        with np.errstate(all="ignore"):
            for i in ids:
                Gs = Gs + self.g[i]
                O.ssgd_worker(np.float32(-rates[i]), wd, st.w[i], self.g[i], self.acc)
            gbar = np.float32(1.0 / self.wpc) * Gs
            if not (on and ids):
                O.ssgd_sync(st, [self.acc], self.wpc)
            for v, count in enumerate(self.variables if on and ids else ()):
                sl = slice(lo, lo + count)
                sq = [[float(x) * float(x) for x in a[sl][np.isfinite(a[sl])]] for a in (st.z[0], gbar)]
                Z, G = math.fsum(sq[0]), math.fsum(sq[1])
                K = int(np.sum(~np.isfinite(st.z[0][sl])) + np.sum(~np.isfinite(gbar[sl])))
                if device is not None:
                    for got, want, terms in ((device["w_sq"][v], Z, sq[0]), (device["g_sq"][v], G, sq[1])):
                        assert abs(got - want) <= 2 * len(terms) * 2.0 ** -53 * want, (v, got, want)
                    Z, G = float(device["w_sq"][v]), float(device["g_sq"][v])
                t, flags = _trust(Z, G, K, count, self.enable[v], eta, wd, mode)
                recs.append((Z, G, K, t, flags))
                if count:
                    sub = dataclasses.replace(st, n=count, z=[st.z[0][sl]], s=[s[sl] for s in st.s],
                                              w=[w[sl] for w in st.w],
                                              last=None if st.last is None else [st.last[0][sl]])
                    O.ssgd_sync(sub, [np.float32(t) * self.acc[sl]], self.wpc)
                lo += count
        self.acc[:] = 0.0
        for i in ids if not keep else ():  # the device leaves g of a stepping replica alone
            self.g[i][:] = kept[i]
        return recs

    def read(self, gpu):
        from crossbow_amd import BUF_GRADIENT
        return dict(super().read(gpu), **{"base gradient": gpu.base_read(0, BUF_GRADIENT)})

    def everything(self):
        """want() and the base gradient."""
        return dict(self.want(), **{"base gradient": self.acc})


def _fused(gpu, tasks, flags=0, first=0, call="step_and_synchronise_ssgd_adaptive"):
    gpu.lockAny()
    getattr(gpu, call)(first, 1, 0, tasks, None, flags)
    gpu.unlockAny()
    gpu.wait()


def _compare(gpu, state, what=""):
    got, want = state.read(gpu), state.everything()
    for name in want:
        assert_edge_equal(got[name], want[name], what + name)


def _run_exact(variables, replicas, momentum, wd, mode, multipliers, flags, shape):
    """``shape``: (unroll, policy), or None for the default launch configuration."""
    tasks, first, wpc = SETS[replicas]
    state, mults = SsgdState(variables, len(tasks), momentum, wpc, first), _mults(variables, multipliers)
    make = lambda: context(variables, state.enable, len(tasks), momentum, wd, mults, wpc)  # noqa: E731
    rates = _rates(make, tasks)
    gpu = make()
    try:
        gpu.set_variable_learning_rates(multipliers)  # they play no part
        if shape:
            # Unroll 2 with a forced occupancy: in auto mode a launch this small is reshaped to unroll 1
            # (small_launch_shape), and the unroll-2 instantiations would not run.
            gpu.set_task_barrier_kernel_config(64, shape[0], 2 if shape[0] == 2 else -1)
            gpu.set_kernel_config(policy=shape[1])
        gpu.set_adaptive_rate(ETA, EPS, mode)
        state.upload(gpu)
        _fused(gpu, tasks, flags, first)
        recs = state.step(tasks, rates, wd, mode, keep=flags == 0)
        _compare(gpu, state)
        _check_records(gpu.base_adaptive_stats(0, len(variables)), recs)
        assert not any(gpu.replica_adaptive_stats(i, len(variables)).view(np.uint8).any() for i in range(len(tasks)))
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum, wd, mode, multipliers, flags, shape", CASES)
@pytest.mark.parametrize("variables, replicas", PATHS)
def test_every_buffer_and_record_in_the_exact_regime(variables, replicas, momentum, wd, mode, multipliers, flags, shape):
    _run_exact(SHAPES[variables], replicas, momentum, wd, mode, multipliers, flags, shape)


def test_grid_stride_trips_in_the_exact_regime():
    # The default configuration on a launch too small to fill the chip 16 waves per CU over (small_launch_shape): one
    # float4 per lane, 8 blocks per CU.  800,001 floats are 200,704 padded float4s = 3,136 waves on at most 2,048
    # blocks, so some blocks of the apply kernel take a second trip; the variable boundary lies inside a float4.
    _run_exact((300_001, 500_000), "joiner", 0.9, 1e-4, 1, False, 0, None)


def run_normal(momentum=0.9, wd=1e-4, mode=1, tasks=(3, 5, -1)):
    """One call on normal data, checked; returns every buffer's and the records' bytes."""
    state = SsgdState(RAGGED, len(tasks), momentum, 3, exact=False)
    make = lambda: context(RAGGED, state.enable, len(tasks), momentum, wd, _mults(RAGGED, False), 3)  # noqa: E731
    rates = _rates(make, tasks)
    gpu = make()
    try:
        gpu.set_adaptive_rate(0.002, EPS, mode)
        state.upload(gpu)
        _fused(gpu, list(tasks))
        recs = gpu.base_adaptive_stats(0, len(RAGGED))
        _check_records(recs, state.step(tasks, rates, wd, mode, True, device=recs, eta=0.002))
        _compare(gpu, state)
        return {k: v.tobytes() for k, v in state.read(gpu).items()}, recs.tobytes(), rates
    finally:
        gpu.free()


def test_normal_data_is_within_the_bound_and_two_calls_return_the_same_bytes():
    assert run_normal()[:2] == run_normal()[:2]


# adaptive call's context: (enable all?, rates on?, tasks); the other context runs the plain call with the rates off
@pytest.mark.parametrize("name, enabled, on, tasks", [("excluded", False, True, [3, 5]), ("off", True, False, [3, 5]),
                                                      ("nobody", True, True, [-1, -1])])
def test_degenerations_are_the_plain_call_bit_for_bit(name, enabled, on, tasks):
    out = []
    for call in ("step_and_synchronise_ssgd_adaptive", "step_and_synchronise_ssgd"):
        state = SsgdState(RAGGED, 2, 0.9, 2, exact=False)
        enable = state.enable if enabled else [False] * len(RAGGED)
        gpu = context(RAGGED, enable, 2, 0.9, 1e-4, _mults(RAGGED, False), 2)
        try:
            if on and call.endswith("adaptive"):
                gpu.set_adaptive_rate(ETA, EPS, 0)
            state.upload(gpu)
            _fused(gpu, tasks, call=call)
            out.append({k: v.tobytes() for k, v in state.read(gpu).items()})
            recs = gpu.base_adaptive_stats(0, len(RAGGED))
            if name == "excluded" and call.endswith("adaptive"):
                assert [(r["trust"], r["flags"]) for r in recs] == [(1.0, 2)] * len(RAGGED)
            else:
                assert not recs.view(np.uint8).any()
        finally:
            gpu.free()
    assert out[0] == out[1]


def _raw_bytes_context():
    from crossbow_amd import TheGPU
    gpu = TheGPU()
    gpu.init([0])
    gpu.setModel(1, 4 * sum(RAGGED))  # registered as raw bytes
    gpu.setUpdateModelType(WORKER)
    gpu.setMomentum(0.9, 0)
    gpu.setLearningRateDecayPolicyFixed(LR)
    gpu.setModelWorkPerClock(2)
    gpu.setModelManager(2, 0)
    return gpu


REFUSALS = {
    "update model 7": (lambda s: context(RAGGED, s.enable, 2, 0.9, 1e-4, _mults(RAGGED, False), 2, 7), lambda g: None,
                       "cbx_step_and_synchronise_adaptive"),
    "clipping": (lambda s: context(RAGGED, s.enable, 2, 0.9, 1e-4, _mults(RAGGED, False), 2),
                 lambda g: g.set_gradient_clip(1.0), "cbx_set_gradient_clip"),
    "raw bytes": (lambda s: _raw_bytes_context(), lambda g: None, "turn them off for cbx_step_and_synchronise_ssgd"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing_and_name_the_call_to_take(name):
    from crossbow_amd import _lib
    make, prepare, names = REFUSALS[name]
    state = SsgdState(RAGGED, 2, 0.9, 2)
    gpu = make(state)
    try:
        gpu.set_adaptive_rate(ETA, EPS, 0)
        prepare(gpu)
        state.upload(gpu)
        gpu.lockAny()
        with pytest.raises(_lib.CbxError) as e:
            gpu.step_and_synchronise_ssgd_adaptive(0, 1, 0, [3, 5])
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED and names in str(e.value), str(e.value)
        assert "cbx_step_and_synchronise_ssgd_adaptive" in str(e.value)
        _compare(gpu, state, name + ": ")
        if name != "raw bytes":  # which has no records to read
            assert not gpu.base_adaptive_stats(0, len(RAGGED)).view(np.uint8).any()
        assert [(gpu.replica_copy(i), gpu.replica_clock(i)) for i in range(2)] == [(0, 0)] * 2
    finally:
        gpu.free()
