"""GPU parity of ``cbx_step_and_synchronise_elastic_adaptive`` (task_elastic_adaptive_kernels.hip).  The
reference is tests/test_gpu_adaptive_rate.py's per stepping replica (``math.fsum`` of exact products, rule 2 in
float64, the oracle's replica step per variable with ``(-lr * m_v) * t_v``), then the CPU restatement of the
elastic barrier.  w and g are in that file's exact regime, so no device value enters an expectation."""
from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests.edge_values import assert_edge_equal
from tests.test_gpu_adaptive_rate import EPS, RAGGED, SHAPES, _check_records, _mults, _trust
from tests.test_gpu_step_and_synchronise import _exp
from tests.test_gpu_step_and_synchronise_adaptive import CASES, ETA, PATHS, State, _context, _rates

pytestmark = pytest.mark.gpu

EAMSGD = 3  # CBX_UPDATE_SYNCHRONOUSEAMSGD


def _elastic(gpu):
    _exp(gpu)
    gpu.setElasticAverage(True)


def context(variables, enable, R, momentum, wd, mults, policy=_elastic, update_type=EAMSGD):
    return _context(variables, enable, R, momentum, wd, mults, policy, update_type)


class ElasticState(State):
    """State with the elastic barrier behind the replica steps: d comes from the stepped w."""

    def step(self, tasks, rates, mults, wd, mode, keep):
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
        with np.errstate(all="ignore"):
            AV.elastic_average(st)  # z and w; the base model's last is left alone
        if not keep:  # the device leaves s and g of a stepping replica alone
            for i, (s, g) in kept.items():
                st.s[i][:], self.g[i][:] = s, g
        return recs


def _fused(gpu, tasks, flags=0, clock=1):
    gpu.lockAny()
    gpu.step_and_synchronise_elastic_adaptive(0, clock, 0, tasks, None, flags)
    gpu.unlockAny()
    gpu.wait()


@pytest.mark.parametrize("momentum, wd, mode, multipliers, flags, shape", CASES)
@pytest.mark.parametrize("variables, tasks", PATHS)
def test_every_buffer_and_record_in_the_exact_regime(variables, tasks, momentum, wd, mode, multipliers, flags, shape):
    variables, R = SHAPES[variables], len(tasks)
    state, mults = ElasticState(variables, R, momentum), _mults(variables, multipliers)
    make = lambda: context(variables, state.enable, R, momentum, wd, mults)  # noqa: E731
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


def _both_doors(tasks, adaptive):
    """The fused call and the device's own sequence (with the rates off: the other elastic fused call) from the
    same normal data in two contexts: every buffer's and every record's bytes and the host state."""
    R, out = len(tasks), []
    state, mults = ElasticState(RAGGED, R, 0.9, exact=False), _mults(RAGGED, True)
    for fused in (True, False):
        gpu = context(RAGGED, state.enable, R, 0.9, 1e-4, mults)
        try:
            gpu.set_variable_learning_rates(True)
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
                else:
                    gpu.step_and_synchronise_elastic_clipped_variables(0, 7, 0, tasks)
                gpu.unlockAny()
                gpu.wait()
            bufs = {k: v.tobytes() for k, v in state.read(gpu).items()}
            recs = [gpu.replica_adaptive_stats(i, len(RAGGED)).tobytes() for i in range(R)]
            out.append((bufs, recs, [(gpu.replica_copy(i), gpu.replica_clock(i)) for i in range(R)]))
        finally:
            gpu.free()
    return out


@pytest.mark.parametrize("tasks, adaptive", [([3, -1, 7], True), ([3, 5], False), ([-1, -1], True)])
def test_the_fused_call_is_the_other_door_bit_for_bit(tasks, adaptive):
    fused, want = _both_doors(tasks, adaptive)
    assert fused == want
    assert [any(r) for r in fused[1]] == [adaptive and t >= 0 for t in tasks]  # records for the steppers only


REFUSALS = {
    "clipping": (EAMSGD, _elastic, lambda g: g.set_gradient_clip(1.0), "UNSUPPORTED", "cbx_set_gradient_clip"),
    "elastic off": (EAMSGD, _exp, lambda g: None, "UNSUPPORTED", "cbx_step_and_synchronise_adaptive"),
    "worker": (1, _exp, lambda g: None, "UNSUPPORTED", "cbx_set_adaptive_rate"),
    "not locked": (EAMSGD, _elastic, lambda g: g.unlockAny(), "INVALID", "not locked"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing_and_name_the_call_to_take(name):
    from crossbow_amd import _lib
    update_type, policy, prepare, code, names = REFUSALS[name]
    state, mults = ElasticState(RAGGED, 2, 0.9), _mults(RAGGED, False)
    gpu = context(RAGGED, state.enable, 2, 0.9, 1e-4, mults, policy, update_type)
    try:
        gpu.set_adaptive_rate(ETA, EPS, 0)
        state.upload(gpu)
        gpu.lockAny()
        prepare(gpu)
        with pytest.raises(_lib.CbxError) as e:
            gpu.step_and_synchronise_elastic_adaptive(0, 1, 0, [3, 5])
        assert e.value.code == getattr(_lib, "CBX_ERR_" + code) and names in str(e.value), str(e.value)
        assert "cbx_step_and_synchronise_elastic_adaptive" in str(e.value)
        got, want = state.read(gpu), state.want()
        for key in want:
            assert_edge_equal(got[key], want[key], f"{name}: {key}")
        assert not any(gpu.replica_adaptive_stats(i, len(RAGGED)).view(np.uint8).any() for i in range(2))
        assert [(gpu.replica_copy(i), gpu.replica_clock(i)) for i in range(2)] == [(0, 0)] * 2
    finally:
        gpu.free()
