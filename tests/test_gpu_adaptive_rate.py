"""GPU parity of the replica step with layer-wise adaptive rates (``cbx_set_adaptive_rate``,
``cbx_sma_plan_optimise_adaptive``; adaptive_rate_kernels.hip).  The reference is numpy and ``math``:
rule 1 by ``math.fsum`` over exact products, rule 2 in float64 with ``math.sqrt``, rule 3 by the oracle's
replica step once per variable with the rate ``(-lr * m_v) * t_v`` formed in fp32 in that order.  In the
exact regime (integers |k| <= 2^10 times one power of two per buffer, so every partial sum is exact in any
order) no device value enters an expectation; on normal data W_v and G_v are held to the reordering bound
2 m 2^-53 sum|term| and the ratio and the step are restated from the device's own sums.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import oracle as O
from tests.edge_values import assert_edge_equal
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-9
RAGGED = (1, 3, 35, 4093, 4096, 1000)  # tests/test_gpu_stats.py: boundaries inside a float4, a chunk, at a tile
SHAPES = {"ragged": RAGGED, "ragged0": RAGGED[:3] + (0,) + RAGGED[3:], "one": (9095,), "small": (771,)}
APPLIED, EXCLUDED, DEGENERATE, CAPPED = 1, 2, 4, 8
# momentum, weight decay, (unroll, policy), mode, trust, multipliers: every value of each with each path
CASES = [(0.0, 0.0, (1, 1), 0, 0.05, False), (0.9, 1e-4, (2, 0), 1, 0.05, True), (0.9, 0.0, (1, 0), 1, 0.05, False),
         (0.0, 1e-4, (2, 1), 0, 0.05, True)]


def _data(variables, exact, momentum, seed=7):
    """w, g, last, s and the enable list.  In the ragged lists the variable of 3 floats has w all zero,
    the one of 35 has g all +0 and -0, the one of 1000 is excluded, the one of 4093 holds a NaN and an
    inf in g, and the one of 4096 has small weights, so that mode 1 caps some ratios and not others."""
    n, rng = sum(variables), np.random.default_rng(seed)
    if exact:
        w = (rng.integers(-1024, 1025, n) * 2.0 ** -7).astype(np.float32)
        g = (rng.integers(-1024, 1025, n) * 2.0 ** -12).astype(np.float32)
    else:
        w, g = O.fill_normal(n, seed, 1.0), O.fill_normal(n, seed + 1, 1e-2)
    last = O.fill_normal(n, seed + 2, 1e-3) if momentum > 0 else None
    enable, lo = [], 0
    for count in variables:
        v = slice(lo, lo + count)
        if len(variables) > 1 and exact:
            if count == 3:
                w[v] = 0.0
            elif count == 35:
                g[v] = np.where(np.arange(count) % 2, -0.0, 0.0)
            elif count == 4093:
                g[lo + 5], g[lo + 4092] = np.nan, np.inf
            elif count == 4096:
                w[v] = (rng.integers(-8, 9, count) * 2.0 ** -7).astype(np.float32)
        enable.append(not (len(variables) > 1 and count == 1000))
        lo += count
    return [w, g, last, O.fill_normal(n, seed + 3, 7.0)], enable


def _trust(W, G, K, count, on, eta, beta, mode):
    """Rule 2: (t_v, flags)."""
    if not on:
        return np.float32(1), EXCLUDED
    if count == 0:
        return np.float32(1), 0
    if W == 0.0 or G == 0.0 or K > 0:
        return np.float32(1), DEGENERATE
    nw, ng = math.sqrt(W), math.sqrt(G)
    den = (ng + float(np.float32(beta)) * nw) + float(np.float32(EPS))
    t = np.float32((float(np.float32(eta)) * nw) / den)
    return (np.float32(1), APPLIED | CAPPED) if mode == 1 and t > 1 else (t, APPLIED)


def _reference(variables, enable, bufs, mults, momentum, wd, eta, mode, device=None):
    """Rules 1 to 3 in place on ``bufs``; returns the expected records.  ``device``: the device's records,
    whose W_v and G_v then stand in for the sums (normal data) after the bound on them has been checked."""
    w, g, last, s = bufs
    recs, lo = [], 0
    for v, count in enumerate(variables):
        sl = slice(lo, lo + count)
        sq = [[float(x) * float(x) for x in a[sl][np.isfinite(a[sl])]] for a in (w, g)]  # exact products
        W, G = math.fsum(sq[0]), math.fsum(sq[1])
        K = int(np.sum(~np.isfinite(w[sl])) + np.sum(~np.isfinite(g[sl])))
        if device is not None:
            for got, want, terms in ((device["w_sq"][v], W, sq[0]), (device["g_sq"][v], G, sq[1])):
                assert abs(got - want) <= 2 * len(terms) * 2.0 ** -53 * want, (v, got, want)
            W, G = float(device["w_sq"][v]), float(device["g_sq"][v])
        t, flags = _trust(W, G, K, count, enable[v], eta, wd, mode)
        recs.append((W, G, K, t, flags))
        if count:
            rate = (np.float32(-LR) * np.float32(mults[v])) * t
            O.sma_optimise(rate, momentum, wd, w[sl], g[sl], last[sl] if last is not None else None, s[sl])
        lo += count
    return recs


def _check_records(got, want):
    assert len(got) == len(want)
    for v, (W, G, K, t, flags) in enumerate(want):
        r = got[v]
        assert (r["w_sq"], r["g_sq"], r["nonfinite"], r["flags"]) == (W, G, K, flags), (v, r, want[v])
        assert np.float32(r["trust"]).view(np.uint32) == np.float32(t).view(np.uint32), (v, r, want[v])


def _context(variables, enable, momentum, wd, mults=None, update_type=7):
    from crossbow_amd import TheGPU
    gpu = TheGPU()
    gpu.init([0])
    gpu.setModel(len(variables), 4 * sum(variables))
    for v, count in enumerate(variables):
        gpu.setModelVariable(v, 1, [count], 4 * count)
        if mults and mults[v] != 1.0:
            gpu.setModelVariableLearningRateMultiplier(v, 1, mults[v])
        if not enable[v]:
            gpu.set_model_variable_adaptive_rate(v, 1, False)
    gpu.setUpdateModelType(update_type)
    gpu.setEamsgdAlpha(0.1)
    gpu.setMomentum(momentum, 0)
    gpu.setWeightDecay(wd)
    gpu.setLearningRateDecayPolicyFixed(LR)
    gpu.setModelManager(1, 0)
    return gpu


def _kinds():
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    return (BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF)


def _put(gpu, bufs):
    for kind, a in zip(_kinds(), bufs):
        if a is not None:
            gpu.replica_write(0, kind, a)


def _check(gpu, bufs, what):
    for kind, name, a in zip(_kinds(), "wgls", bufs):
        if a is not None:
            assert_edge_equal(gpu.replica_read(0, kind), a, f"{what}: {name}")


def _mults(variables, on):
    return [2.0 if on and v == 4 % len(variables) else 1.0 for v in range(len(variables))]


def _context_step(variables, exact, momentum, wd, shape, mode, eta, multipliers):
    bufs, enable = _data(variables, exact, momentum)
    mults = _mults(variables, multipliers)
    gpu = _context(variables, enable, momentum, wd, mults)
    try:
        gpu.set_variable_learning_rates(multipliers)
        gpu.set_aux_kernel_config(64, shape[0], -1)
        gpu.set_adaptive_kernel_policy(shape[1])
        assert not gpu.replica_adaptive_stats(0, len(variables)).view(np.uint8).any()  # all zeros before the first step
        gpu.set_adaptive_rate(eta, EPS, mode)
        _put(gpu, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        recs = gpu.replica_adaptive_stats(0, len(variables))
        want = _reference(variables, enable, bufs, mults, momentum, wd, eta, mode, None if exact else recs)
        _check_records(recs, want)
        _check(gpu, bufs, "context")
        return recs.tobytes()
    finally:
        gpu.free()


def _seam_step(variables, exact, momentum, wd, mode, eta, multipliers, repeat=1):
    import torch
    from crossbow_amd.seam import SmaPlan
    bufs, enable = _data(variables, exact, momentum)
    mults = _mults(variables, multipliers)
    stream, out = torch.cuda.Stream(), []
    with SmaPlan([0], sum(variables)) as plan:
        plan.set_variables(list(variables), mults)
        plan.set_adaptive(enable, slots=2)
        assert not plan.adaptive_stats(0, 1, stream.cuda_stream, len(variables)).view(np.uint8).any()
        for k in range(repeat):  # a repeat goes through the measuring entry: the same launches, timed
            dev = [Guarded(a, tag) if a is not None else None for tag, a in enumerate(bufs)]
            step = plan.optimise_adaptive_timed if k else plan.optimise_adaptive
            ms = step(0, 1, stream.cuda_stream, dev[0].ptr, dev[1].ptr, dev[2].ptr if dev[2] else None, dev[3].ptr,
                      LR, momentum, wd, eta, EPS, mode)
            assert ms is None or all(x > 0 for x in ms), ms
            out.append(plan.adaptive_stats(0, 1, stream.cuda_stream, len(variables)))
        want = _reference(variables, enable, bufs, mults, momentum, wd, eta, mode, None if exact else out[-1])
        _check_records(out[-1], want)
        for name, d, a in zip("wgls", dev, bufs):
            if a is not None:
                host = d.t.cpu().numpy()
                assert_edge_equal(host[:d.n], a, f"seam: {name}")
                assert np.array_equal(host[d.n:].view(np.uint32), d.sentinel.view(np.uint32)), f"behind {name}"
    return [r.tobytes() for r in out]


@pytest.mark.parametrize("momentum, wd, shape, mode, eta, multipliers", CASES)
@pytest.mark.parametrize("variables", ["ragged", "ragged0", "one"])
def test_context_step_in_the_exact_regime(variables, momentum, wd, shape, mode, eta, multipliers):
    _context_step(SHAPES[variables], True, momentum, wd, shape, mode, eta, multipliers)


# the seam runs one launch shape (aux_launch_config: unroll 1, nontemporal), so CASES without theirs
@pytest.mark.parametrize("momentum, wd, mode, eta, multipliers", [c[:2] + c[3:] for c in CASES])
@pytest.mark.parametrize("variables", ["ragged", "ragged0", "one", "small"])
def test_seam_step_in_the_exact_regime(variables, momentum, wd, mode, eta, multipliers):
    _seam_step(SHAPES[variables], True, momentum, wd, mode, eta, multipliers)


def test_normal_data_is_within_the_bound_repeatable_and_the_same_through_both_doors():
    args = (SHAPES["ragged"], False, 0.9, 1e-4)
    first, second = _seam_step(*args, 1, 0.002, True, repeat=2)
    assert first == second == _context_step(*args, (1, 1), 1, 0.002, True)


def test_switched_off_the_step_is_the_plain_one():
    bufs, enable = _data(RAGGED, False, 0.9)
    gpu = _context(RAGGED, enable, 0.9, 1e-4)
    try:
        gpu.set_adaptive_rate(0.05, EPS, 1)
        gpu.set_adaptive_rate(0.0, 0.0, 0)
        _put(gpu, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        O.sma_optimise(np.float32(-LR), 0.9, 1e-4, *bufs)
        _check(gpu, bufs, "off")
        assert not gpu.replica_adaptive_stats(0, len(RAGGED)).view(np.uint8).any()
    finally:
        gpu.free()


REFUSALS = {
    "worker": (1, lambda g: g.replica_optimise(0, task=0), "cbx_set_adaptive_rate"),
    "default": (0, lambda g: g.replica_optimise(0, task=0), "cbx_set_adaptive_rate"),
    "clipping": (7, lambda g: (g.set_gradient_clip(1.0), g.replica_optimise(0, task=0)), "cbx_set_gradient_clip"),
    "per-operator": (7, lambda g: g.replica_optimise_variables(0, task=0, op=1), "cbx_replica_optimise"),
    "fused": (7, lambda g: (g.lockAny(), g.step_and_synchronise(0, 1, 0, [0])), "cbx_synchronise"),
    "fused elastic": (3, lambda g: (g.setElasticAverage(True), g.lockAny(), g.step_and_synchronise_elastic(0, 1, 0, [0])),
                      "cbx_synchronise"),
    "fused ssgd": (1, lambda g: (g.lockAny(), g.step_and_synchronise_ssgd(0, 1, 0, [0])), "cbx_synchronise"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing_and_name_the_other_call(name):
    from crossbow_amd import _lib
    update_type, call, names = REFUSALS[name]
    bufs, enable = _data(RAGGED, True, 0.9)
    gpu = _context(RAGGED, enable, 0.9, 1e-4, update_type=update_type)
    try:
        gpu.set_adaptive_rate(0.05, EPS, 0)
        _put(gpu, bufs)
        with pytest.raises(_lib.CbxError) as e:
            call(gpu)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED and names in str(e.value), str(e.value)
        _check(gpu, bufs, name)
        assert not gpu.replica_adaptive_stats(0, len(RAGGED)).view(np.uint8).any()
    finally:
        gpu.free()


def test_a_model_without_variable_ranges_is_refused_as_the_per_variable_step_refuses_it():
    from crossbow_amd import TheGPU, _lib
    gpu = TheGPU()
    gpu.init([0])
    try:
        gpu.setModel(1, 4 * 771)  # registered as raw bytes
        gpu.setUpdateModelType(7)
        gpu.setLearningRateDecayPolicyFixed(LR)
        gpu.setModelManager(1, 0)
        gpu.set_adaptive_rate(0.05, EPS, 0)
        with pytest.raises(_lib.CbxError) as e:
            gpu.replica_optimise(0, task=0)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED and "no variables" in str(e.value)
    finally:
        gpu.free()


@pytest.mark.parametrize("trust, epsilon, mode", [(-1.0, 0.0, 0), (math.nan, 0.0, 0), (math.inf, 0.0, 0),
                                                  (0.1, -1.0, 0), (0.1, math.nan, 0), (0.1, 0.0, 2)])
def test_bad_arguments_are_invalid(trust, epsilon, mode):
    from crossbow_amd import TheGPU, _lib
    gpu = TheGPU()
    gpu.init([0])
    try:
        with pytest.raises(_lib.CbxError) as e:
            gpu.set_adaptive_rate(trust, epsilon, mode)
        assert e.value.code == _lib.CBX_ERR_INVALID
    finally:
        gpu.free()
