"""The fused task-step barrier with per-variable rates on IEEE edge values
(run with -m gpu): the inputs of tests/edge_values.py through
cbx_step_and_synchronise_variables and cbx_sma_plan_step_and_optimise_variables,
held to rules 1-3 of DESIGN.md's edge-value contract by
tests/test_gpu_edge_values.py's own comparison (``_check_fused``).

The multipliers are 2^-126, 0.5, 3 and 2^127, the rates 4 for replica 0 and
below 1/8 for the others, so rate x multiplier underflows to a subnormal
(0.0625 x 2^-126), stays normal, and overflows to an infinity (4 x 2^127), and
no multiplier is an exact 0.  The variables put each class in a uniform chunk
of the bulk (floats [0, 256) and [1792, 2048)), in chunks with boundaries
inside (50-float variables cycling through the four), and in the seam's tail
(floats from 2,048 on, the same cycle).  The oracle's output is checked to
hold NaNs in less than a quarter of every compared array before the device is
compared.  One separate test pins multiplier 0 over a non-finite g: the product
form gives NaN (rule 4).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import edge_values as E
from tests.helpers import assert_bitexact, upload
from tests.test_gpu_edge_values import MASKS, _check_fused
from tests.test_gpu_seam_step_and_optimise import DISCARD
from tests.test_gpu_seam_step_and_optimise_variables import VarBuffers, VarData

pytestmark = pytest.mark.gpu

N, ALPHA, WD = E.N, E.ALPHA, E.WD
CYCLE = (2.0 ** -126, 3.0, 2.0 ** 127, 0.5)


def _model():
    variables, mults = [256], [2.0 ** -126]
    at, k = 256, 0
    while at < 1792:
        c = min(50, 1792 - at)
        variables.append(c), mults.append(CYCLE[k % 4])
        at, k = at + c, k + 1
    variables.append(256), mults.append(2.0 ** 127)
    at = 2048
    while at < N:
        c = min(50, N - at)
        variables.append(c), mults.append(CYCLE[k % 4])
        at, k = at + c, k + 1
    assert sum(variables) == N and all(m != 0.0 for m in mults)
    return tuple(variables), tuple(mults)


VARS, MULTS = _model()
RATES = (4.0, 0.0625, 0.015625)  # 8 x 0.5^(task + 1) at tasks 0, 6, 8: the context's exponential policy gives the same


def _rates(R):
    """4 for replica 0, distinct rates of 1/16 and below for the others, exact in fp32."""
    return [RATES[0]] + [float(np.float32(RATES[1] / (1.0 + 0.37 * i))) for i in range(R - 1)]


def test_the_products_underflow_stay_normal_and_overflow():
    r = np.float32(-RATES[1])
    assert E.is_subnormal(np.array([r * np.float32(2.0 ** -126)], np.float32))[0]
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(-RATES[0]) * np.float32(2.0 ** 127))
    for m in (0.5, 3.0):
        p = np.array([r * np.float32(m)], np.float32)
        assert np.isfinite(p[0]) and not E.is_subnormal(p)[0] and p[0] != 0


def _data(R, rmom, wd, bmom, steps):
    """The fused catalogue as tests/edge_values.py writes it for its own rates
    (its fma ties are tuned to a rate below 1/4; under a multiplier no rate of
    this test is that rate anyway)."""
    d = VarData(VARS, MULTS, R, rmom, bmom)
    labels = E.fused_case(d, rmom, wd, E.replica_rates(R), steps)
    d0 = VarData(VARS, MULTS, R, rmom, bmom)
    E.fused_case(d0, rmom, wd, E.replica_rates(R), steps)
    return d, d0, labels


def _nans_within_a_quarter(d):
    st = d.st
    arrays = {"z": st.z[0]}
    if st.last is not None:
        arrays["base last"] = st.last[0]
    for i in range(st.size):
        arrays.update({f"w[{i}]": st.w[i], f"s[{i}]": st.s[i], f"g[{i}]": d.g[i]})
        if d.last[i] is not None:
            arrays[f"last[{i}]"] = d.last[i]
    for name, a in arrays.items():
        assert E.nan_fraction(a) < 0.25, f"the oracle's {name} holds {E.nan_fraction(a):.2%} NaNs"


SEAM_CONFIGS = {"mom-wd": (0.9, WD, 0.9), "plain": (0.0, 0.0, 0.0), "base-mom-only": (0.0, WD, 0.9)}


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(SEAM_CONFIGS))
def test_seam(config, mask, flags):
    import torch

    from crossbow_amd.seam import SmaPlan
    rmom, wd, bmom = SEAM_CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    rates = _rates(R)
    d, d0, labels = _data(R, rmom, wd, bmom, steps)
    buf = VarBuffers(d)
    with SmaPlan([0], N) as plan:
        plan.set_variables(list(VARS), list(MULTS))
        got = buf.call(plan, steps, rates, wd, flags)
        buf.stream.synchronize()
    with np.errstate(all="ignore"):
        assert got == d.step(steps, rates, wd, keep=flags == 0) == 0
    _nans_within_a_quarter(d)
    torch.cuda.synchronize()
    table = {"z": [buf.z], "blast": [buf.blast], "w": buf.w, "s": buf.s, "g": buf.g, "r": buf.last}
    _check_fused(lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, rmom, wd, flags == 0, False)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")


def _context(R, momentum, wd, variables=VARS, mults=MULTS):
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(len(variables), 4 * sum(variables))
    for v, count in enumerate(variables):
        g.setModelVariable(v, 1, [count], 4 * count)
        g.setModelVariableLearningRateMultiplier(v, 1, mults[v])
    g.setUpdateModelType(7)
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, 0)
    g.setWeightDecay(wd)
    g.setLearningRateDecayPolicyExp(8.0, 0.5)
    g.setModelManager(R, 0)
    g.set_variable_learning_rates(True)
    return g


CONTEXT_CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD)}


def _context_tasks(R, steps):
    """Replica 0 at task 0 (rate 4), the others at tasks from 6 on (rates of 1/16 and below)."""
    return [(0 if i == 0 else 5 + i) if steps[i] else -1 for i in range(R)]


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(CONTEXT_CONFIGS))
def test_context(config, mask, flags):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    momentum, wd = CONTEXT_CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    tasks = _context_tasks(R, steps)
    twin = _context(R, momentum, 0.0, (4,), (1.0,))
    try:
        rates = [twin.replica_learning_rate(i, t) if t >= 0 else 0.0 for i, t in enumerate(tasks)]
    finally:
        twin.free()
    assert rates[0] == 4.0 and all(0 < r <= 0.0625 for r, s in zip(rates[1:], steps[1:]) if s), rates
    d, d0, labels = _data(R, momentum, wd, momentum, steps)
    gpu = _context(R, momentum, wd)
    try:
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_variables(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            assert d.step(steps, rates, wd, keep=flags == 0) == 0
        _nans_within_a_quarter(d)
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "r": BUF_LAST}

        def read(kind, i):
            if kind in ("z", "blast"):
                return gpu.base_read(0, BUF_DATA if kind == "z" else BUF_LAST)
            return gpu.replica_read(i, kinds[kind])
        _check_fused(read, d, d0, labels, steps, momentum, wd, flags == 0, False)
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_multiplier_zero_over_a_nonfinite_gradient_is_nan(momentum):
    # rule 4: r = rate x 0 is a zero, and 0 x inf (the product, or the fma without momentum) is NaN,
    # not "the variable is frozen"
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST
    variables, mults, R = (300, 700), (0.0, 2.0), 2
    n = sum(variables)
    d = VarData(variables, mults, R, momentum, momentum)
    hit = [3, 150, 299]  # variable 0: bulk lanes of a mixed chunk and of a uniform one
    for i in range(R):
        d.g[i].view(np.uint32)[hit] = [E.PINF, E.NINF, E.QNAN]
    tasks = [0, 6]
    gpu = _context(R, momentum, 0.0, variables, mults)
    try:
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        gpu.lockAny()
        gpu.step_and_synchronise_variables(0, 1, 0, tasks, None, 0)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            d.step([True] * R, [4.0, 0.0625], 0.0)
        for i in range(R):
            assert np.isnan(d.st.w[i][hit]).all(), "the oracle: 0 x inf is NaN"
            got = gpu.replica_read(i, BUF_DATA)
            assert np.isnan(got[hit]).all(), f"w[{i}] at the non-finite gradients: {got[hit]}"
            E.assert_edge_equal(got, d.st.w[i], f"w[{i}]")
            if momentum > 0:
                E.assert_edge_equal(gpu.replica_read(i, BUF_LAST), d.last[i], f"last[{i}]")
        assert E.nan_fraction(d.st.z[0]) < 0.25
        E.assert_edge_equal(gpu.base_read(0, BUF_DATA), d.st.z[0], "z")
        assert n == 1000
    finally:
        gpu.free()
