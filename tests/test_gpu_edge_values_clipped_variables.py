"""The clipped fused task-step barrier with a learning rate per variable on IEEE
edge values (run with -m gpu): the fused catalogue of tests/edge_values.py, in
the bulk and in the last n mod 1,024 floats, through
cbx_sma_plan_step_and_optimise_clipped_variables and
cbx_step_and_synchronise_clipped_variables, held to rules 1-3 of DESIGN.md's
edge-value contract (section 4): where the oracle has a NaN the device has a
NaN, everywhere else the 32 bits are equal, and a value that is only copied
keeps every bit.

The scales are tests/test_gpu_edge_values_clipped.py's: S = k * FLT_MAX^2 is the
same bits in any order, so the expectation takes the host's, and with the skip
off three values of max_norm give a normal scale, a subnormal scale and a scale
that rounds to zero.  With the skip on every stepping replica is skipped over
signalling NaNs with payloads: w as the step sees it, g and last keep every
bit, and s is the bit copy of w.

The multipliers are 2^-126, 3, 2 and 0.5, none of them 1: every rate here lies
below 1/4, so rate x 2^-126 is a subnormal.  (A product that overflows, as in
tests/test_gpu_edge_values_variables.py, would turn a quarter of a replica's
floats into NaN under the scale that rounds to zero, 0 x inf: more than the
quarter a compared array may hold.)  The variables put each multiplier in a
uniform chunk of the bulk, in chunks with boundaries inside (50-float variables
cycling through the four) and in the seam's tail (floats from 2,048 on).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import edge_values as E
from tests.helpers import assert_bitexact, upload
from tests.test_gpu_edge_values_clipped import CONTEXT_CONFIGS, SCALES, SEAM_CONFIGS, _check, _steps
from tests.test_gpu_edge_values import MASKS
from tests.test_gpu_seam_step_and_optimise import DISCARD, Data
from tests.test_gpu_seam_step_and_optimise_clipped_variables import BothBuffers, BothData

pytestmark = pytest.mark.gpu

N = E.N
CYCLE = (2.0 ** -126, 3.0, 2.0, 0.5)


def _model():
    variables, mults = [256], [2.0 ** -126]
    at, k = 256, 0
    while at < 1792:
        c = min(50, 1792 - at)
        variables.append(c), mults.append(CYCLE[k % 4])
        at, k = at + c, k + 1
    variables.append(256), mults.append(3.0)
    at = 2048
    while at < N:
        c = min(50, N - at)
        variables.append(c), mults.append(CYCLE[k % 4])
        at, k = at + c, k + 1
    assert sum(variables) == N and all(m not in (0.0, 1.0) for m in mults)
    return tuple(variables), tuple(mults)


VARS, MULTS = _model()


class EdgeData(BothData):
    def __init__(self, R, rmom, bmom):
        Data.__init__(self, N, R, rmom, bmom)  # ordinary data; the catalogue is written over it
        self.variables, self.mults = VARS, MULTS
        self.slots = list(range(R))
        self.max_norm = None


def _data(R, rmom, wd, bmom, rates, steps):
    d, d0 = EdgeData(R, rmom, bmom), EdgeData(R, rmom, bmom)
    labels = E.fused_case(d, rmom, wd, rates, steps)
    E.fused_case(d0, rmom, wd, rates, steps)
    return d, d0, labels


def _subnormal_products(rates, steps):
    for r, s in zip(rates, steps):
        if s:
            p = np.array([np.float32(-r) * np.float32(2.0 ** -126)], np.float32)
            assert E.is_subnormal(p)[0], (r, p)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("scale", list(SCALES) + ["skipped"])
@pytest.mark.parametrize("config", list(SEAM_CONFIGS))
def test_seam(config, scale, mask, flags):
    import torch

    from crossbow_amd.seam import SmaPlan
    rmom, wd, bmom = SEAM_CONFIGS[config]
    R, steps = _steps(mask)
    rates = E.replica_rates(R)
    _subnormal_products(rates, steps)
    skip = scale == "skipped"
    c = SCALES["normal" if skip else scale]
    d, d0, labels = _data(R, rmom, wd, bmom, rates, steps)
    buf = BothBuffers(d)
    with SmaPlan([0], N) as plan:
        plan.set_variables(list(VARS), list(MULTS))
        got = buf.call(plan, steps, rates, wd, flags, c=c, skip=skip)
        buf.stream.synchronize()
        records = [plan.clip_stats(0, d.slots[i], buf.stream.cuda_stream) if steps[i] else None for i in range(R)]
    with np.errstate(all="ignore"):
        assert got == d.step(steps, rates, wd, keep=flags == 0, c=c, skip=skip) == 0
    torch.cuda.synchronize()
    table = {"z": [buf.z], "blast": [buf.blast], "w": buf.w, "s": buf.s, "g": buf.g, "r": buf.last}
    _check(lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, flags == 0, skip, records)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("scale", list(SCALES) + ["skipped"])
@pytest.mark.parametrize("config", list(CONTEXT_CONFIGS))
def test_context(config, scale, mask, flags):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    from tests.test_gpu_step_and_synchronise import _exp, _rates
    from tests.test_gpu_step_and_synchronise_variables import _gpu
    momentum, wd = CONTEXT_CONFIGS[config]
    R, steps = _steps(mask)
    tasks = [3 + 2 * i if steps[i] else -1 for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    _subnormal_products(rates, steps)
    skip = scale == "skipped"
    c = SCALES["normal" if skip else scale]
    d, d0, labels = _data(R, momentum, wd, momentum, rates, steps)
    gpu = _gpu(R, momentum, wd, _exp, variables=VARS, mults=MULTS)
    try:
        gpu.set_gradient_clip(c, skip)
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_clipped_variables(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        with np.errstate(all="ignore"):
            assert d.step(steps, rates, wd, keep=flags == 0, c=c, skip=skip) == 0
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "r": BUF_LAST}

        def read(kind, i):
            if kind in ("z", "blast"):
                return gpu.base_read(0, BUF_DATA if kind == "z" else BUF_LAST)
            return gpu.replica_read(i, kinds[kind])
        records = [gpu.replica_clip_stats(i) if steps[i] else None for i in range(R)]
        _check(read, d, d0, labels, steps, flags == 0, skip, records)
    finally:
        gpu.free()
