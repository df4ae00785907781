"""The clipped fused task-step barrier on IEEE edge values (run with -m gpu):
the fused catalogue of tests/edge_values.py, in the bulk and in the last
n mod 1,024 floats, through cbx_sma_plan_step_and_optimise_clipped and
cbx_step_and_synchronise_clipped, held to rules 1-3 of DESIGN.md's edge-value
contract: where the oracle has a NaN the device has a NaN, everywhere else the
32 bits are equal, and a value that is only copied keeps every bit.

The catalogue puts +-FLT_MAX, infinities and NaNs into every stepping replica's
g, so K > 0 and S = k * FLT_MAX^2 for a k below 32: each square has 48
significant bits, every partial sum of them is exact in fp64, and whatever else
g holds lies below half an ulp of it.  S is therefore the same bits in any
order, and the expectation takes the host's (the device's record is held to
it).  With the skip off, three values of max_norm give the three regimes of the
scale c / sqrt(S):

  c = 2^127    a normal scale near 0.5 / sqrt(k): scale * g stays normal
  c = 1        a subnormal scale: scale * g underflows
  c = FLT_MIN  the scale rounds to zero: scale * g is a signed zero, or NaN at an infinity

With the skip on every stepping replica is skipped: w as the step sees it, g
and last, signalling NaNs with payloads among them, keep every bit, and s is
the bit copy of w.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import edge_values as E
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact, upload
from tests.test_gpu_edge_values import MASKS
from tests.test_gpu_seam_step_and_optimise import DISCARD, Data
from tests.test_gpu_seam_step_and_optimise_clipped import ClipBuffers, ClipData

pytestmark = pytest.mark.gpu

N, WD = E.N, E.WD
SCALES = {"normal": 2.0 ** 127, "subnormal": 1.0, "zero": float(E.f32(E.FLT_MIN))}
SEAM_CONFIGS = {"mom-wd": (0.9, WD, 0.9), "plain": (0.0, 0.0, 0.0), "base-mom-only": (0.0, WD, 0.9)}
CONTEXT_CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD)}


class EdgeData(ClipData):
    def __init__(self, R, rmom, bmom):
        Data.__init__(self, N, R, rmom, bmom)  # ordinary data; the catalogue is written over it
        self.slots = list(range(R))
        self.max_norm = None


def _data(R, rmom, wd, bmom, rates, steps):
    d, d0 = EdgeData(R, rmom, bmom), EdgeData(R, rmom, bmom)
    labels = E.fused_case(d, rmom, wd, rates, steps)
    E.fused_case(d0, rmom, wd, rates, steps)
    return d, d0, labels


def test_the_three_regimes_of_the_scale():
    d, _, _ = _data(3, 0.9, WD, 0.9, E.replica_rates(3), [True] * 3)
    fmax2 = float(E.f32(E.FLT_MAX)) ** 2
    for g in d.g:
        S, K = C.exact_sum_sq(g)
        k = S / fmax2
        assert K > 0 and k == int(k) and 0 < k < 32, (S, K, k)  # S is k squares of FLT_MAX, exact in any order
        scales = {name: C.decide(S, K, c, False)[0] for name, c in SCALES.items()}
        assert 2.0 ** -126 <= scales["normal"] < 1 and np.isfinite(np.float32(0.01) * scales["normal"])
        assert E.is_subnormal(np.array([scales["subnormal"]], np.float32))[0]
        assert scales["zero"] == 0.0
        assert E.is_subnormal(np.array([np.float32(0.01) * scales["subnormal"]], np.float32))[0] or \
            np.float32(0.01) * scales["subnormal"] == 0


def _check(read, d, d0, labels, steps, keep, skipped, records):
    """_check_fused of tests/test_gpu_edge_values.py for the clipped step: a kept g
    is always written, and a skipped replica's g and last keep every bit."""
    st = d.st
    E.assert_edge_equal(read("z", 0), st.z[0], "z", labels)
    if st.last is not None:
        E.assert_edge_equal(read("blast", 0), st.last[0], "base last", labels)
    for name in ("z", "w0", "w1"):
        a = st.z[0] if name == "z" else st.w[int(name[1])]
        assert E.nan_fraction(a) < 0.25, f"the oracle's {name} holds {E.nan_fraction(a):.2%} NaNs"
    for i in range(st.size):
        E.assert_edge_equal(read("w", i), st.w[i], f"w[{i}]", labels)
        if steps[i] and keep:
            assert_bitexact(read("s", i), d0.st.w[i], f"s[{i}] is a copy of the old w")
            assert_bitexact(st.s[i], d0.st.w[i], "the oracle's s")
        else:
            assert_bitexact(read("s", i), d0.st.s[i], f"s[{i}] is not written")
        if steps[i] and keep and not skipped:
            E.assert_edge_equal(read("g", i), d.g[i], f"g[{i}]", labels)
        else:
            assert_bitexact(read("g", i), d0.g[i], f"g[{i}] keeps every bit")
        if d.last[i] is not None:
            if steps[i] and not skipped:
                E.assert_edge_equal(read("r", i), d.last[i], f"last[{i}]", labels)
            else:
                assert_bitexact(read("r", i), d0.last[i], f"last[{i}] keeps every bit")
        if steps[i]:  # the record is the host's: S exact, K, the scale's bits, the flags
            rec, want = records[i], d.decision[i]
            assert {k: rec[k] for k in want} == want, (i, rec, want)
            assert bool(rec["flags"] & C.SKIPPED) == skipped


def _steps(mask):
    R, who = MASKS[mask]
    return R, [who is None or i in who for i in range(R)]


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
    skip = scale == "skipped"
    c = SCALES["normal" if skip else scale]
    d, d0, labels = _data(R, rmom, wd, bmom, rates, steps)
    buf = ClipBuffers(d)
    with SmaPlan([0], N) as plan:
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
    from tests.test_gpu_step_and_synchronise import _exp, _gpu, _rates
    momentum, wd = CONTEXT_CONFIGS[config]
    R, steps = _steps(mask)
    tasks = [3 + 2 * i if steps[i] else -1 for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    skip = scale == "skipped"
    c = SCALES["normal" if skip else scale]
    d, d0, labels = _data(R, momentum, wd, momentum, rates, steps)
    gpu = _gpu(N, R, momentum, wd, _exp)
    try:
        gpu.set_gradient_clip(c, skip)
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        assert gpu.lockAny() == R
        gpu.step_and_synchronise_clipped(0, 1, 0, tasks, None, flags)
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
