"""The numpy oracle of gradient clipping by global norm (include/crossbow_sma.h,
cbx_set_gradient_clip), shared by the context's and the seam's GPU tests:

1. S by exact fp64 on the host (``math.fsum`` of the exact squares);
2. the decision and the scale as the header defines them;
3. ``g <- np.float32(scale) * g``;
4. then ``oracle.sma_optimise`` (or ``per_variable_step``) unchanged.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from tests.helpers import bits

CLIPPED, SKIPPED = 1, 2
LR = 0.05


def exact_sum_sq(g: np.ndarray):
    """(S, K): the correctly rounded sum of squares of the finite floats and
    the count of the others."""
    fin = np.isfinite(g)
    x = g[fin].astype(np.float64)
    return math.fsum((x * x).tolist()), int(g.size - np.count_nonzero(fin))  # x * x is exact: 48 bits


def decide(S: float, K: int, c: float, skip: bool):
    """(scale, flags) from S and K, with the header's arithmetic."""
    c64 = float(np.float32(c))
    clipped = c64 > 0 and S > c64 * c64
    scale = np.float32(c64 / np.sqrt(np.float64(S))) if clipped else np.float32(1.0)
    skipped = bool(skip) and K > 0
    return scale, (CLIPPED if clipped else 0) | (SKIPPED if skipped else 0)


def step(bufs, scale, flags, momentum, wd, lr=LR, variables=None, mults=None):
    """The expected step in place on [w, g, last, s]."""
    w, g, last, s = bufs
    if flags & SKIPPED:
        s[:] = w
        return
    with np.errstate(all="ignore"):
        g[:] = np.float32(scale) * g
    if variables is None:
        O.sma_optimise(np.float32(-lr), momentum, wd, w, g, last, s)
    else:
        from tests.test_optimise_plan import per_variable_step
        per_variable_step(lr, mults, momentum, wd, w, g, last, s, variables=variables)


def host(seed, n, momentum, sigma_g=0.01):
    """w, g, last, s on the host; s holds a pattern of its own, so an
    unwritten float is told from a written one."""
    w = O.fill_normal(n, seed, 0.05)
    g = O.fill_normal(n, seed + 1, sigma_g)
    last = O.fill_normal(n, seed + 2, 0.001) if momentum > 0 else None
    s = O.fill_normal(n, seed + 3, 7.0)
    return [w, g, last, s]


def exact_gradient(n):
    """Small integers, so S is exact in any order: +-2 on up to 4,096 elements
    spread over the buffer, zeros elsewhere.  Returns (g, S, c) with
    c / sqrt(S) = 0.5 exactly."""
    g = np.zeros(n, np.float32)
    m = min(n, 4096)
    # a power of four elements, so sqrt(S) is a power of two
    m = 4 ** int(math.log(m, 4) + 1e-9)
    idx = (np.arange(m, dtype=np.int64) * n) // m
    g[idx] = np.where(np.arange(m) % 3 == 0, -2.0, 2.0).astype(np.float32)
    S = 4.0 * m
    return g, S, math.sqrt(S) / 2.0


def assert_same_with_nans(got, want, what):
    """Bit for bit, except that a NaN only has to be a NaN."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    a, b = bits(got)[~gn], bits(want)[~wn]
    if not np.array_equal(a, b):
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {bad.size} of {a.size} non-NaN elements differ; first at {bad[0]}")


def nonfinite_positions(n):
    """Element 0, n - 1 and one in a second tile, as far as n has them."""
    return sorted({0, n - 1} | ({4096 + 5} if n > 4096 + 5 else set()))
