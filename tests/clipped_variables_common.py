"""What the GPU tests of the clipped fused barrier with a learning rate per
variable share (cbx_step_and_synchronise_clipped_variables,
cbx_sma_plan_step_and_optimise_clipped_variables): gradients whose S is exact
in any summation order *and* that are non-zero in every variable, so that no
device value enters an expectation and every variable sees its multiplier even
with momentum and weight decay off.  Plain numpy: no GPU.

``tests.gradient_clip_common.exact_gradient`` leaves most floats zero: whole
small variables of ``V`` (tests/test_optimise_plan.py) would step by nothing.
"""
from __future__ import annotations

import math

import numpy as np

from tests import gradient_clip_common as C
from tests.test_optimise_plan import M, V

N = sum(V)  # 21,523 = 5 * 4,096 + 1,043: six norm tiles, the last partial
ONES, TWOS = 6_852, 14_671  # S = 6,852 + 4 * 14,671 = 65,536 = 256^2
MAX_NORM = 128.0  # scale exactly 0.5
KINDS = ("unclipped", "clipped", "skipped")
assert ONES + TWOS == N and ONES + 4 * TWOS == 256 ** 2


def spans(variables):
    lo = 0
    for count in variables:
        yield lo, lo + count
        lo += count


def dense_gradient(n=N):
    """(g, S, c): every float non-zero, S exact in any order (small integers),
    c / sqrt(S) = 0.5 exactly.  At n = sum(V): +-1 on 6,852 floats and +-2 on
    the other 14,671, S = 256^2, c = 128.  Elsewhere: +-2 everywhere when n is a
    power of four (S = 4 n), else ``exact_gradient``'s sparse one."""
    if n == N:
        g = np.full(n, 2.0, np.float32)
        g[np.random.default_rng(7).permutation(n)[:ONES]] = 1.0
        g[np.arange(n) % 3 == 0] *= np.float32(-1.0)
        S, c = 65_536.0, MAX_NORM
    elif 4 ** round(math.log(n, 4)) == n:
        g = np.where(np.arange(n) % 3 == 0, -2.0, 2.0).astype(np.float32)
        S = 4.0 * n
        c = math.sqrt(S) / 2.0
    else:
        g, S, c = C.exact_gradient(n)
    assert C.exact_sum_sq(g) == (S, 0) and float(np.float32(c)) == c and c / math.sqrt(S) == 0.5
    return g, S, c


def gradient(n, kind, i, variables):
    """Replica i's gradient of outcome ``kind`` for a call clipping at
    ``dense_gradient(n)``'s max_norm: "clipped" has scale exactly 0.5,
    "unclipped" a quarter of those values (S = c^2 / 4: scale 1), "skipped" the
    clipped one with a NaN and two infinities in it (as far as n has three
    places).  Non-zero in every variable, which is asserted here on the host."""
    g, S, c = dense_gradient(n)
    g = np.roll(g, 3 * i)
    if kind == "unclipped":
        g = g * np.float32(0.25)
    elif kind == "skipped":
        for p, v in zip(C.nonfinite_positions(n), (np.nan, np.inf, -np.inf)):
            g[p] = v
    else:
        assert kind == "clipped", kind
    g = np.ascontiguousarray(g, np.float32)
    for lo, hi in spans(variables):
        assert hi == lo or np.any(g[lo:hi] != 0), f"variable [{lo}, {hi}) of replica {i} has a zero gradient"
    S_k, K = C.exact_sum_sq(g)
    scale, flags = C.decide(S_k, K, c, True)
    want = {"unclipped": (1.0, 0), "clipped": (0.5, C.CLIPPED), "skipped": (float(scale), flags | C.SKIPPED)}[kind]
    assert (float(scale), flags) == want and (K > 0) == (kind == "skipped"), (kind, scale, flags, K)
    return g


def multipliers_show(variables, mults, momentum, wd, lr=0.05, n=None, kinds=("unclipped", "clipped")):
    """The host-only guard: for a stepping replica that is not skipped, the
    expected w with every multiplier forced to 1 (the clipped kernel's step)
    differs from the per-variable one somewhere in every variable whose
    multiplier is not 1, and nowhere in the others."""
    from oracle import oracle as O
    n = n or sum(variables)
    _, _, c = dense_gradient(n)
    for kind in kinds:
        g = gradient(n, kind, 1, variables)
        scale, flags = C.decide(*C.exact_sum_sq(g), c, True)
        out = []
        for m in (mults, (1.0,) * len(variables)):
            w = O.fill_normal(n, 11, 0.05)
            last = O.fill_normal(n, 12, 0.001) if momentum > 0 else None
            C.step([w, g.copy(), last, np.zeros(n, np.float32)], scale, flags, momentum, wd, lr=lr,
                   variables=variables, mults=m)
            out.append(w)
        for v, (lo, hi) in enumerate(spans(variables)):
            differs = not np.array_equal(out[0][lo:hi].view(np.uint32), out[1][lo:hi].view(np.uint32))
            assert differs == (mults[v] != 1.0 and hi > lo), (kind, momentum, wd, v, mults[v])
    assert any(m != 1.0 for m in mults)


__all__ = ["C", "M", "V", "N", "MAX_NORM", "KINDS", "spans", "dense_gradient", "gradient", "multipliers_show"]
