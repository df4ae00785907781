"""Pins the inputs of the reductions' edge-value tests on the CPU
(tests/test_gpu_reduction_edges.py; DESIGN.md, the reductions' clause of the
edge-value contract), before any kernel sees them.  Every reference here is
exact: Python integers, ``fractions.Fraction`` or ``math.fsum`` of exact
products; never a device value, never a plain ``np.sum``.

* the exact regimes are exact: with integers, n max k^2 and n max (k - k_ref)^2
  stay below 2^53, and every expected sum is a double;
* the regimes separate fp64 from fp32 arithmetic: a product rounded to fp32, a
  difference taken in fp32 and a flushed input each change the expected value
  by more than the test allows;
* the wide catalogue lies twice in the statistics tests' variable list, once
  in aligned pieces and once in non-aligned ones (the piece-table rule of
  stats_plan.h restated);
* the decision table's gradients yield their S exactly, and ``C.decide``
  equals exact arithmetic on the decision and the header's sequence on the
  scale; every listed hard case lies within 1 double ulp of a float midpoint;
* the clipped-step inputs bite: special values of every kind in the expected
  outputs, NaNs under a quarter, a flushed device seen in w and g.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest

from tests import edge_values as E
from tests import gradient_clip_common as C

N = E.N_RED
CONFIGS = E.OPT_CONFIGS
EXACT = [r for r in E.REGIMES if r.exact]
RANGE_END = [r for r in E.REGIMES if not r.exact]


def _is_double(f: Fraction) -> bool:
    return Fraction(float(f)) == f


def test_shape_of_the_reductions():
    assert N == 9095 and N % 4 == 3
    assert N // 4096 == 2 and (N % 4096) // 4 == 225 and N % 1024 == 903 == E.TAIL
    first, second = E.layout(len(E.reduction_catalogue()), N)
    assert second + len(E.reduction_catalogue()) == N and first < 4096 < 2 * 4096 < second


@pytest.mark.parametrize("regime", EXACT, ids=repr)
def test_exact_regimes_are_exact_in_fp64_in_any_order(regime):
    x, ref = regime.make(N, 1), regime.make(N, 2)
    assert not np.array_equal(x, ref)
    kx, kr = E.to_ints(x), E.to_ints(ref)
    unit = math.gcd(*[abs(k) for k in kx + kr])  # the regime's common power of two
    assert unit & (unit - 1) == 0
    ix, ir = [k // unit for k in kx], [k // unit for k in kr]
    assert max(abs(k) for k in ix + ir) <= E.K_MAX
    # every partial sum, in any order, is an integer below 2^53 times one power of two
    assert N * max(abs(k) for k in ix) < 2 ** 53
    assert N * max(k * k for k in ix) < 2 ** 53
    assert N * max((a - b) ** 2 for a, b in zip(ix, ir)) < 2 ** 53
    want = E.exact_stats(kx, E.bits(x), kr)
    u = Fraction(unit) * E.ULP
    assert want["sum"] == sum(ix) * u and want["sum_sq"] == sum(k * k for k in ix) * u * u
    assert want["dist_sq"] == sum((a - b) ** 2 for a, b in zip(ix, ir)) * u * u
    assert all(_is_double(want[f]) for f in ("sum", "sum_sq", "dist_sq")) and want["dist_sq"] > 0
    assert want["nonfinite"] == 0
    assert want["max_abs"] == int(E.bits(np.abs(x)).max())
    if regime.name in ("subnormal", "min-sub"):
        assert np.all(E.is_subnormal(x)) and 0 < want["max_abs"] <= E.MAX_SUB  # the maximum is a subnormal's bits


def test_the_regimes_separate_fp64_from_fp32_arithmetic():
    with np.errstate(all="ignore"):
        for regime in E.REGIMES:
            x, ref = regime.make(N, 1), regime.make(N, 2)
            want = E.exact_stats(E.to_ints(x), E.bits(x), E.to_ints(ref))
            bound = 0 if regime.exact else 2 * N * E.EPS53 * want["sum_sq"]
            # the product rounded to fp32 before it is widened
            q32 = math.fsum((x * x).astype(np.float64).tolist())
            d32 = x - ref  # the difference taken in fp32
            dd = math.fsum((d32.astype(np.float64) ** 2).tolist())
            if regime.name in ("subnormal", "min-sub", "FLT_MIN"):
                assert q32 == 0.0 and want["sum_sq"] > 0, regime  # every square underflows in fp32
            elif regime.name in ("mid-range", "2^127", "range-end"):
                assert q32 == math.inf, regime                    # every square overflows in fp32
            if regime.name in ("2^127", "range-end"):
                assert not np.isfinite(dd), regime                 # x - ref overflows in fp32
            assert not np.isfinite(q32) or abs(Fraction(q32) - want["sum_sq"]) > bound, regime
            # a flushed subnormal input
            if regime.name in ("subnormal", "min-sub"):
                y = x.copy()
                E.flush(y)
                assert not y.any() and want["sum"] != 0 and want["sum_sq"] != 0


@pytest.mark.parametrize("regime", RANGE_END, ids=repr)
def test_range_end_regime(regime):
    x, ref = regime.make(N, 1), regime.make(N, 2)
    mag = np.abs(x).astype(np.float64)
    assert mag.min() >= 2.0 ** 126 and E.bits(np.abs(x)).max() == E.FLT_MAX and np.all(np.isfinite(x))
    assert 0.3 < np.mean(x < 0) < 0.7
    x64, r64 = x.astype(np.float64), ref.astype(np.float64)
    want = E.exact_stats(E.to_ints(x), E.bits(x), E.to_ints(ref))
    # math.fsum of the exact terms is the correctly rounded exact sum
    assert math.fsum(x64.tolist()) == float(want["sum"])
    assert math.fsum((x64 * x64).tolist()) == float(want["sum_sq"])
    assert math.fsum(((x64 - r64) ** 2).tolist()) == float(want["dist_sq"])
    # every term has the same scale: the reordering bound has teeth (about 2 n 2^-53, relatively)
    assert 2 * N * E.EPS53 * want["sum_sq"] < want["sum_sq"] / 2 ** 38
    # the same sums in fp32 leave the range
    with np.errstate(all="ignore"):
        one = np.float32(1)
        assert np.cumsum(x * x, dtype=np.float32)[-1] == np.inf
        assert np.cumsum((x - ref) * (x - ref), dtype=np.float32)[-1] == np.inf
        assert not np.isfinite(np.cumsum(x * one, dtype=np.float32)[-1])


def test_wide_catalogue_and_the_statistics_variable_list():
    scen = E.reduction_catalogue()
    L = len(scen)
    labels = [s[0] for s in scen]
    for needle in ("x=+min-sub", "x=snan", "ref=payload-nan", "ref=-inf", "zeros +-", "x=+inf beside a finite ref",
                   "x finite beside ref=+inf", "x=snan beside a finite ref", "x finite beside ref=payload-nan",
                   "x=+min-sub ref=-min-sub", "x == ref", "x=+FLT_MAX ref=-FLT_MAX"):
        assert needle in labels, needle
    variables, first, second = E.stats_variables(L)
    assert sum(variables) == N and variables[0] == 1 and variables.count(3) == -(-L // 3)
    assert variables.index(3) == 2 and variables[-1] > 3  # the scalar run is not at the buffer's end
    pieces = E.stats_pieces(variables)
    assert pieces[0] == (0, 1, 0, False) and [p[:2] for p in pieces] == sorted(p[:2] for p in pieces)
    assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and pieces[-1][1] == N
    aligned = np.zeros(N, bool)
    for lo, hi, _, al in pieces:
        assert not al or (lo % 4 == 0 and hi % 4 == 0)
        assert al or hi - lo <= 3
        aligned[lo:hi] = al
    assert aligned[first:first + L].all(), "the first copy lies in aligned pieces"
    assert not aligned[second:second + L].any(), "the second copy lies in non-aligned pieces"
    assert (second - first) % 4 != 0
    # written twice, and a group of three never mixes the huge values with a mask pair
    x, ref = np.ones(N, np.float32), np.ones(N, np.float32)
    lab = E.apply_at({"x": x, "ref": ref}, scen, (first, second))
    assert lab[first:first + L] == lab[second:second + L] == labels
    assert sum(v is not None for v in lab) == 2 * L
    lo = second
    for v in range(2, 2 + L // 3):
        group = labels[lo - second:lo - second + 3]
        if any("beside" in g for g in group):
            assert np.all(~np.isfinite(x[lo:lo + 3]) | (np.abs(x[lo:lo + 3]) <= 1)), group
        lo += 3
    allnan = [k for k in range(0, L, 3) if np.isnan(x[second + k:second + k + 3]).all()]
    allneg0 = [k for k in range(0, L, 3) if np.all(E.bits(x[second + k:second + k + 3]) == E.NZERO)]
    assert allnan and allneg0, "a variable of NaNs only and one of -0 only: max_abs is +0"


# ---- the decision and the scale --------------------------------------------------------------
def _exact_decision(cb, S):
    c = Fraction(C._f32(cb))
    return c > 0 and S > c * c


def test_decision_table():
    rows = C.decision_table()
    assert len(rows) >= 256 + 8
    seen = set()
    for label, cb, S in rows:
        g = C.gradient_of(S)
        assert g.size == C.N_DECIDE == 8 and S < 2 ** 46
        assert all(abs(int(v)) < 2 ** 23 and float(int(v)) == float(v) for v in g)
        assert sum(int(v) ** 2 for v in g) == S and C.exact_sum_sq(g) == (float(S), 0)
        scale, flags = C.decide(float(S), 0, C._f32(cb), False)
        clipped = _exact_decision(cb, S)
        assert flags == (C.CLIPPED if clipped else 0), label
        if clipped:
            assert E.bits(np.array([scale]))[0] == C.scale_bits(cb, S), label
            assert float(scale) <= 1.0
        else:
            assert E.bits(np.array([scale]))[0] == E.b32(1.0), label
        seen.add((clipped, float(scale) == 1.0))
    assert seen == {(False, True), (True, True), (True, False)}
    by = {label: (cb, S) for label, cb, S in rows}
    cb, S = by["S == c^2: not clipped, scale 1"]
    assert Fraction(C._f32(cb)) ** 2 == S
    cb, S = by["S = c^2 + 1: clipped, the scale rounds to 1.0f"]
    assert C._f32(cb) == 4096.0 and S == 4096 ** 2 + 1 and C.scale_bits(cb, S) == E.b32(1.0)
    cb, S = by["c one float below sqrt(S)"]
    up = Fraction(float(np.nextafter(np.float32(C._f32(cb)), np.float32(np.inf))))
    assert Fraction(C._f32(cb)) ** 2 < S < up ** 2
    g0 = C.gradient_of(0)
    assert not g0.any() and {int(b) for b in E.bits(g0)} == {E.PZERO, E.NZERO}
    assert C.decide(0.0, 0, 4096.0, False) == (np.float32(1.0), 0)
    random = [r for r in rows if r[0].startswith("random pair")]
    assert len(random) >= 256
    share = np.mean([_exact_decision(cb, S) for _, cb, S in random])
    assert 0.25 < share < 0.75, share


def _sqrt_is_correctly_rounded(S):
    r = Fraction(math.sqrt(S))
    half = Fraction(math.ulp(math.sqrt(S))) / 2
    return (r - half) ** 2 <= S <= (r + half) ** 2


def test_hard_cases_lie_within_one_double_ulp_of_a_float_midpoint():
    assert len(C.HARD_CASES) >= 24 and len(set(C.HARD_CASES)) == len(C.HARD_CASES)
    ties = down = up = 0
    for cb, S, dist in C.HARD_CASES:
        c = C._f32(cb)
        assert 2.0 ** 13 <= c < 2.0 ** 14 and c * 1024 == int(c * 1024)
        assert 2 ** 20 <= S < 2 ** 44 and len(C.squares(S)) <= C.N_DECIDE
        assert _exact_decision(cb, S), "clipped: the scale is computed"
        assert _sqrt_is_correctly_rounded(S)
        q = c / math.sqrt(S)  # the header's sequence in IEEE double
        f = float(np.float32(q))
        other = float(np.nextafter(np.float32(f), np.float32(np.inf if q > f else -np.inf)))
        if q == f:
            raise AssertionError("a float itself is no hard case")
        mid = (Fraction(f) + Fraction(other)) / 2
        off = (Fraction(q) - mid) / Fraction(math.ulp(q))
        assert off == dist and abs(off) <= 1, (hex(cb), S, off)
        assert C.midpoint_distance(cb, S) == dist
        ties += dist == 0
        scale, flags = C.decide(float(S), 0, c, False)
        assert flags == C.CLIPPED and E.bits(np.array([scale]))[0] == C.scale_bits(cb, S)
        # a quotient one ulp off: a tie moves for exactly one direction, a neighbour of a tie when
        # the nudge lands on the tie and ties-to-even goes the other way
        moved = C.nudge_moves(cb, S)
        assert sum(moved) == 1 if dist == 0 else sum(moved) <= 1, (hex(cb), S)
        down, up = down + moved[0], up + moved[1]
    assert ties >= 4 and down >= 8 and up >= 8, (ties, down, up)


# ---- the clipped-step inputs --------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("finite", [False, True], ids=["as-is", "finite-g"])
def test_clipped_step_inputs_bite(config, finite):
    momentum, wd = CONFIGS[config]
    a, labels, S, K, c = C.clipped_inputs(momentum, wd, finite)
    assert a["g"].size == N and (K > 0) != finite
    if finite:
        assert np.all(np.isfinite(a["g"])) and np.isnan(a["w"]).any()
        assert momentum == 0 or np.isnan(a["last"]).any()
    else:
        assert np.isnan(a["g"]).any() and np.isinf(a["g"]).any()
    assert any(np.any(E.bits(a["w"]) == p) for p in (E.SNAN,)) and np.any(E.bits(a["w"]) == E.PAYLOAD_NAN)
    want, scale, flags = C.clipped_expectation(a, S, K, c, False, momentum, wd)
    assert flags == C.CLIPPED and 0.19 < float(scale) < 0.21
    outs = [want[k] for k in ("w", "g", "last") if want[k] is not None]
    census = E.census(outs)
    assert all(v > 0 for v in census.values()), census
    assert max(E.nan_fraction(o) for o in outs + [want["s"]]) <= 0.25
    # skipped: s = w and nothing else
    skipped, _, f2 = C.clipped_expectation(a, S, K, c, True, momentum, wd)
    assert bool(f2 & C.SKIPPED) == (not finite)
    if not finite:
        assert np.array_equal(E.bits(skipped["s"]), E.bits(a["w"]))
        assert all(np.array_equal(E.bits(skipped[k]), E.bits(a[k])) for k in ("w", "g", "last") if a[k] is not None)
    # a device that flushes subnormals, inputs and outputs, is seen in w and in g
    b = {k: (v.copy() if v is not None else None) for k, v in a.items()}
    for v in b.values():
        if v is not None:
            E.flush(v)
    got, _, _ = C.clipped_expectation(b, S, K, c, False, momentum, wd)
    for k in ("w", "g"):
        E.flush(got[k])
        assert E.edge_mismatches(got[k], want[k]).size > 0, f"{config}: a flushed device goes unseen in {k}"
