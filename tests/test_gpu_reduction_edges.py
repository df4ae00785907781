"""The two reductions and the CLIP step kernels on IEEE edge values (run with
-m gpu): ``gradient_norm_kernel`` / ``gradient_norm_reduce_kernel``
(clip_kernels.hip), the ``CLIP=1`` instantiations of ``sma_optimise_kernel``
and ``sma_optimise_variables_kernel``, and ``stats_pass_kernel`` /
``stats_reduce_kernel`` (stats_kernels.hip).  DESIGN.md section 4 has the
reductions' clause of the edge-value contract; tests/test_reduction_edges.py
pins every input on the CPU.

Every reference is exact (``E.exact_stats``: Python integers and Fractions).
In the exact regimes the device's doubles equal it; in the range-end regime
and over the wide catalogue they lie within the reordering bound of an fp64
sum, 2 m 2^-53 sum |term|.  The decision and the scale are compared, bits and
counters, with ``C.decide`` on exact integer sums, the hard cases included.
The step kernels are compared by the edge-value contract: ``assert_edge_equal``
on w, g, last, ``assert_bitexact`` on s against the old w and on the sentinels.

Shapes: ``E.N_RED`` = 9,095 floats and n = 8 for the decision tables.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_values as E
from tests import gradient_clip_common as C
from tests.helpers import Guarded, assert_bitexact

pytestmark = pytest.mark.gpu

N = E.N_RED
OPT_CONFIGS, WD = E.OPT_CONFIGS, E.WD
_gpu, _put, _get = C.context, C.put, C.get
KINDS = ("w", "g", "last", "s")
INPUTS = [r.name for r in E.REGIMES] + ["wide"]


def _dbits(x) -> int:
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _fbits(x) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).copy()).to("cuda:0")
    assert t.numel() == a.size and t.data_ptr() % 16 == 0  # exactly n floats: nothing behind them is the model's
    return t


# ---- 2. the norm reduction and the record ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _norm_input(name):
    """(g, the exact statistics of g, exact?)."""
    if name == "wide":
        g = O.fill_normal(N, 810, 0.01)
        E.apply({"x": g, "ref": np.zeros(N, np.float32)}, E.reduction_catalogue(), N)
        exact = False
    else:
        regime = next(r for r in E.REGIMES if r.name == name)
        g, exact = regime.make(N, 1), regime.exact
    g.setflags(write=False)
    return g, E.exact_stats(E.to_ints(g), E.bits(g)), exact


def _check_sum_sq(rec, want, exact, what):
    v = float(rec["sum_sq"])
    print(f"{what}: sum_sq {v!r} nonfinite {rec['nonfinite']}; want {float(want['sum_sq'])!r} {want['nonfinite']}")
    assert np.isfinite(v) and rec["nonfinite"] == want["nonfinite"], (what, rec)
    if exact:
        assert Fraction(v) == want["sum_sq"], (what, v, float(want["sum_sq"]))
    else:
        assert abs(Fraction(v) - want["sum_sq"]) <= 2 * want["m"] * E.EPS53 * want["sum_sq"], (what, v)


@pytest.mark.parametrize("name", INPUTS)
def test_norm_regimes_through_both_doors_and_both_load_policies(name):
    import torch

    from crossbow_amd.seam import SmaPlan
    g, want, exact = _norm_input(name)
    gt = _device(g)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    sums = []
    with SmaPlan([0], N) as plan:
        for slot, loads in ((0, 0), (1, 1), (1, -1)):
            rec, _, _ = plan.gradient_norm(0, slot, stream.cuda_stream, gt.data_ptr(), 0.0, True, loads)
            _check_sum_sq(rec, want, exact, f"{name}, seam, loads {loads}")
            assert rec["flags"] == (C.SKIPPED if want["nonfinite"] else 0) and _fbits(rec["scale"]) == E.b32(1.0)
            sums.append(_dbits(rec["sum_sq"]))
    assert_bitexact(gt.cpu().numpy(), g, "the reduction alone writes nothing")
    gpu = _gpu(N, 0.0, 0.0)
    try:
        gpu.set_gradient_clip(0.0, True)  # no clipping: a finite g is stepped as it is, another is skipped
        bufs = C.host(820, N, 0.0)
        bufs[1] = g.copy()
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        _check_sum_sq(rec, want, exact, f"{name}, context")
        sums.append(_dbits(rec["sum_sq"]))
    finally:
        gpu.free()
    assert len(set(sums)) == 1, [hex(s) for s in sums]


def _decision_rows():
    rows = [(label, cb, S) for label, cb, S in C.decision_table()]
    rows += [(f"hard case {k} ({dist:+d} ulp of the midpoint)", cb, S) for k, (cb, S, dist) in enumerate(C.HARD_CASES)]
    return rows


def _check_decision(rec, label, cb, S, prev, bad):
    scale, flags = C.decide(float(S), 0, C._f32(cb), False)
    want = (flags, _fbits(scale), _dbits(float(S)), 0, prev["steps"] + 1,
            prev["clipped_steps"] + (1 if flags & C.CLIPPED else 0), prev["skipped_steps"])
    got = (rec["flags"], _fbits(rec["scale"]), _dbits(rec["sum_sq"]), rec["nonfinite"], rec["steps"],
           rec["clipped_steps"], rec["skipped_steps"])
    if got != want:
        bad.append(f"{label} (c = {cb:#010x}, S = {S}): flags, scale bits, sum_sq bits, nonfinite, steps, clipped, "
                   f"skipped = {got}, want {want}")


def test_decision_and_scale_tables_on_one_plan_and_one_slot():
    import torch

    from crossbow_amd.seam import SmaPlan
    rows = _decision_rows()
    gt = _device(np.zeros(C.N_DECIDE, np.float32))
    stream = torch.cuda.Stream()
    bad = []
    with SmaPlan([0], C.N_DECIDE) as plan:
        prev = plan.clip_stats(0, 5, stream.cuda_stream)
        assert prev["steps"] == 0
        for label, cb, S in rows:
            gt.copy_(torch.from_numpy(C.gradient_of(S)))
            torch.cuda.synchronize()
            rec, _, _ = plan.gradient_norm(0, 5, stream.cuda_stream, gt.data_ptr(), C._f32(cb), False)
            _check_decision(rec, label, cb, S, prev, bad)
            prev = rec
    print(f"{len(rows)} pairs, {len(bad)} differ")
    assert not bad, "\n".join(bad)
    assert prev["steps"] == len(rows) and 0 < prev["clipped_steps"] < len(rows)


def test_decision_boundaries_and_hard_cases_through_the_context():
    from crossbow_amd import BUF_GRADIENT
    rows = _decision_rows()
    table = C.decision_table(random_pairs=0)
    # every boundary row, and the first three hard cases that a quotient 1 ulp low would move, and 1 ulp high
    hard = [r for r, (cb, S, _) in zip(rows[-len(C.HARD_CASES):], C.HARD_CASES)]
    moves = [C.nudge_moves(cb, S) for cb, S, _ in C.HARD_CASES]
    rows = rows[:len(table)] + [r for r, m in zip(hard, moves) if m[0]][:3] + [r for r, m in zip(hard, moves) if m[1]][:3]
    assert len(rows) == len(table) + 6 >= 12
    gpu = _gpu(C.N_DECIDE, 0.0, 0.0)
    bad = []
    try:
        prev = gpu.replica_clip_stats(0)
        for k, (label, cb, S) in enumerate(rows):
            # max_norm 0 alone would switch the feature off: the skip keeps it on, and K is 0
            gpu.set_gradient_clip(C._f32(cb), cb == 0)
            gpu.replica_write(0, BUF_GRADIENT, C.gradient_of(S))
            gpu.replica_optimise(0, task=k)
            gpu.wait()
            rec = gpu.replica_clip_stats(0)
            _check_decision(rec, label, cb, S, prev, bad)
            prev = rec
    finally:
        gpu.free()
    assert not bad, "\n".join(bad)


def _signs(n, seed):
    return np.where(np.random.default_rng(seed).integers(0, 2, n) == 1, np.float32(-1), np.float32(1))


SPECIAL = {
    # name: (n, g, bits of max_norm)
    "subnormal-max-norm": (C.N_DECIDE, lambda n: _signs(n, 1) * E.f32(E.MIN_SUB), E.MIN_SUB),
    "subnormal-scale": (N, lambda n: _signs(n, 2) * E.f32(E.FLT_MAX), E.b32(1.0)),
    "zero-scale": (N, lambda n: _signs(n, 3) * E.f32(E.FLT_MAX), E.FLT_MIN),
    "clipped-at-scale-one": (C.N_DECIDE, lambda n: C.gradient_of(4096 ** 2 + 1), E.b32(4096.0)),
}


def _special_scale(name, S):
    scale, flags = C.decide(S, 0, float(E.f32(SPECIAL[name][2])), False)
    assert flags == C.CLIPPED
    if name == "subnormal-max-norm":
        assert _fbits(scale) == E.b32(1.0 / np.sqrt(8.0))
    elif name == "subnormal-scale":
        assert E.is_subnormal(np.array([scale]))[0] and 2.5e-41 < float(scale) < 3.5e-41
    elif name == "zero-scale":
        assert _fbits(scale) == E.PZERO
    else:
        assert _fbits(scale) == E.b32(1.0)
    return scale, flags


@pytest.mark.parametrize("door", ["context", "seam"])
@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_scales_as_full_steps(name, door):
    import torch

    from crossbow_amd.seam import SmaPlan
    n, make, cb = SPECIAL[name]
    momentum, wd = 0.9, WD
    c = float(E.f32(cb))
    bufs = C.host(840, n, momentum)
    bufs[1] = np.ascontiguousarray(make(n), dtype=np.float32)
    before = [b.copy() for b in bufs]
    want = E.exact_stats(E.to_ints(bufs[1]), E.bits(bufs[1]))
    if door == "context":
        gpu = _gpu(n, momentum, wd)
        try:
            gpu.set_gradient_clip(c, False)
            _put(gpu, 0, bufs)
            gpu.replica_optimise(0, task=0)
            gpu.wait()
            rec = gpu.replica_clip_stats(0)
            got = _get(gpu, 0, momentum)
        finally:
            gpu.free()
    else:
        dev = [Guarded(b, 40 + k) for k, b in enumerate(bufs)]
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with SmaPlan([0], n) as plan:
            plan.optimise_clipped(0, 2, stream.cuda_stream, *[d.ptr for d in dev], C.LR, momentum, wd, c)
            rec = plan.clip_stats(0, 2, stream.cuda_stream)
        host = [d.t.cpu().numpy() for d in dev]
        for k, d in enumerate(dev):
            assert_bitexact(host[k][n:], d.sentinel, f"the floats behind {KINDS[k]}")
        got = [h[:n] for h in host]
    _check_sum_sq(rec, want, n == C.N_DECIDE, f"{name}, {door}")
    scale, flags = _special_scale(name, rec["sum_sq"])
    assert (rec["flags"], _fbits(rec["scale"])) == (flags, _fbits(scale)), rec
    assert (rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == (1, 1, 0), rec
    C.step(bufs, scale, flags, momentum, wd)
    for k, kind in enumerate(KINDS):
        E.assert_edge_equal(got[k], bufs[k], f"{name}, {door}: {kind}")
    assert_bitexact(got[3], before[0], "s is a copy of the old w")
    if name == "clipped-at-scale-one":  # bit for bit the plain step, while the record counts a clipped one
        plain = [b.copy() for b in before]
        O.sma_optimise(np.float32(-C.LR), momentum, wd, *plain)
        for k, kind in enumerate(KINDS):
            assert_bitexact(got[k], plain[k], f"{kind} equals the plain step's")


@pytest.mark.parametrize("skip", [False, True], ids=["no-skip", "skip"])
def test_zero_scale_writes_signed_zeros_back_and_an_all_nonfinite_gradient(skip):
    """Without momentum and weight decay the g written back is scale * g itself."""
    import torch

    from crossbow_amd.seam import SmaPlan
    stream = torch.cuda.Stream()
    # scale 0: g comes back as +-0 with the sign of g
    bufs = C.host(850, N, 0.0)
    bufs[1] = np.ascontiguousarray(_signs(N, 3) * E.f32(E.FLT_MAX))
    g0 = bufs[1].copy()
    dev = [Guarded(b, 50 + k) if b is not None else None for k, b in enumerate(bufs)]
    # every g non-finite: S = +0, K = n
    every = C.host(860, N, 0.0)
    pats = np.array([E.PINF, E.NINF, E.QNAN, E.PAYLOAD_NAN, E.SNAN], np.uint32)
    every[1] = pats[np.arange(N) % 5].view(np.float32).copy()
    before = [b.copy() if b is not None else None for b in every]
    dev2 = [Guarded(b, 60 + k) if b is not None else None for k, b in enumerate(every)]
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        plan.optimise_clipped(0, 0, stream.cuda_stream, dev[0].ptr, dev[1].ptr, None, dev[3].ptr, C.LR, 0.0, 0.0,
                              float(E.f32(E.FLT_MIN)), skip_nonfinite=skip)
        rec = plan.clip_stats(0, 0, stream.cuda_stream)
        plan.optimise_clipped(0, 1, stream.cuda_stream, dev2[0].ptr, dev2[1].ptr, None, dev2[3].ptr, C.LR, 0.0, 0.0,
                              0.5, skip_nonfinite=skip)
        rec2 = plan.clip_stats(0, 1, stream.cuda_stream)
    assert (rec["flags"], _fbits(rec["scale"]), rec["nonfinite"]) == (C.CLIPPED, E.PZERO, 0), rec
    got_g = dev[1].t.cpu().numpy()[:N]
    assert np.array_equal(E.bits(got_g), E.bits(g0) & np.uint32(E.SIGN)), "g = +-0 with the sign of the old g"
    assert_bitexact(dev[0].t.cpu().numpy()[:N], bufs[0], "w + rate * (+-0) is w")
    assert (_dbits(rec2["sum_sq"]), rec2["nonfinite"], _fbits(rec2["scale"])) == (0, N, E.b32(1.0)), rec2
    assert rec2["flags"] == (C.SKIPPED if skip else 0) and rec2["skipped_steps"] == int(skip)
    C.step(every, np.float32(1.0), rec2["flags"], 0.0, 0.0)
    for k, kind in enumerate(KINDS):
        if every[k] is None:
            continue
        host = dev2[k].t.cpu().numpy()
        assert_bitexact(host[N:], dev2[k].sentinel, f"the floats behind {kind}")
        if skip or kind == "s":
            assert_bitexact(host[:N], before[0] if kind == "s" else before[k], f"all non-finite, skipped: {kind}")
        else:
            E.assert_edge_equal(host[:N], every[k], f"all non-finite, stepped: {kind}")


# ---- 3. the CLIP=1 step kernels ---------------------------------------------------------------
def _check_record(rec, S, K, c, skip, what):
    print(f"{what}: sum_sq {rec['sum_sq']!r} (exact {S!r}) nonfinite {rec['nonfinite']} scale {rec['scale']!r} "
          f"flags {rec['flags']}")
    assert rec["nonfinite"] == K, (what, rec)
    assert abs(rec["sum_sq"] - S) <= 2 * N * 2.0 ** -53 * S, (what, rec["sum_sq"], S)
    scale, flags = C.decide(rec["sum_sq"], K, c, skip)
    assert (rec["flags"], _fbits(rec["scale"])) == (flags, _fbits(scale)), (what, rec, scale, flags)
    assert flags & C.CLIPPED and bool(flags & C.SKIPPED) == (skip and K > 0), (what, flags)


def _check_step(read, a, want, labels, flags, what):
    """`read(name)`: the device's w, g, last or s; a the inputs, want the oracle's outputs."""
    assert np.any(E.bits(a["w"]) == E.SNAN) and np.any(E.bits(a["w"]) == E.PAYLOAD_NAN)
    assert_bitexact(read("s"), a["w"], f"{what}s is a copy of the old w, signalling NaNs included")
    for name in ("w", "g", "last"):
        if a[name] is None:
            continue
        if flags & C.SKIPPED:
            assert_bitexact(read(name), a[name], f"{what}{name} is not written by a skipped step")
        else:
            E.assert_edge_equal(read(name), want[name], f"{what}{name}", labels)


def _context_step(momentum, wd, finite, skip, config=None, variables=None, mults=None, barrier=False):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_LAST
    a, labels, S, K, c = C.clipped_inputs(momentum, wd, finite)
    R, alpha = 2, E.ALPHA
    gpu = _gpu(N, momentum, wd, replicas=R, variables=list(variables) if variables else None, mults=mults, alpha=alpha)
    try:
        if config:
            gpu.set_kernel_config(**config)
        if variables:
            gpu.set_variable_learning_rates(True)
        st = O.make_state(N, 1, R, alpha, momentum)
        if barrier:
            from tests.helpers import upload
            upload(gpu, st)
        gpu.set_gradient_clip(c, skip)
        _put(gpu, 0, [a[k] for k in KINDS])
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        what = f"context, {'finite g' if finite else 'as is'}{', skip' if skip else ''}: "
        _check_record(rec, S, K, c, skip, what)
        want, _, flags = C.clipped_expectation(a, rec["sum_sq"], K, c, skip, momentum, wd, variables, mults)
        got = dict(zip(KINDS, _get(gpu, 0, momentum)))
        _check_step(lambda name: got[name], a, want, labels, flags, what)
        assert (rec["steps"], rec["skipped_steps"]) == (1, 1 if flags & C.SKIPPED else 0)
        if barrier:  # the next barrier sees "no local movement" on replica 0, NaNs and all
            assert flags & C.SKIPPED
            st.w[0][:], st.s[0][:] = a["w"], a["w"]
            gpu.lockAny()
            gpu.synchronise(0, 1, 0, False)
            gpu.unlockAny()
            gpu.wait()
            O.sma_step(st)
            E.assert_edge_equal(gpu.base_read(0, BUF_DATA), st.z[0], "z after the barrier", labels)
            if momentum > 0:
                E.assert_edge_equal(gpu.base_read(0, BUF_LAST), st.last[0], "base last after the barrier", labels)
            for i in range(R):
                E.assert_edge_equal(gpu.replica_read(i, BUF_DATA), st.w[i], f"w[{i}] after the barrier", labels)
            assert_bitexact(gpu.replica_read(0, BUF_DIFF), a["w"], "s[0] is not written by the barrier")
    finally:
        gpu.free()


def _seam_step(momentum, wd, finite, skip, variables=None, mults=None):
    import torch

    from crossbow_amd.seam import SmaPlan
    a, labels, S, K, c = C.clipped_inputs(momentum, wd, finite)
    dev = {k: Guarded(a[k], 70 + j) for j, k in enumerate(KINDS) if a[k] is not None}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        if variables:
            plan.set_variables(variables, mults)
        plan.optimise_clipped(0, 9, stream.cuda_stream, dev["w"].ptr, dev["g"].ptr,
                              dev["last"].ptr if momentum > 0 else None, dev["s"].ptr, C.LR, momentum, wd, c,
                              skip_nonfinite=skip, use_variables=bool(variables))
        rec = plan.clip_stats(0, 9, stream.cuda_stream)
    what = f"seam, {'finite g' if finite else 'as is'}{', skip' if skip else ''}: "
    _check_record(rec, S, K, c, skip, what)
    want, _, flags = C.clipped_expectation(a, rec["sum_sq"], K, c, skip, momentum, wd, variables, mults)
    host = {k: gd.t.cpu().numpy() for k, gd in dev.items()}
    _check_step(lambda name: host[name][:N], a, want, labels, flags, what)
    for k, gd in dev.items():
        assert_bitexact(host[k][N:], gd.sentinel, f"the floats behind {k}")


FORMS = pytest.mark.parametrize("finite,skip", [(False, False), (True, False), (False, True), (True, True)],
                                ids=["as-is", "finite-g", "as-is-skipped", "finite-g-not-skipped"])


@FORMS
@pytest.mark.parametrize("config", list(OPT_CONFIGS))
def test_clipped_step_context(config, finite, skip):
    _context_step(*OPT_CONFIGS[config], finite, skip)


@FORMS
@pytest.mark.parametrize("config", list(OPT_CONFIGS))
def test_clipped_step_seam(config, finite, skip):
    _seam_step(*OPT_CONFIGS[config], finite, skip)


@pytest.mark.parametrize("finite", [False, True], ids=["as-is", "finite-g"])
def test_clipped_step_context_plain_loads_no_unroll(finite):
    _context_step(0.9, WD, finite, False, config=dict(policy=0, unroll=1))


def test_skipped_step_then_the_barrier_matches_the_oracle():
    _context_step(0.9, WD, False, True, barrier=True)


# the middle variable holds the whole first copy of the scenarios and starts and ends off a float4
VARS = (3, 1500, N - 1503)
MULTS = (1.0, 0.5, 2.0)


@pytest.mark.parametrize("door", ["context", "seam"])
@FORMS
@pytest.mark.parametrize("config", list(OPT_CONFIGS))
def test_clipped_per_variable_step(config, finite, skip, door):
    L = len(E.optimiser_scenarios(-E.LR, *OPT_CONFIGS[config]))
    first, _ = E.layout(L, N)
    assert VARS[0] < first and first + L <= VARS[0] + VARS[1]
    (_context_step if door == "context" else _seam_step)(*OPT_CONFIGS[config], finite, skip, variables=VARS,
                                                         mults=MULTS)


# ---- 4. the model statistics --------------------------------------------------------------------
CATALOGUE = E.reduction_catalogue()
STATS_VARS, FIRST, SECOND = E.stats_variables(len(CATALOGUE))
WHERE = ("z", "one-replica", "all-replicas", "s")


def _zeros(i):
    return np.full(N, -0.0 if i % 2 else 0.0, np.float32)


@functools.lru_cache(maxsize=None)
def _stats_case(name, where, R):
    """(z, the R compared buffers): the regime, or ordinary data with the wide
    catalogue written in twice, in z, in replica 1, or in z and every replica."""
    if name == "wide":
        rng = np.random.default_rng(77)
        z = (0.05 * rng.standard_normal(N)).astype(np.float32)
        x = [(z + 0.01 * rng.standard_normal(N)).astype(np.float32) for _ in range(R)]
        spare = np.zeros(N, np.float32)
        if where == "z":
            E.apply_at({"x": z, "ref": spare}, CATALOGUE, (FIRST, SECOND))
        else:
            for i in ([1] if where == "one-replica" else range(R)):
                E.apply_at({"x": x[i], "ref": z}, CATALOGUE, (FIRST, SECOND))
    else:
        regime = next(r for r in E.REGIMES if r.name == name)
        if where == "z":
            z, x = regime.make(N, 0), [_zeros(i) for i in range(R)]
        elif where == "one-replica":
            z, x = _zeros(1), [regime.make(N, 1) if i == 1 else _zeros(i) for i in range(R)]
        else:
            z, x = regime.make(N, 0), [regime.make(N, 1 + i) for i in range(R)]
    for a in [z] + x:
        a.setflags(write=False)
    return z, tuple(x)


def _check_stats(out, z, x, exact, what):
    """Every whole-model and per-variable record against exact arithmetic."""
    base, reps, bv, rv = out
    assert bv.shape[-1] == len(STATS_VARS) and rv.shape == (len(x), len(STATS_VARS))
    zi, zb = E.to_ints(z), E.bits(z)
    cuts = np.concatenate([[0], np.cumsum(STATS_VARS)]).tolist()
    E.assert_stats_record(base, E.exact_stats(zi, zb), exact, f"{what}: z")
    for v in range(len(STATS_VARS)):
        lo, hi = cuts[v], cuts[v + 1]
        E.assert_stats_record(bv[v], E.exact_stats(zi[lo:hi], zb[lo:hi]), exact, f"{what}: z variable {v}")
    for i, a in enumerate(x):
        ai, ab = E.to_ints(a), E.bits(a)
        E.assert_stats_record(reps[i], E.exact_stats(ai, ab, zi), exact, f"{what}: buffer {i}")
        for v in range(len(STATS_VARS)):
            lo, hi = cuts[v], cuts[v + 1]
            E.assert_stats_record(rv[i, v], E.exact_stats(ai[lo:hi], ab[lo:hi], zi[lo:hi]), exact,
                                  f"{what}: buffer {i} variable {v} [{lo}, {hi})")


@pytest.mark.parametrize("R", [8, 9], ids=["unrolled-8", "chunked-9"])
@pytest.mark.parametrize("name", INPUTS)
def test_statistics_regimes_context_and_seam(name, R):
    import torch

    from crossbow_amd import BUF_DATA, BUF_DIFF
    from crossbow_amd.seam import SmaPlan
    from tests.test_gpu_stats import make_ctx, put
    exact = name != "wide" and next(r for r in E.REGIMES if r.name == name).exact
    other = [np.full(N, np.float32(3 + i)) for i in range(R)]
    stream = torch.cuda.Stream()
    with make_ctx(STATS_VARS, R) as g, SmaPlan([0], N) as plan:
        for where in WHERE:
            z, x = _stats_case(name, "all-replicas" if where == "s" else where, R)
            if where == "s":
                put(g, z, other, list(x))
            else:
                put(g, z, list(x), other)
            out = g.modelStats(BUF_DIFF if where == "s" else BUF_DATA, per_variable=True)
            what = f"{name} in {where}, R = {R}"
            _check_stats((out[0][0], out[1], out[2][0], out[3]), z, x, exact, what)
            # the seam over unpadded buffers: the same piece table and tree, the same bytes
            zt, xt = _device(z), [_device(a) for a in x]
            torch.cuda.synchronize()
            r, o, rv, ov = plan.buffer_stats(0, stream.cuda_stream, zt.data_ptr(), [t.data_ptr() for t in xt],
                                             var_elements=STATS_VARS, per_variable=True)
            assert r.tobytes() == out[0][0].tobytes() and o.tobytes() == out[1].tobytes(), what
            assert rv.tobytes() == out[2][0].tobytes() and ov.tobytes() == out[3].tobytes(), what


def test_max_abs_of_a_subnormal_a_minus_zero_and_an_all_nan_variable():
    """The wide catalogue's last groups and the subnormal regime, spelled out."""
    from tests.test_gpu_stats import make_ctx, put
    R = 8
    z, x = _stats_case("wide", "one-replica", R)
    L = len(CATALOGUE)
    v_nan, v_neg0 = 2 + (L - 6) // 3, 2 + (L - 3) // 3
    with make_ctx(STATS_VARS, R) as g:
        put(g, z, list(x))
        _, _, _, rv = g.modelStats(per_variable=True)
        for v, nf in ((v_nan, 3), (v_neg0, 0)):
            rec = rv[1, v]
            assert (_fbits(rec["max_abs"]), int(rec["nonfinite"])) == (E.PZERO, nf), (v, rec)
            assert (_dbits(rec["sum"]), _dbits(rec["sum_sq"])) == (0, 0), (v, rec)  # +0, from -0 terms too
        assert _dbits(rv[1, v_nan]["dist_sq"]) == 0
        zs, xs = _stats_case("subnormal", "all-replicas", R)
        put(g, zs, list(xs))
        base, reps = g.modelStats()
        assert _fbits(base[0]["max_abs"]) == E.K_MAX and all(_fbits(r["max_abs"]) == E.K_MAX for r in reps)


def test_checkpoint_guard_on_edge_values(tmp_path):
    import os

    from crossbow_amd import BUF_DATA, CbxError, _lib
    from tests.test_gpu_stats import make_ctx, put
    R = 2
    sub = next(r for r in E.REGIMES if r.name == "subnormal")
    end = next(r for r in E.REGIMES if r.name == "range-end")
    z, w = sub.make(N, 0), [end.make(N, 1), sub.make(N, 2)]
    w[1][FIRST:FIRST + 4] = E.f32(E.FLT_MAX)
    w[1][SECOND:SECOND + 4] = -E.f32(E.FLT_MAX)
    d = str(tmp_path)
    with make_ctx(STATS_VARS, R) as g:
        g.setCheckpointGuard(True)
        for spot, pattern in ((SECOND + 1, E.SNAN), (FIRST + 2, E.NINF)):
            bad = w[1].copy()
            bad.view(np.uint32)[spot] = pattern
            put(g, z, [w[0], bad])
            with pytest.raises(CbxError) as e:
                g.checkpointModel(d)
            assert e.value.code == _lib.CBX_ERR_STATE and "replica 1" in str(e.value), e.value
            assert os.listdir(d) == []
        # subnormals and both ends of the range are finite: the model is accepted
        g.replica_write(1, BUF_DATA, w[1])
        g.checkpointModel(d)
        assert os.listdir(d) == ["000001"]
        got = np.fromfile(os.path.join(d, "000001", "gpu-00-replica-001-data.dat"), np.float32)
        assert_bitexact(got, w[1], "the checkpointed replica")
