"""Per-variable model statistics and replica divergence reduced on the device
(cbx_model_stats, cbx_sma_plan_buffer_stats, the checkpoint guard;
crossbow_amd/csrc/stats_kernels.hip).

The reference is numpy in float64 over the same float32 inputs, masked as
``cbx_buffer_stats`` defines: a non-finite x only counts; a finite x beside a
non-finite reference adds to everything but ``dist_sq``.

Shapes: a tile of the piece table is 4096 floats and a one-wave workgroup
walks 3 pieces, so n = 64 * 4096 + 5 gives 66 pieces (64 tiles, one float4,
one float) over 22 workgroups of exactly three trips each; n = 1 and 4097 are
the one-float and tile-plus-one edges; the ragged list (1, 3, 35, 4093, 4096,
1000) puts variable boundaries at 1, 4, 39, 4132 and 8228, of which 1, 39 and
4132 fall inside a float4.  R = 8 takes the unrolled kernel, 1 and 9 the
chunked one (9 crosses kChunk).
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

RAGGED = (1, 3, 35, 4093, 4096, 1000)
N_RAGGED = sum(RAGGED)  # 9228
N_TRIPS = 64 * 4096 + 5
EPS = 2.0 ** -53
FIELDS = ("sum", "sum_sq", "dist_sq", "nonfinite", "max_abs", "reserved")


def make_ctx(variables, R, momentum=0.9):
    from crossbow_amd import SYNC_BSP, UPDATE_SMA, TheGPU
    n = sum(variables)
    g = TheGPU()
    g.init([0])
    g.setModel(len(variables), 4 * n)
    for op, v in enumerate(variables):
        g.setModelVariable(op, 1, [v], 4 * v)
    g.setUpdateModelType(UPDATE_SMA)
    g.setEamsgdAlpha(0.1)
    g.setMomentum(momentum, 0)
    g.setModelManager(R, SYNC_BSP)
    return g


def put(g, z, w, s=None):
    from crossbow_amd import BUF_DATA, BUF_DIFF
    g.base_write(0, BUF_DATA, z)
    for i, wi in enumerate(w):
        g.replica_write(i, BUF_DATA, wi)
    for i, si in enumerate(s or []):
        g.replica_write(i, BUF_DIFF, si)


def want(x, ref):
    """(sum, sum_sq, dist_sq, nonfinite, max_abs, sum of |x|) of float32 x against ref (None: x is the reference)."""
    fin = np.isfinite(x)
    x64 = np.where(fin, x, np.float32(0)).astype(np.float64)
    dist = 0.0
    if ref is not None:
        both = fin & np.isfinite(ref)
        d = np.where(both, x64 - np.where(both, ref, np.float32(0)).astype(np.float64), 0.0)
        dist = float(np.sum(d * d))
    mx = np.float32(np.max(np.abs(x[fin]))) if fin.any() else np.float32(0)
    return float(np.sum(x64)), float(np.sum(x64 * x64)), dist, int(np.count_nonzero(~fin)), mx, float(np.sum(np.abs(x64)))


def check(rec, x, ref, exact, what):
    s, q, d, nf, mx, sabs = want(x, ref)
    m = x.size
    print(f"{what}: got sum={rec['sum']!r} sum_sq={rec['sum_sq']!r} dist_sq={rec['dist_sq']!r} "
          f"nonfinite={rec['nonfinite']} max_abs={rec['max_abs']!r}; want {s!r} {q!r} {d!r} {nf} {mx!r}")
    assert int(rec["nonfinite"]) == nf, what
    assert np.float32(rec["max_abs"]) == mx, what
    assert int(rec["reserved"]) == 0, what
    if exact:
        assert (rec["sum"], rec["sum_sq"], rec["dist_sq"]) == (s, q, d), what
    else:
        # two orders of an fp64 sum of m exact terms differ by at most about 2 m 2^-53, relatively
        assert abs(rec["sum"] - s) <= 2 * m * EPS * sabs, what
        assert abs(rec["sum_sq"] - q) <= 2 * m * EPS * q, what
        assert abs(rec["dist_sq"] - d) <= 2 * m * EPS * d, what


def check_all(out, variables, z, bufs, exact):
    """Every whole-model and per-variable record of a modelStats(per_variable=True) result."""
    base, reps, bv, rv = out
    assert base.shape == (1,) and reps.shape == (len(bufs),)
    assert bv.shape == (1, len(variables)) and rv.shape == (len(bufs), len(variables))
    check(base[0], z, None, exact, "z")
    for i, x in enumerate(bufs):
        check(reps[i], x, z, exact, f"replica {i}")
    lo = 0
    for v, cnt in enumerate(variables):
        hi = lo + cnt
        check(bv[0, v], z[lo:hi], None, exact, f"z var {v}")
        for i, x in enumerate(bufs):
            check(rv[i, v], x[lo:hi], z[lo:hi], exact, f"replica {i} var {v}")
        lo = hi


@functools.lru_cache(maxsize=None)
def integer_inputs(n, R):
    """Small integers: every sum is exact in fp64 in any order."""
    rng = np.random.default_rng(1234 + n)
    z = rng.integers(-8, 9, n).astype(np.float32)
    w = tuple(rng.integers(-8, 9, n).astype(np.float32) for _ in range(R))
    for a in (z,) + w:
        a.setflags(write=False)
    return z, w


@functools.lru_cache(maxsize=None)
def normal_inputs(n, R):
    rng = np.random.default_rng(99 + n)
    z = (0.05 * rng.standard_normal(n)).astype(np.float32)
    w = tuple((z + 0.01 * rng.standard_normal(n)).astype(np.float32) for _ in range(R))
    for a in (z,) + w:
        a.setflags(write=False)
    return z, w


EXACT = [((1,), 1), ((1,), 8), ((1,), 9), ((4097,), 1), ((4097,), 8), ((4097,), 9),
         ((N_TRIPS,), 1), ((N_TRIPS,), 8), ((N_TRIPS,), 9), (RAGGED, 1), (RAGGED, 8), (RAGGED, 9)]


@pytest.mark.parametrize("variables,R", EXACT, ids=[f"n{sum(v)}-v{len(v)}-R{r}" for v, r in EXACT])
def test_exact_on_small_integers(variables, R):
    z, w = integer_inputs(sum(variables), R)
    with make_ctx(variables, R) as g:
        put(g, z, w)
        assert [(v["op"], v["order"], v["elements"]) for v in g.modelVariables()] == \
            [(op, 1, cnt) for op, cnt in enumerate(variables)]
        assert [v["offset"] for v in g.modelVariables()] == [sum(variables[:k]) for k in range(len(variables))]
        out = g.modelStats(per_variable=True)
        check_all(out, variables, z, w, exact=True)
        base, reps = g.modelStats()
        assert base.tobytes() == out[0].tobytes() and reps.tobytes() == out[1].tobytes()


ROUNDED = [(RAGGED, 8), ((N_TRIPS,), 9), ((4097,), 1)]


@pytest.mark.parametrize("variables,R", ROUNDED, ids=[f"n{sum(v)}-v{len(v)}-R{r}" for v, r in ROUNDED])
def test_rounded_within_the_reordering_bound(variables, R):
    z, w = normal_inputs(sum(variables), R)
    with make_ctx(variables, R) as g:
        put(g, z, w)
        check_all(g.modelStats(per_variable=True), variables, z, w, exact=False)


def test_nonfinite_values_wherever_they_fall():
    n, R = N_RAGGED, 3
    z0, w0 = integer_inputs(n, R)
    nan, inf = np.float32("nan"), np.float32("inf")
    # element 0, element n - 1, both sides of the boundary at 39 (inside the float4 36..39)
    spots = [(0, nan), (n - 1, inf), (38, -inf), (39, nan), (4131, inf), (4132, -inf)]
    with make_ctx(RAGGED, R) as g:
        # in one replica only: replica 1; the others and z stay clean
        w = [a.copy() for a in w0]
        for i, v in spots:
            w[1][i] = v
        put(g, z0, w)
        out = g.modelStats(per_variable=True)
        check_all(out, RAGGED, z0, w, exact=True)
        assert [int(r["nonfinite"]) for r in out[1]] == [0, len(spots), 0]
        assert int(out[0][0]["nonfinite"]) == 0
        assert [int(x) for x in out[3][1]["nonfinite"]] == [1, 0, 1, 2, 1, 1]
        # in z only: every replica's dist_sq skips those elements, its nonfinite stays 0
        z = z0.copy()
        for i, v in spots:
            z[i] = v
        put(g, z, w0)
        out = g.modelStats(per_variable=True)
        check_all(out, RAGGED, z, w0, exact=True)
        assert int(out[0][0]["nonfinite"]) == len(spots)
        keep = np.ones(n, dtype=bool)
        keep[[i for i, _ in spots]] = False
        for i in range(R):
            assert int(out[1][i]["nonfinite"]) == 0
            d = w0[i][keep].astype(np.float64) - z0[keep].astype(np.float64)
            assert out[1][i]["dist_sq"] == float(np.sum(d * d))
            assert out[1][i]["sum"] == float(np.sum(w0[i].astype(np.float64)))
        # every value of a buffer non-finite: max_abs 0, sums 0
        put(g, z0, [np.full(n, nan, np.float32)] + [a for a in w0[1:]])
        base, reps = g.modelStats()
        assert (reps[0]["sum"], reps[0]["sum_sq"], reps[0]["dist_sq"], reps[0]["max_abs"]) == (0.0, 0.0, 0.0, 0.0)
        assert int(reps[0]["nonfinite"]) == n


def test_two_calls_return_identical_bytes():
    z, w = normal_inputs(N_TRIPS, 9)
    with make_ctx((N_TRIPS,), 9) as g:
        put(g, z, w)
        a = g.modelStats(per_variable=True)
        b = g.modelStats(per_variable=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        pass_ms, total_ms = g.model_stats_last_ms()
        assert 0 < pass_ms <= total_ms


def test_read_only_and_the_next_step_is_still_bitexact():
    from crossbow_amd import BUF_DATA, BUF_DIFF
    from oracle import oracle as O
    n, R = 4099, 4
    st = O.make_state(n, 1, R, 0.1, 0.9)
    g = H.make_gpu(n, R, 0.1, 0.9)
    try:
        H.upload(g, st)
        g.modelStats(BUF_DATA, per_variable=True)
        g.modelStats(BUF_DIFF)
        H.compare_states(H.download(g, st), st)  # z, last, every w and every s: bit-identical
        g.lockAny()
        g.synchronise(0, 1, 0, False)
        g.modelStats(BUF_DATA)  # between lock and unlock, behind an enqueued step
        g.unlockAny()
        g.wait()
        O.sma_step(st)
        H.compare_states(H.download(g, st), st)
    finally:
        g.free()


def test_kind_diff_measures_s_not_w():
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, CbxError, _lib
    z, w = integer_inputs(N_RAGGED, 3)
    s = [np.roll(a, 7) + np.float32(1) for a in w]
    with make_ctx(RAGGED, 3) as g:
        put(g, z, w, s)
        check_all(g.modelStats(BUF_DIFF, per_variable=True), RAGGED, z, s, exact=True)
        check_all(g.modelStats(BUF_DATA, per_variable=True), RAGGED, z, w, exact=True)
        with pytest.raises(CbxError) as e:
            g.modelStats(BUF_GRADIENT)
        assert e.value.code == _lib.CBX_ERR_INVALID


def test_seam_over_unpadded_buffers_equals_the_context():
    import torch

    from crossbow_amd.seam import SmaPlan
    n, R = 4099, 3
    variables = (1, 3, 35, 4060)
    z, w = normal_inputs(n, R)
    dev = torch.device("cuda:0")
    zt = torch.from_numpy(z.copy()).to(dev)
    wt = [torch.from_numpy(a.copy()).to(dev) for a in w]
    assert zt.numel() == n and all(t.numel() == n for t in wt)  # exactly n floats: the unpadded tail
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], n) as plan:
        r, o, rv, ov = plan.buffer_stats(0, stream.cuda_stream, zt.data_ptr(), [t.data_ptr() for t in wt],
                                         var_elements=variables, per_variable=True)
        r1, o1 = plan.buffer_stats(0, stream.cuda_stream, zt.data_ptr(), [t.data_ptr() for t in wt])
    with make_ctx(variables, R) as g:
        put(g, z, w)
        base, reps, bv, rvs = g.modelStats(per_variable=True)
    check_all((np.array([r]), o, rv[None, :], ov), variables, z, w, exact=False)
    # the same piece table and summation tree: the same bits
    assert r.tobytes() == base[0].tobytes() and o.tobytes() == reps.tobytes()
    assert rv.tobytes() == bv[0].tobytes() and ov.tobytes() == rvs.tobytes()
    # one variable (nvars = 0) sums the same pieces of a different table: within the bound
    check(r1, z, None, False, "seam z, one variable")
    for i in range(R):
        check(o1[i], w[i], z, False, f"seam buffer {i}, one variable")


def test_checkpoint_guard(tmp_path):
    from crossbow_amd import BUF_DATA, CbxError, _lib
    n, R = 4099, 2
    z, w = normal_inputs(n, R)
    bad = w[1].copy()
    bad[4098] = np.float32("nan")
    d = str(tmp_path)
    with make_ctx((1, 3, 35, 4060), R) as g:
        put(g, z, [w[0], bad])
        g.setCheckpointGuard(True)
        with pytest.raises(CbxError) as e:
            g.checkpointModel(d)
        assert e.value.code == _lib.CBX_ERR_STATE
        assert "replica 1" in str(e.value) and "variable 3" in str(e.value)
        assert os.listdir(d) == []  # no version folder
        g.replica_write(1, BUF_DATA, w[1])  # repaired
        g.checkpointModel(d)
        assert os.listdir(d) == ["000001"]  # numbered as if the refused call had never happened
        assert np.array_equal(np.fromfile(os.path.join(d, "000001", "gpu-00-replica-001-data.dat"), np.float32), w[1])
        # guard off: the same poisoned model checkpoints as it does today
        g.setCheckpointGuard(False)
        g.replica_write(1, BUF_DATA, bad)
        g.checkpointModel(d)
        assert sorted(os.listdir(d)) == ["000001", "000002"]
        got = np.fromfile(os.path.join(d, "000002", "gpu-00-replica-001-data.dat"), np.float32)
        assert np.array_equal(got.view(np.uint32), bad.view(np.uint32))
        # and a non-finite momentum buffer is caught too
        from crossbow_amd import BUF_LAST
        g.replica_write(1, BUF_DATA, w[1])
        g.setCheckpointGuard(True)
        last = np.zeros(n, np.float32)
        last[0] = np.float32("inf")
        g.base_write(0, BUF_LAST, last)
        with pytest.raises(CbxError) as e:
            g.checkpointModel(d)
        assert e.value.code == _lib.CBX_ERR_STATE and "base model" in str(e.value) and "last" in str(e.value)
        assert sorted(os.listdir(d)) == ["000001", "000002"]
