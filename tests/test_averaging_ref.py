"""Pins the CPU restatement of the elastic-averaging and Polyak-Ruppert
barriers (tests/native/averaging_ref.c) before the GPU tests trust it:

* bit for bit against a replay of the reference's call sequence (memset,
  device copy, cuBLAS saxpy -> cblas_saxpy) on OpenBLAS, G = 1;
* the semantics that are easy to get wrong, against plain numpy;
* for G > 1, its per-device-then-rank-order sum against one chain over all
  replicas (synchronouseamsgd.c:141-273 chains every replica into the default
  device's accumulator), within the project's G > 1 tolerance.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV

N = 2053
RTOL, ATOL = 1e-5, 1e-6


def _eq(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _same_state(a: O.SmaState, b: O.SmaState) -> bool:
    pairs = list(zip(a.z + a.w + a.s, b.z + b.w + b.s))
    if a.last is not None:
        pairs += list(zip(a.last, b.last))
    return all(_eq(x, y) for x, y in pairs) and list(a.copy) == list(b.copy)


# ---- the OpenBLAS replay ----------------------------------------------------
def _saxpy():
    path = O.openblas_path()
    if path is None:
        return None
    h = ctypes.CDLL(path)
    f = getattr(h, "cblas_saxpy", None) or getattr(h, "scipy_cblas_saxpy")
    fp = ctypes.POINTER(ctypes.c_float)
    f.restype = None
    f.argtypes = [ctypes.c_int, ctypes.c_float, fp, ctypes.c_int, fp, ctypes.c_int]

    def saxpy(a, x, y):
        assert x.dtype == y.dtype == np.float32 and x.size == y.size
        f(x.size, a, x.ctypes.data_as(fp), 1, y.ctypes.data_as(fp), 1)
    return saxpy


def _replay_elastic(saxpy, st):
    """synchronouseamsgd.c:42-90 on one device."""
    z = st.z[0]
    gradient = np.zeros(st.n, np.float32)                  # :43
    for i in range(st.first, st.size):                     # :46
        if not st.locked[i]:
            continue
        diff = st.w[i].copy()                              # :55
        saxpy(-1.0, z, diff)                               # :56-61
        saxpy(-st.alpha, diff, st.w[i])                    # :64-69
        saxpy(st.alpha, diff, gradient)                    # :72-77
    saxpy(1.0, gradient, z)                                # :85-90


def _replay_polyak(saxpy, st, clock):
    """polyakruppert.c:15-16, 42-137 on one device; base->last is the
    reference's scratch, a private buffer where the model has none."""
    z = st.z[0]
    sf = np.float32(1.0 / float(np.float32(st.size)))      # :15
    raf = np.float32(1.0 / float(np.float32(clock + 1)))   # :16
    last = st.last[0] if st.last is not None else np.empty(st.n, np.float32)
    gradient = np.zeros(st.n, np.float32)                  # :43
    for i in range(st.first, st.size):                     # :46
        if not st.locked[i]:
            continue
        saxpy(sf, st.w[i], gradient)                       # :51-56
        last[:] = st.w[i]                                  # :63
        saxpy(-1.0, z, last)                               # :64-69
        if st.alpha != 0:                                  # :72
            saxpy(-st.alpha, last, st.w[i])                # :73-78
    last[:] = gradient                                     # :98
    saxpy(-1.0, z, last)                                   # :99-104
    saxpy(raf, last, z)                                    # :107-112
    for i in range(st.first, st.size):                     # :122
        if st.locked[i] and st.copy[i] > 0:                # :124-126
            st.w[i][:] = z                                 # :129
            st.copy[i] = 0                                 # :131


def test_restatement_equals_openblas_sequence():
    saxpy = _saxpy()
    if saxpy is None:
        pytest.skip("no OpenBLAS with a 32-bit-int cblas on this host")
    for polyak in (False, True):
        for R in (1, 2, 4, 8):
            for alpha in (0.1, 0.0):
                for momentum in (0.0, 0.9):  # without and with base->last
                    st = O.make_state(N, 1, R, alpha, momentum)
                    if R > 1:
                        st.copy[R - 1] = 1
                    a, b = st.clone(), st.clone()
                    if polyak:
                        AV.polyak_ruppert(a, 3)
                        _replay_polyak(saxpy, b, 3)
                    else:
                        AV.elastic_average(a)
                        _replay_elastic(saxpy, b)
                    assert _same_state(a, b), (polyak, R, alpha, momentum)


# ---- semantics ---------------------------------------------------------------
def test_elastic_ignores_momentum_and_copy_flags():
    plain = O.make_state(N, 1, 4, 0.1, 0.0)
    st = O.make_state(N, 1, 4, 0.1, 0.9)
    st.copy[:] = [0, 1, 0, 1]
    before = st.clone()
    AV.elastic_average(st)
    AV.elastic_average(plain)
    assert all(_eq(x, y) for x, y in zip(st.z + st.w, plain.z + plain.w))
    assert _eq(st.last[0], before.last[0]) and list(st.copy) == [0, 1, 0, 1]
    assert all(_eq(x, y) for x, y in zip(st.s, before.s))
    assert not _eq(st.z[0], before.z[0])


def test_elastic_reads_w_on_one_device_and_s_on_several():
    one = O.make_state(N, 1, 2, 0.1, 0.0)
    w0, z0 = [w.copy() for w in one.w], one.z[0].copy()
    for s in one.s:
        s[:] = np.nan  # never read at G = 1
    AV.elastic_average(one)
    for i in range(2):
        want = w0[i].astype(np.float64) - 0.1 * (w0[i].astype(np.float64) - z0)
        np.testing.assert_allclose(one.w[i], want, rtol=1e-6)
    assert np.all(np.isfinite(one.z[0]))
    two = O.make_state(N, 2, 1, 0.1, 0.0)
    w0, z0 = [w.copy() for w in two.w], two.z[0].copy()
    AV.elastic_average(two)
    for i in range(2):
        want = w0[i].astype(np.float64) - 0.1 * (two.s[i].astype(np.float64) - z0)
        np.testing.assert_allclose(two.w[i], want, rtol=1e-6)
    moved = sum(np.float64(0.1) * (two.s[i].astype(np.float64) - z0) for i in range(2))
    np.testing.assert_allclose(two.z[0], z0 + moved, rtol=1e-5, atol=1e-7)
    assert _eq(two.z[0], two.z[1])


def test_polyak_divides_by_every_replica_locked_or_not():
    st = O.make_state(N, 1, 4, 0.0, 0.0)
    st.locked[2] = 0
    w = [x.astype(np.float64) for x in st.w]
    AV.polyak_ruppert(st, 0)  # clock 0: z becomes acc
    np.testing.assert_allclose(st.z[0], (w[0] + w[1] + w[3]) / 4.0, rtol=1e-5, atol=1e-7)


def test_polyak_copies_only_into_flagged_replicas():
    st = O.make_state(N, 1, 4, 0.1, 0.9)
    st.copy[:] = [0, 1, 0, 1]
    st.locked[3] = 0  # flagged but not in the step: keeps its data and its flag
    before = st.clone()
    assert AV.polyak_ruppert(st, 2) == 1
    assert _eq(st.w[1], st.z[0]) and list(st.copy) == [0, 0, 0, 1]
    assert _eq(st.w[3], before.w[3])
    for i in (0, 2):
        assert not _eq(st.w[i], st.z[0]) and not _eq(st.w[i], before.w[i])
    # base->last is left holding acc - z (polyakruppert.c:98-104): z' = z + L / 3
    L = st.last[0].astype(np.float64)
    np.testing.assert_allclose(st.z[0], before.z[0] + L / 3.0, rtol=1e-5, atol=1e-7)


def test_polyak_with_alpha_zero_leaves_the_replicas_alone():
    st = O.make_state(N, 1, 3, 0.0, 0.0)
    before = st.clone()
    AV.polyak_ruppert(st, 1)
    assert all(_eq(x, y) for x, y in zip(st.w, before.w))
    assert not _eq(st.z[0], before.z[0])


@pytest.mark.parametrize("polyak", [False, True])
def test_first_and_unlocked_replicas_are_skipped(polyak):
    st = O.make_state(N, 1, 6, 0.1, 0.0)
    st.first = 2
    st.locked[4] = 0
    before = st.clone()
    AV.step(st, polyak, 1)
    for i in (0, 1, 4):
        assert _eq(st.w[i], before.w[i])
    # the same step over the three replicas that took part (6 in all for the 1 / p of Polyak-Ruppert)
    sub = before.clone()
    keep = [2, 3, 5]
    for i in (0, 1, 4):
        sub.w[i] = np.zeros(N, np.float32)
        sub.s[i] = np.zeros(N, np.float32)
    sub.locked[:] = [1 if i in keep else 0 for i in range(6)]
    sub.first = 0
    AV.step(sub, polyak, 1)
    assert _eq(st.z[0], sub.z[0]) and all(_eq(st.w[i], sub.w[i]) for i in keep)


def test_polyak_z_is_the_running_mean_of_the_replica_mean():
    # Values near 1, so no element of the mean sits near zero and a relative
    # tolerance is meaningful; the step does not move w (alpha = 0).
    st = O.make_state(N, 1, 4, 0.0, 0.0)
    st.z[0] += np.float32(1.0)
    for w in st.w:
        w += np.float32(1.0)
    mean = np.mean([w.astype(np.float64) for w in st.w], axis=0)
    running = np.zeros(N, np.float64)
    for clock in range(5):
        AV.polyak_ruppert(st, clock)
        running += (mean - running) / (clock + 1)
        np.testing.assert_allclose(st.z[0], running, rtol=1e-6)


# ---- summation order ----------------------------------------------------------
def _f(x):
    return np.asarray(x, np.float32)


def _chain_elastic(st):
    """One accumulator over every replica, device by device
    (synchronouseamsgd.c:141-273), fp32 with each fma through fp64: the
    product of two floats is exact in a double."""
    z = st.z[0].copy()
    acc = np.zeros(st.n, np.float32)
    a = np.float64(np.float32(st.alpha))
    w = [x.copy() for x in st.w]
    for g in range(st.G):
        for i in range(g, st.size, st.G):
            d = _f(st.s[i] - z)
            w[i] = _f(w[i].astype(np.float64) - a * d)
            acc = _f(acc.astype(np.float64) + a * d)
    return _f(z + acc), w


def _chain_polyak(st, clock):
    z = st.z[0].copy()
    acc = np.zeros(st.n, np.float32)
    sf = np.float64(np.float32(1.0 / float(np.float32(st.size))))
    raf = np.float64(np.float32(1.0 / float(np.float32(clock + 1))))
    a = np.float64(np.float32(st.alpha))
    w = [x.copy() for x in st.w]
    for g in range(st.G):
        for i in range(g, st.size, st.G):
            acc = _f(acc.astype(np.float64) + sf * w[i])
            d = _f(w[i] - z)
            w[i] = _f(w[i].astype(np.float64) - a * d)
    L = _f(acc - z)
    return _f(z.astype(np.float64) + raf * L), w


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("polyak", [False, True])
def test_per_device_sums_against_one_chain(G, polyak):
    st = O.make_state(N, G, 3, 0.1, 0.0)
    z, w = _chain_polyak(st, 2) if polyak else _chain_elastic(st)
    AV.step(st, polyak, 2)
    for g in range(G):
        assert _eq(st.z[g], st.z[0])
    # every element, no exclusions
    np.testing.assert_allclose(st.z[0], z, rtol=RTOL, atol=ATOL)
    for i in range(st.size):
        np.testing.assert_allclose(st.w[i], w[i], rtol=RTOL, atol=ATOL)
