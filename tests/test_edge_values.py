"""Pins the edge-value inputs (tests/edge_values.py) on the CPU, before any
kernel sees them:

* the fma oracle and its OpenBLAS replay agree bit for bit on them, NaNs
  included (both run on this host's ISA), for every operation the GPU edge
  tests take their expectation from;
* the inputs bite: the expected outputs hold both zeros, subnormals, both
  infinities, an inf and a NaN that arithmetic produced, a subnormal produced
  from normal inputs;
* at most a quarter of any compared output array is NaN, so the relaxed NaN
  rule of ``assert_edge_equal`` cannot hollow out the compare;
* a device that flushed subnormals to zero would be seen;
* the one place where the fma form and the BLAS replay part: a scalar of
  exactly 0 over non-finite data (the edge-value contract).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import edge_values as E
from tests.helpers import assert_bitexact
from tests.test_averaging_ref import _replay_elastic, _replay_polyak, _saxpy

WPC = 6
RATE = np.float32(-E.LR)


def _need_blas():
    if O.openblas_path() is None:
        pytest.skip("no OpenBLAS with a 32-bit-int cblas on this host")


class Op:
    """One operation on edge inputs: ``make`` builds the named input arrays,
    ``run`` steps them in place and returns the compared outputs by name."""

    def __init__(self, name, make, run, fma_tie=None):
        self.name, self.make, self.run, self.fma_tie = name, make, run, fma_tie

    def __repr__(self):
        return self.name


def _sma(R, momentum):
    def make():
        st, labels = E.sma_case(R, momentum)
        return st, labels

    def run(st, blas=False):
        (O.sma_step_blas if blas else O.sma_step)(st)
        out = {"z": st.z[0]}
        if st.last is not None:
            out["last"] = st.last[0]
        out.update({f"w{i}": st.w[i] for i in range(st.size)})
        return out
    return Op(f"sma-R{R}-mom{momentum}", make, run, fma_tie=(-E.ALPHA, 3.0))


def _averaging(polyak, momentum, clock=3):
    def make():
        st, labels = E.averaging_case(3, momentum)
        st.copy[1] = 1
        return st, labels

    def run(st, blas=False):
        if blas:
            (_replay_polyak(_saxpy(), st, clock) if polyak else _replay_elastic(_saxpy(), st))
        else:
            AV.step(st, polyak, clock)
        out = {"z": st.z[0]}
        if polyak and st.last is not None:
            out["last"] = st.last[0]
        out.update({f"w{i}": st.w[i] for i in range(st.size)})
        return out
    return Op(f"{'polyak' if polyak else 'elastic'}-mom{momentum}", make, run)


def _task(kind, momentum, wd):
    extra = {"optimise": (), "default": ("z",), "worker": ("acc",)}[kind]

    def make():
        return E.optimiser_case(momentum, wd, RATE, extra=extra, last=kind != "worker")

    def run(a, blas=False):
        if kind == "optimise":
            O.sma_optimise(RATE, momentum, wd, a["w"], a["g"], a["last"], a["s"], blas=blas)
            out = {x: a[x] for x in ("w", "g", "s")}
        elif kind == "default":
            O.default_task(RATE, momentum, wd, a["w"], a["g"], a["last"], a["z"], blas=blas)
            out = {x: a[x] for x in ("w", "g", "z")}
        else:
            O.ssgd_worker(RATE, wd, a["w"], a["g"], a["acc"], blas=blas)
            out = {x: a[x] for x in ("g", "acc")}
        if a.get("last") is not None:
            out["last"] = a["last"]
        return out
    tie = (float(RATE), 3.0) if kind == "optimise" and momentum == 0 and wd == 0 else None
    return Op(f"{kind}-mom{momentum}-wd{wd}", make, run, fma_tie=tie)


def _ssgd_sync(momentum):
    def make():
        st = O.make_state(E.N, 1, 3, E.ALPHA, momentum)
        acc = O.fill_normal(E.N, 777, 0.01)
        arrays = {"z": st.z[0], "acc": acc}
        if st.last is not None:
            arrays["last"] = st.last[0]
        labels = E.apply(arrays, E.ssgd_sync_scenarios(momentum > 0, WPC))
        return (st, acc), labels

    def run(sa, blas=False):
        st, acc = sa
        O.ssgd_sync(st, [acc], WPC, blas=blas)
        out = {"z": st.z[0], "w0": st.w[0]}
        if st.last is not None:
            out["last"] = st.last[0]
        return out
    return Op(f"ssgd-sync-mom{momentum}", make, run)


CONFIGS = [(0.9, 5e-4), (0.0, 0.0), (0.0, 5e-4), (0.9, 0.0)]
OPS = ([_sma(R, m) for R in (3, 9) for m in (0.0, 0.9)]
       + [_task(kind, m, wd) for kind in ("optimise", "default") for m, wd in CONFIGS]
       + [_task("worker", 0.0, wd) for wd in (0.0, 5e-4)]
       + [_ssgd_sync(m) for m in (0.0, 0.9)]
       + [_averaging(p, m) for p in (False, True) for m in (0.0, 0.9)])
IDS = [op.name for op in OPS]


def _arrays(x):
    """Every fp32 input array of an operation's inputs."""
    if isinstance(x, dict):
        return [a for a in x.values() if a is not None]
    if isinstance(x, tuple):
        return _arrays(x[0]) + [x[1]]
    return x.z + (x.last or []) + x.s + x.w


def test_layout_two_copies_on_different_lanes_bulk_and_tail():
    assert E.N % 4 != 0 and E.N < 16_384
    for op in OPS:
        _, labels = op.make()
        idx = [k for k, x in enumerate(labels) if x is not None]
        L = len(idx) // 2
        first, second = idx[0], idx[L]
        assert idx == list(range(first, first + L)) + list(range(second, second + L))
        assert labels[first:first + L] == labels[second:second + L]
        assert first + L <= 2048 <= second and second + L == E.N, (op, first, second, L)
        assert (second - first) % 4 != 0


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_fma_oracle_equals_its_openblas_replay_on_edge_inputs(op):
    _need_blas()
    a, labels = op.make()
    b, _ = op.make()
    got, want = op.run(a), op.run(b, blas=True)
    assert got.keys() == want.keys()
    for name in got:
        try:
            assert_bitexact(got[name], want[name], f"{op.name} {name}")
        except AssertionError as e:
            k = int(np.nonzero(E.bits(got[name]) != E.bits(want[name]))[0][0])
            raise AssertionError(f"{e} (scenario: {labels[k]})") from None


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_inputs_bite(op):
    a, labels = op.make()
    inputs = [x.copy() for x in _arrays(a)]
    out = op.run(a)
    c = E.census(out.values())
    for kind in ("+0", "-0", "subnormal", "+inf", "-inf", "nan"):
        assert c[kind] > 0, (op.name, kind, c)
    scen = np.array([x is not None for x in labels])
    any_in = lambda pred: np.any([pred(x) for x in inputs], axis=0)  # noqa: E731
    finite_in = ~any_in(lambda x: ~np.isfinite(x))
    no_nan_in = ~any_in(np.isnan)
    normal_in = ~any_in(lambda x: ~np.isfinite(x) | E.is_subnormal(x) | (x == 0))
    made_inf = sum(int(np.sum(np.isinf(o) & finite_in)) for o in out.values())
    made_nan = sum(int(np.sum(np.isnan(o) & no_nan_in)) for o in out.values())
    made_sub = sum(int(np.sum(E.is_subnormal(o) & normal_in)) for o in out.values())
    assert made_inf > 0, f"{op.name}: no inf from finite inputs"
    assert made_nan > 0, f"{op.name}: no NaN from non-NaN inputs"
    assert made_sub > 0, f"{op.name}: no subnormal from normal inputs"
    # outside the scenarios the data is ordinary: every special value comes from one
    for o in out.values():
        assert np.all(np.isfinite(o[~scen]) & ~E.is_subnormal(o[~scen]) & (o[~scen] != 0))


@pytest.mark.parametrize("op", [o for o in OPS if o.name.startswith(("sma", "optimise", "default"))],
                         ids=lambda o: o.name)
def test_signed_zero_block_holds_both_signs(op):
    """The all-zero elements.  In the task steps every output takes both signs.
    In the SMA step only w can: acc starts at +0, and under round-to-nearest a
    sum with +0 is never -0, so D, the base last and z come out +0 for every
    sign combination -- an accumulator started at -0, or fma(alpha, d, +0)
    folded to alpha*d, would show as a -0 here.  (Their -0 comes from the
    scenario in which every alpha*d underflows to -0.)"""
    a, labels = op.make()
    out = op.run(a)
    block = np.array([x is not None and x.startswith("zeros ") for x in labels])
    assert block.sum() >= 2 * 4
    for name, o in out.items():
        b = E.bits(o[block])
        assert np.all((b == E.PZERO) | (b == E.NZERO)), (op.name, name)
        if op.name.startswith("sma") and name in ("z", "last"):
            assert np.all(b == E.PZERO), (op.name, name)
            assert np.any(E.bits(o) == E.NZERO), f"{op.name} {name}: no -0 from the underflow scenario"
        else:
            assert np.any(b == E.PZERO) and np.any(b == E.NZERO), (op.name, name)


@pytest.mark.parametrize("op", [o for o in OPS if o.fma_tie], ids=lambda o: o.name)
def test_the_tie_scenario_separates_fma_from_multiply_then_add(op):
    c, x = op.fma_tie
    y = -float(np.float32(c) * np.float32(x))
    fma, muladd = E.fma_and_muladd(c, x, y)
    assert fma != muladd and muladd == 0 and fma != 0
    a, labels = op.make()
    out = op.run(a)
    k = [i for i, s in enumerate(labels) if s and "round differently" in s]
    assert len(k) >= 2
    name = "w0" if op.name.startswith("sma") else "w"
    assert np.all(E.bits(out[name][k]) == E.bits(np.array([fma])))


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_nan_cap(op):
    a, _ = op.make()
    for name, o in op.run(a).items():
        assert E.nan_fraction(o) <= 0.25, (op.name, name, E.nan_fraction(o))


def test_nan_cap_of_the_fused_inputs():
    from tests.test_gpu_seam_step_and_optimise import CONFIGS as FUSED, Data
    for R, steps in ((3, [True] * 3), (9, [i in (0, 3, 8) for i in range(9)])):
        for rmom, wd, bmom in FUSED.values():
            d = Data(E.N, R, rmom, bmom)
            rates = E.replica_rates(R)
            E.fused_case(d, rmom, wd, rates, steps)
            d.step(steps, rates, wd)
            outs = [d.st.z[0]] + d.st.w + d.st.s + d.g + [x for x in d.last if x is not None] + (d.st.last or [])
            assert max(E.nan_fraction(o) for o in outs) <= 0.25
            c = E.census(outs)
            assert all(v > 0 for v in c.values()), c


def _fused_cases():
    from tests.test_gpu_seam_step_and_optimise import CONFIGS as FUSED, Data
    for R, steps in ((3, [True] * 3), (9, [i in (0, 3, 8) for i in range(9)])):
        for name, (rmom, wd, bmom) in FUSED.items():
            for keep in (True, False):
                def make(flush=False):
                    d = Data(E.N, R, rmom, bmom)
                    rates = E.replica_rates(R)
                    labels = E.fused_case(d, rmom, wd, rates, steps)
                    ins = [d.st.z[0]] + d.st.w + d.st.s + d.g + [x for x in d.last if x is not None] + (d.st.last or [])
                    if flush:
                        for x in ins:
                            _flush(x)
                    d.step(steps, rates, wd, keep=keep)
                    out = {"z": d.st.z[0]}
                    if d.st.last is not None:
                        out["last"] = d.st.last[0]
                    for i in range(R):
                        out.update({f"w{i}": d.st.w[i], f"s{i}": d.st.s[i], f"g{i}": d.g[i]})
                        if d.last[i] is not None:
                            out[f"r{i}"] = d.last[i]
                    return out, labels
                yield f"R{R}-{name}-{'keep' if keep else 'discard'}", make


def test_flush_to_zero_would_be_seen_in_the_fused_step():
    """In every configuration, mask and flag of the fused task steps, in an
    output that is arithmetic (z, w): s and g may be copies or unwritten."""
    for name, make in _fused_cases():
        want, labels = make()
        got, _ = make(flush=True)
        seen = [k for k in want if k[0] in "zw" and E.edge_mismatches(got[k], want[k]).size]
        assert seen, f"{name}: flushed inputs went unseen"
        flushed = {k: v.copy() for k, v in want.items()}
        for v in flushed.values():
            _flush(v)
        assert any(E.edge_mismatches(flushed[k], want[k]).size for k in want if k[0] in "zw"), name


def _sma_zero_block(st, idx, acc0):
    """The SMA step on all-zero elements in numpy fp32 (exact there, signs by
    IEEE 754), with the accumulator started at ``acc0``."""
    z = st.z[0][idx].copy()
    acc = np.full(z.size, acc0, np.float32)
    a = np.float32(st.alpha)
    for i in range(st.size):
        d = st.s[i][idx] - z
        acc = a * d + acc
    if st.last is not None:
        acc = np.float32(0.9) * st.last[0][idx] + acc
    return z + acc, acc


@pytest.mark.parametrize("R", [3, 9])
def test_an_accumulator_started_at_minus_zero_would_be_seen(R):
    st, labels = E.sma_case(R, 0.9)
    idx = np.array([k for k, x in enumerate(labels) if x is not None and x.startswith("zeros ")])
    z_ok, last_ok = _sma_zero_block(st, idx, np.float32(0.0))
    z_bad, last_bad = _sma_zero_block(st, idx, np.float32(-0.0))
    O.sma_step(st)
    assert_bitexact(z_ok, st.z[0][idx], "the emulation's z")
    assert_bitexact(last_ok, st.last[0][idx], "the emulation's last")
    # every s is -0 while z is +0 and last is -0: D and last' turn -0
    assert E.edge_mismatches(last_bad, st.last[0][idx]).size > 0
    # Polyak-Ruppert: acc = sum w_i / p shows it wherever every w is -0
    st, labels = E.averaging_case(3, 0.9)
    idx = np.array([k for k, x in enumerate(labels) if x is not None and x.startswith("zeros ")])
    assert np.any(np.all([E.bits(w[idx]) == E.NZERO for w in st.w], axis=0))


_flush = E.flush


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_flush_to_zero_would_be_seen(op):
    a, _ = op.make()
    want = op.run(a)
    # a device that flushes its inputs
    b, labels = op.make()
    for x in _arrays(b):
        _flush(x)
    got = op.run(b)
    failed = 0
    for name in want:
        try:
            E.assert_edge_equal(got[name], want[name], name, labels)
        except AssertionError as e:
            assert "scenario: " in str(e) and "ordinary data" not in str(e), str(e)
            failed += 1
    assert failed > 0, f"{op.name}: flushed inputs went unseen"
    # a device that flushes its outputs
    failed = 0
    for name in want:
        flushed = want[name].copy()
        _flush(flushed)
        try:
            E.assert_edge_equal(flushed, want[name], name, labels)
        except AssertionError:
            failed += 1
    assert failed > 0, f"{op.name}: flushed outputs went unseen"


def test_assert_edge_equal_rules():
    q, p, s = (np.array([v], np.uint32).view(np.float32) for v in (E.QNAN, E.PAYLOAD_NAN, E.SNAN))
    E.assert_edge_equal(p, q)                       # any NaN for a NaN
    E.assert_edge_equal(np.array([0xFFC00000], np.uint32).view(np.float32), s)
    for got, want in ((np.float32([0.0]), np.float32([-0.0])), (np.float32([1.0]), q), (q, np.float32([1.0])),
                      (np.float32([np.inf]), q), (np.float32([1e-45]), np.float32([0.0]))):
        with pytest.raises(AssertionError, match="1 of 1 elements differ; first at 0"):
            E.assert_edge_equal(got, want, "x")
    with pytest.raises(AssertionError):            # the strict compare still sees a payload
        assert_bitexact(p, q)
    with pytest.raises(AssertionError, match=r"scenario: the label"):
        E.assert_edge_equal(np.float32([0.0, 1.0]), np.float32([0.0, 2.0]), "x", [None, "the label"])


def test_alpha_zero_and_rate_zero_part_the_fma_form_from_the_blas_replay():
    """OpenBLAS returns from saxpy at once when the scalar is 0, so y stays put;
    fmaf(0, NaN or inf, y) is NaN.  The kernels take the fma form.  What cuBLAS
    does is unobserved.  (the edge-value contract.)"""
    _need_blas()
    n, R = 64, 3
    special = {5: E.QNAN, 6: E.SNAN, 9: E.PINF, 10: E.NINF}
    idx = sorted(special)
    rest = np.ones(n, bool)
    rest[idx] = False
    # alpha = 0, a NaN and an inf in s
    a = O.make_state(n, 1, R, 0.0, 0.9)
    for k, v in special.items():
        a.s[1].view(np.uint32)[k] = v
    b, before = a.clone(), a.clone()
    O.sma_step(a)
    O.sma_step_blas(b)
    for k in idx:
        for name, x, y, x0 in [("z", a.z[0], b.z[0], None), ("last", a.last[0], b.last[0], None),
                               ("w1", a.w[1], b.w[1], before.w[1])]:
            assert np.isnan(x[k]), (name, k, "the fma form yields NaN")
            assert np.isfinite(y[k]), (name, k, "the replay leaves the destination finite")
            if x0 is not None:
                assert E.bits(y)[k] == E.bits(x0)[k], (name, k, "the replay leaves the destination unchanged")
    # with alpha = 0 the replay's acc stays 0: z moves by the momentum alone
    want_last = (np.float32(0.9) * before.last[0].astype(np.float64)).astype(np.float32)
    assert_bitexact(b.last[0], want_last, "the replay's last")
    for x, y, name in [(a.z[0], b.z[0], "z"), (a.last[0], b.last[0], "last")] + \
            [(a.w[i], b.w[i], f"w{i}") for i in range(R)]:
        assert_bitexact(x[rest], y[rest], f"{name} off the special elements")
    for i in (0, 2):
        assert_bitexact(a.w[i], before.w[i], f"w{i}: finite data times 0 changes nothing")
    # rate = 0 without momentum, a NaN and an inf in g
    w = O.fill_normal(n, 1, 0.05)
    g = O.fill_normal(n, 2, 0.01)
    for k, v in special.items():
        g.view(np.uint32)[k] = v
    w2, g2, w0 = w.copy(), g.copy(), w.copy()
    O.sma_optimise(np.float32(-0.0), 0.0, 0.0, w, g, None, np.zeros(n, np.float32))
    O.sma_optimise(np.float32(-0.0), 0.0, 0.0, w2, g2, None, np.zeros(n, np.float32), blas=True)
    for k in idx:
        assert np.isnan(w[k]), (k, "the fma form yields NaN")
        assert E.bits(w2)[k] == E.bits(w0)[k], (k, "the replay leaves w unchanged")
    assert_bitexact(w[rest], w2[rest], "w off the special elements")
    assert_bitexact(w2, w0, "the replay's w")
