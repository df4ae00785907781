"""IEEE edge values for the step kernels: signed zeros, subnormals, the ends of
the fp32 range, infinities, NaNs, exact cancellations and an fma tie.

Every parity test elsewhere feeds the kernels ``oracle.fill_normal`` data.  The
tests built on this module keep that data as the base of every buffer and
overwrite single elements with *scenarios*: one element each, a value for some
of the buffers that element of the operation reads.  The scenario list is
written twice (``layout``): once inside the float4 bulk and once, shifted by
one lane, against the end of the buffer, which the ``TAIL`` workgroups of the
seam kernels take and which lies against the arena's padding in a context.

Values are carried as uint32 bit patterns throughout: a signalling NaN does not
survive a conversion through a Python float.

The comparison (``assert_edge_equal``) and its reasons are DESIGN.md's
edge-value contract: where the reference holds a NaN the device must hold a NaN
of any sign and payload (the default NaN and the payload an fma propagates are
ISA-defined); everywhere else the 32 bits are equal.  Buffers that are copies
in the reference are compared with ``tests.helpers.assert_bitexact``, NaN
payloads included.

The last section serves the two reductions (the gradient norm and the model
statistics; tests/test_reduction_edges.py, tests/test_gpu_reduction_edges.py):
whole-buffer regimes whose fp64 sums are exact in any order, a wide catalogue
over the pair (x, ref), and an exact reference in Python integers.

Test infrastructure only; not a conftest.
"""
from __future__ import annotations

import itertools
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# One size for every edge test: two whole 1,024-float chunks of bulk and a tail
# of 903 floats, which holds the longest scenario list; not a multiple of 4.
N = 2 * 1024 + 900 + 3
TAIL = N % 1024
assert N < 16_384 and N % 4 != 0

ALPHA = 0.1
LR = 0.05  # the base learning rate; the kernels see -rate
WD = 5e-4
# (replica momentum, weight decay) of the task steps: momentum + wd, plain, wd only, momentum only
OPT_CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD), "mom-only": (0.9, 0.0)}


def b32(x) -> int:
    """The bit pattern of ``x`` rounded to fp32."""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def f32(bits: int) -> np.float32:
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


PZERO, NZERO = 0x00000000, 0x80000000
MIN_SUB, MAX_SUB = 0x00000001, 0x007FFFFF
FLT_MIN, FLT_MAX = 0x00800000, 0x7F7FFFFF
PINF, NINF = 0x7F800000, 0xFF800000
QNAN, PAYLOAD_NAN, SNAN = 0x7FC00000, 0xFFC12345, 0x7FA00001
SIGN = 0x80000000
NANS = (("qnan", QNAN), ("payload-nan", PAYLOAD_NAN), ("snan", SNAN))

# every buffer in turn gets each of these
SWEEP = (("+min-sub", MIN_SUB), ("-min-sub", MIN_SUB | SIGN), ("+max-sub", MAX_SUB), ("-max-sub", MAX_SUB | SIGN),
         ("+FLT_MIN", FLT_MIN), ("-FLT_MIN", FLT_MIN | SIGN), ("+FLT_MAX", FLT_MAX), ("-FLT_MAX", FLT_MAX | SIGN),
         ("+inf", PINF), ("-inf", NINF)) + NANS

Scenario = Tuple[str, Dict[str, int]]  # (label, {buffer name: bit pattern})


def _scaled(bits: int, k: float) -> int:
    """``k`` times the value of ``bits``, which must be exact in fp32."""
    v = np.float64(f32(bits)) * k
    out = b32(v)
    assert np.float64(f32(out)) == v, (hex(bits), k)
    return out


def signed_zeros(names: Sequence[str], cover: Optional[Sequence[str]] = None) -> List[Scenario]:
    """Every sign combination of +-0 over ``cover`` (at most 6 buffers; default
    the first 5 names, or all of them).  Every other buffer of the element is a
    zero too, so that the whole element is zeros and the outputs are: replica
    i's buffer takes the sign of the same kind of buffer of replica i mod 2
    where the cover holds one (so every s can be -0 while z is +0, the one case
    in which the sign of the accumulator's start shows), any other buffer that
    of the cover buffer it is folded onto."""
    cover = list(cover if cover is not None else names[:5])
    assert len(cover) <= 6
    rest = [x for x in names if x not in cover]
    fold = {}
    for k, x in enumerate(rest):
        like = f"{x[0]}{int(x[1:]) % 2}" if x[1:].isdigit() else None
        fold[x] = cover.index(like) if like in cover else k % len(cover)
    out = []
    for combo in itertools.product((PZERO, NZERO), repeat=len(cover)):
        vals = dict(zip(cover, combo))
        for x in rest:
            vals[x] = combo[fold[x]]
        out.append(("zeros " + "".join("+" if c == PZERO else "-" for c in combo), vals))
    return out


def sweep(names: Sequence[str]) -> List[Scenario]:
    return [(f"{x}={label}", {x: v}) for x in names for label, v in SWEEP]


def pair_block(a: str, b: str) -> List[Scenario]:
    """The element takes d = a - b."""
    h = b32(0.75)
    return [
        (f"{a}-{b} underflows from a normal pair", {a: _scaled(FLT_MIN, 1.5), b: _scaled(FLT_MIN, 1.25)}),
        (f"{a}-{b} = 2 FLT_MIN", {a: FLT_MIN, b: FLT_MIN | SIGN}),
        (f"{a}-{b} overflows to +inf", {a: FLT_MAX, b: FLT_MAX | SIGN}),
        (f"{a}-{b} overflows to -inf", {a: FLT_MAX | SIGN, b: FLT_MAX}),
        (f"{a}=+inf {b}=+inf", {a: PINF, b: PINF}),
        (f"{a}=-inf {b}=-inf", {a: NINF, b: NINF}),
        (f"{a}=+inf {b}=-inf", {a: PINF, b: NINF}),
        (f"{a}=-inf {b}=+inf", {a: NINF, b: PINF}),
        (f"{a}=={b}: d = +0", {a: h, b: h}),
        (f"{a}=payload-nan {b}=snan", {a: PAYLOAD_NAN, b: SNAN}),
        (f"{a}=qnan {b}=payload-nan", {a: QNAN, b: PAYLOAD_NAN}),
    ]


def _direct(x: str):
    return lambda v: {x: v}


def _through(a: str, b: str):
    """Set d = a - b to the value of ``v`` exactly."""
    def put(v):
        x = abs(float(f32(v)))
        if np.isnan(x):
            return {a: v}
        if x >= 1e30:
            return {a: v, b: PZERO}
        if 0.5 <= x <= 1024.0:
            return {a: b32(float(f32(v)) + 1.0), b: b32(1.0)}
        return {a: _scaled(v, 1.5), b: _scaled(v, 0.5)}
    return put


def fma_block(put, xname: str, y: str, c: float) -> List[Scenario]:
    """The element takes y' = fma(c, x, y), c a scalar of magnitude below
    0.25; ``put(bits)`` gives the buffer values that make x that value."""
    c = float(np.float32(c))
    assert 0.0 < abs(c) < 0.25
    neg = SIGN if c > 0 else 0  # the sign bit of an x > 0 times -sign(c)
    out = []

    def add(label, xbits, ybits):
        vals = dict(put(xbits))
        assert y not in vals
        vals[y] = ybits
        out.append((f"{y}'=fma({c:g},{xname},{y}): {label}", vals))

    x4 = _scaled(FLT_MIN, 4.0)
    # |c*x| is below FLT_MIN: subnormal, and FLT_MIN less it is too
    add("c*x underflows from a normal x, the sum is subnormal", x4, FLT_MIN | neg)
    add("c*x underflows from a normal x, added to -0", x4, NZERO)
    # c*x has y's sign: the sum is past FLT_MAX
    add("overflows to +inf from finite operands", FLT_MAX | (0 if c > 0 else SIGN), FLT_MAX)
    add("overflows to -inf from finite operands", FLT_MAX | (SIGN if c > 0 else 0), FLT_MAX | SIGN)
    add("y = -c*x exactly: the sum is an exact zero", b32(1.0), b32(-c))
    # c*3 needs 26 bits: multiply-then-add gives 0 here, the fma the product's rounding error
    add("fma and multiply-then-add round differently", b32(3.0), b32(-float(np.float32(c) * np.float32(3.0))))
    add("two NaNs in one element", PAYLOAD_NAN, SNAN)
    add("NaN times c plus inf", QNAN, PINF)
    return out


def fma_and_muladd(c, x, y):
    """(fma(c, x, y), c*x + y with the product rounded) in fp32, through fp64:
    the product of two floats is exact in a double."""
    c, x, y = (np.float64(np.float32(v)) for v in (c, x, y))
    with np.errstate(all="ignore"):
        return np.float32(c * x + y), np.float32(np.float64(np.float32(c * x)) + y)


# ---- the operations' catalogues --------------------------------------------------
def sma_names(R: int, base_last: bool) -> List[str]:
    return ["z"] + (["last"] if base_last else []) + [f"{k}{i}" for i in range(R) for k in ("s", "w")]


def sma_scenarios(R: int, base_last: bool, alpha: float = ALPHA) -> List[Scenario]:
    """The SMA step: d = s_i - z, w_i' = fma(-alpha, d, w_i), acc = fma(alpha, d, acc)
    from +0, last' = D = fma(0.9, last, acc), z' = z + D."""
    names = sma_names(R, base_last)
    cover = [x for x in ("z", "last", "s0", "w0", "s1", "w1") if x in names]
    out = signed_zeros(names, cover) + sweep(names) + pair_block("s0", "z")
    out += fma_block(_through("s0", "z"), "s0-z", "w0", -alpha)
    if R > 1:
        out += pair_block(f"s{R - 1}", "z")[:2]
    # every alpha*d underflows to -0 and z, last are -0: the only way to a -0 in acc, last' and z'
    vals = {x: NZERO for x in names}
    vals.update({f"s{i}": MIN_SUB | SIGN for i in range(R)})
    out.append(("every alpha*d underflows to -0 onto z = last = -0", vals))
    vals = {x: PZERO for x in names}
    vals.update({f"s{i}": _scaled(FLT_MIN, 2.0) for i in range(R)})
    vals.update({f"w{i}": FLT_MIN for i in range(R)})
    out.append(("every alpha*d is subnormal: acc, last' and z' stay subnormal", vals))
    return out


def averaging_names(R: int, base_last: bool) -> List[str]:
    return ["z"] + (["last"] if base_last else []) + [f"w{i}" for i in range(R)]


def averaging_scenarios(R: int, base_last: bool) -> List[Scenario]:
    """Elastic averaging (d = w_i - z, w_i' = fma(-alpha, d, w_i), z' = z + sum alpha d)
    and Polyak-Ruppert (acc = sum w_i / p, L = acc - z, z' = fma(1/(clock+1), L, z))."""
    names = averaging_names(R, base_last)
    out = signed_zeros(names, names[:6]) + sweep(names) + pair_block("w0", "z")
    if R > 1:
        out += pair_block(f"w{R - 1}", "z")[:2]
    vals = {x: NZERO for x in names}
    vals.update({f"w{i}": MIN_SUB | SIGN for i in range(R)})
    out.append(("every w is -min-sub onto z = -0", vals))
    vals = {x: _scaled(FLT_MIN, 2.0) for x in names}
    vals["z"] = FLT_MIN
    out.append(("every w = 2 FLT_MIN, z = FLT_MIN", vals))
    vals = {x: FLT_MIN for x in names}
    vals["z"] = PZERO
    out.append(("every w = FLT_MIN onto z = +0: the mean's terms are subnormal", vals))
    return out


def optimiser_scenarios(rate: float, momentum: float, wd: float, w="w", g="g", last: Optional[str] = "last",
                        extra: Sequence[str] = (), zeros: bool = True) -> List[Scenario]:
    """The task steps: gk = fma(wd, w, g); with momentum gk = fma(mu, last, rate*gk),
    last' = gk, w' = w + gk; without, w' = fma(rate, gk, w).  ``rate`` is the
    negated learning rate; ``extra`` names further buffers the element reads
    (the base model of the DEFAULT step, the accumulator of S-SGD)."""
    names = [w, g] + ([last] if last is not None else []) + list(extra)
    out = (signed_zeros(names) if zeros else []) + sweep(names)
    out += fma_block(_direct(g), g, w, rate)
    if wd > 0:
        out += fma_block(_direct(w), w, g, wd)
    out += [(f"{w}=+inf {g}=+inf", {w: PINF, g: PINF}), (f"{w}=-inf {g}=-inf", {w: NINF, g: NINF}),
            (f"{w}=+inf {g}=-inf", {w: PINF, g: NINF}), (f"{w}=snan {g}=payload-nan", {w: SNAN, g: PAYLOAD_NAN})]
    if last is not None:
        out += [(f"{g}=+inf {last}=+inf", {g: PINF, last: PINF}), (f"{g}=+inf {last}=-inf", {g: PINF, last: NINF}),
                (f"{g}=qnan {last}=snan", {g: QNAN, last: SNAN}),
                # rate*g = -mu*last up to rounding: last' is the fma's rounding error or an exact zero
                (f"{last}' cancels", {g: b32(0.9), last: b32(-rate)}),
                (f"rate*{g} underflows onto a subnormal {last}", {g: _scaled(FLT_MIN, 4.0), last: MIN_SUB | SIGN}),
                # rate*g = -0.8 FLT_MIN is subnormal, and 0.9 FLT_MIN less it is too
                (f"{last}' is subnormal from normal operands", {w: FLT_MIN, g: _scaled(FLT_MIN, 16.0), last: FLT_MIN}),
                (f"everything FLT_MAX: {last}' and {w}' overflow", {w: FLT_MAX | SIGN, g: FLT_MAX, last: FLT_MAX | SIGN})]
    for x in extra:
        out += fma_block(_direct(g), g, x, rate)[:4]
        out += [(f"{g}=+inf {x}=+inf", {g: PINF, x: PINF}), (f"{g}=+inf {x}=-inf", {g: PINF, x: NINF})]
    # nothing here leaves the subnormal range: a flushed input or output changes every output
    vals = {w: MAX_SUB, g: 0x00400000}
    if last is not None:
        vals[last] = 0x00000100 | SIGN
    vals.update({x: 0x00200000 | SIGN for x in extra})
    out.append(("every operand subnormal", vals))
    return out


def ssgd_sync_scenarios(base_last: bool, wpc: int) -> List[Scenario]:
    """The S-SGD barrier: D = acc / wpc (rounded), D = fma(mu, last, D), z' = z + D."""
    names = ["z"] + (["last"] if base_last else []) + ["acc"]
    ratio = float(np.float32(1.0 / float(np.float32(wpc))))
    out = signed_zeros(names) + sweep(names) + pair_block("z", "acc")[2:] + fma_block(_direct("acc"), "acc", "z", ratio)
    vals = {"z": 0x00200000 | SIGN, "acc": 0x00400000}
    if base_last:
        vals["last"] = 0x00000100
        # acc / wpc is subnormal, and 0.9 FLT_MIN less it is too
        out.append(("last' is subnormal from normal operands",
                    {"z": FLT_MIN | SIGN, "last": FLT_MIN | SIGN, "acc": _scaled(FLT_MIN, 4.0)}))
    out.append(("every operand subnormal", vals))
    return out


def fused_names(R: int, base_last: bool, replica_last: bool) -> List[str]:
    kinds = ("s", "w", "g") + (("r",) if replica_last else ())
    return ["z"] + (["last"] if base_last else []) + [f"{k}{i}" for i in range(R) for k in kinds]


def fused_scenarios(R: int, base_last: bool, rmom: float, wd: float, rates: Sequence[float], steps: Sequence[bool],
                    alpha: float = ALPHA) -> List[Scenario]:
    """The task steps fused into the barrier: a stepping replica's s is
    overwritten by its w before d = s - z is taken, so its edges enter through
    w_i, g_i and its momentum r_i; a joining replica's through s_i and w_i."""
    names = fused_names(R, base_last, rmom > 0)
    cover = [x for x in ("z", "last", "s0", "w0", "s1", "w1") if x in names]
    out = signed_zeros(names, cover) + sweep(names)
    stepping = [i for i in range(R) if steps[i]]
    joining = [i for i in range(R) if not steps[i]]
    for i in stepping[:2]:
        out += pair_block(f"w{i}", "z")
        out += optimiser_scenarios(-rates[i], rmom, wd, f"w{i}", f"g{i}", f"r{i}" if rmom > 0 else None,
                                   zeros=False)[len(SWEEP) * (3 if rmom > 0 else 2):]
    for i in joining[:1]:
        out += pair_block(f"s{i}", "z") + fma_block(_through(f"s{i}", "z"), f"s{i}-z", f"w{i}", -alpha)
    # nothing here leaves the subnormal range, whoever steps: without it an ordinary gradient swamps
    # every small value of a stepping replica, and a flushed input or output would go unseen
    small = {"z": 0x00200000 | SIGN, "l": 0x00000100, "s": 0x00300000, "w": MAX_SUB, "g": 0x00400000,
             "r": 0x00000100 | SIGN}
    out.append(("every operand subnormal", {x: small[x[0]] for x in names}))
    return out


# ---- writing the scenarios into the buffers ---------------------------------------
def layout(L: int, n: int = N) -> Tuple[int, int]:
    """Where the two copies of a list of ``L`` scenarios start: the second ends
    the buffer (inside the last n mod 1,024 floats), the first lies in the bulk
    at an offset that puts every scenario on another lane of its float4."""
    assert 0 < L <= n % 1024 and L + 8 <= (n // 1024) * 1024, (L, n)
    second = n - L
    first = 5
    while (second - first) % 4 != 1:
        first += 1
    assert first + L <= (n // 1024) * 1024 and second >= (n // 1024) * 1024
    return first, second


def apply(arrays: Dict[str, np.ndarray], scen: Sequence[Scenario], n: int = N) -> List[Optional[str]]:
    """Overwrite, in place, the two copies' elements of the named fp32 arrays.
    Returns the scenario label of every element (None: ordinary data)."""
    labels: List[Optional[str]] = [None] * n
    first, second = layout(len(scen), n)
    views = {}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.size == n and a.flags.c_contiguous, name
        views[name] = a.view(np.uint32)
    for start in (first, second):
        for k, (label, vals) in enumerate(scen):
            for name, v in vals.items():
                views[name][start + k] = v
            labels[start + k] = label
    return labels


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def edge_mismatches(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Indices at which ``got`` misses the edge-value contract against ``want``."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    want_nan = np.isnan(w.view(np.float32))
    got_nan = np.isnan(g.view(np.float32))
    return np.nonzero(np.where(want_nan, ~got_nan, g != w))[0]


def assert_edge_equal(got: np.ndarray, want: np.ndarray, what: str = "",
                      labels: Optional[Sequence[Optional[str]]] = None) -> None:
    """Where ``want`` is NaN, ``got`` is a NaN of any sign and payload;
    everywhere else the 32 bits are equal."""
    bad = edge_mismatches(got, want)
    if bad.size:
        k = int(bad[0])
        g, w = bits(got), bits(want)
        where = f" (scenario: {labels[k] or 'ordinary data'})" if labels is not None else ""
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ; first at {k}{where}: "
                             f"got {g[k]:#010x} ({g.view(np.float32)[k]!r}) want {w[k]:#010x} "
                             f"({w.view(np.float32)[k]!r})")


def is_subnormal(a: np.ndarray) -> np.ndarray:
    b = bits(a)
    return ((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)


def flush(a: np.ndarray) -> None:
    """What a flush-to-zero device makes of ``a``, in place: every subnormal a zero of its sign."""
    b = a.view(np.uint32)
    b[is_subnormal(a)] &= np.uint32(SIGN)


def census(arrays: Sequence[np.ndarray]) -> Dict[str, int]:
    """How many +0, -0, subnormals, +inf, -inf and NaNs the arrays hold."""
    out = dict.fromkeys(("+0", "-0", "subnormal", "+inf", "-inf", "nan"), 0)
    for a in arrays:
        b = bits(a)
        out["+0"] += int(np.sum(b == PZERO))
        out["-0"] += int(np.sum(b == NZERO))
        out["subnormal"] += int(np.sum(is_subnormal(a)))
        out["+inf"] += int(np.sum(b == PINF))
        out["-inf"] += int(np.sum(b == NINF))
        out["nan"] += int(np.sum(np.isnan(b.view(np.float32))))
    return out


# ---- the operations' inputs ---------------------------------------------------------
def sma_case(R: int, momentum: float, alpha: float = ALPHA, scen=None):
    """``oracle.make_state`` at N with the SMA catalogue written in.  Returns
    (state, labels)."""
    from oracle import oracle as O
    st = O.make_state(N, 1, R, alpha, momentum)
    scen = scen if scen is not None else sma_scenarios(R, momentum > 0, alpha)
    return st, apply(_state_arrays(st), scen)


def _state_arrays(st, s=True):
    arrays = {"z": st.z[0]}
    if st.last is not None:
        arrays["last"] = st.last[0]
    for i in range(st.size):
        if s:
            arrays[f"s{i}"] = st.s[i]
        arrays[f"w{i}"] = st.w[i]
    return arrays


def averaging_case(R: int, momentum: float, alpha: float = ALPHA):
    """The same for the elastic-averaging and Polyak-Ruppert barriers at one
    device, which never read s."""
    from oracle import oracle as O
    st = O.make_state(N, 1, R, alpha, momentum)
    return st, apply(_state_arrays(st, s=False), averaging_scenarios(R, momentum > 0))


def optimiser_case(momentum: float, wd: float, rate: float = -LR, seed: int = 300, extra: Sequence[str] = (),
                   last: bool = True, n: int = N):
    """w, g, last (None without momentum) and one array per name in ``extra``
    of ``n`` floats with the task step's catalogue written in, and an s of
    ordinary data that the step overwrites.  Returns (arrays by name, labels)."""
    from oracle import oracle as O
    a = {"w": O.fill_normal(n, seed, 0.05), "g": O.fill_normal(n, seed + 1, 0.01)}
    if momentum > 0 and last:
        a["last"] = O.fill_normal(n, seed + 2, 0.001)
    for k, x in enumerate(extra):
        a[x] = O.fill_normal(n, seed + 4 + k, 0.05 if x == "z" else 0.001)
    labels = apply(a, optimiser_scenarios(rate, momentum, wd, last="last" if "last" in a else None, extra=extra), n)
    a["s"] = O.fill_normal(n, seed + 3, 7.0)
    a.setdefault("last", None)
    return a, labels


def replica_rates(R: int) -> List[float]:
    """A distinct non-zero learning rate per replica, exact in fp32."""
    return [float(np.float32(LR / (1.0 + 0.37 * i))) for i in range(R)]


def fused_case(data, rmom: float, wd: float, rates: Sequence[float], steps: Sequence[bool]):
    """Write the fused catalogue into a ``Data`` of tests/test_gpu_seam_step_and_optimise.py
    (or a ``Case`` of tests/test_gpu_step_and_synchronise.py), in place."""
    st = data.st
    arrays = _state_arrays(st)
    for i in range(st.size):
        arrays[f"g{i}"] = data.g[i]
        if data.last[i] is not None:
            arrays[f"r{i}"] = data.last[i]
    return apply(arrays, fused_scenarios(st.size, st.last is not None, rmom, wd, rates, steps, st.alpha))


def nan_fraction(a: np.ndarray) -> float:
    return float(np.mean(np.isnan(np.ascontiguousarray(a, dtype=np.float32))))


# ---- the reductions: the gradient norm and the model statistics ---------------------------
# Two whole 4,096-float tiles of the norm pass (its unrolled path) and a partial
# one of 225 float4s and 3 floats; a 903-float tail on the seam's TAIL workgroups.
N_RED = 2 * 4096 + 903
assert N_RED % 4 == 3 and N_RED % 1024 == TAIL and (N_RED % 4096) // 4 == 225

ULP = Fraction(1, 2 ** 149)  # every finite float is an integer multiple of it


def to_ints(a: np.ndarray) -> List[Optional[int]]:
    """Every finite float as the integer k of x = k * 2^-149; None for a
    non-finite one."""
    out = []
    for b in bits(a).tolist():
        e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
        if e == 0xFF:
            out.append(None)
            continue
        k = m if e == 0 else (m | 0x800000) << (e - 1)
        out.append(-k if b & SIGN else k)
    return out


def exact_stats(x: Sequence[Optional[int]], xbits: np.ndarray, ref: Optional[Sequence[Optional[int]]] = None):
    """The statistics of ``cbx_buffer_stats`` over the integers of ``to_ints``,
    in exact arithmetic: sum, sum_sq, dist_sq and the sums of their terms'
    magnitudes as Fractions; nonfinite; the bits of max_abs.  A non-finite x
    only counts; a finite x beside a non-finite reference adds to everything
    but dist_sq (against None: x is the reference, dist_sq is 0)."""
    s = sa = q = d = 0
    nf = 0
    for i, k in enumerate(x):
        if k is None:
            nf += 1
            continue
        s += k
        sa += abs(k)
        q += k * k
        if ref is not None and ref[i] is not None:
            d += (k - ref[i]) ** 2
    b = xbits & np.uint32(0x7FFFFFFF)
    b = b[b < PINF]
    return {"sum": s * ULP, "sum_abs": sa * ULP, "sum_sq": q * ULP * ULP, "dist_sq": d * ULP * ULP, "nonfinite": nf,
            "max_abs": int(b.max()) if b.size else 0, "m": len(x)}


EPS53 = Fraction(1, 2 ** 53)


def assert_stats_record(rec, want, exact: bool, what: str) -> None:
    """One ``cbx_buffer_stats`` record against ``exact_stats``: the counts and
    the bits of max_abs always equal; the sums equal (``exact``) or within the
    reordering bound of an fp64 sum of m exact terms, 2 m 2^-53 sum |term|."""
    assert int(rec["nonfinite"]) == want["nonfinite"], (what, int(rec["nonfinite"]), want["nonfinite"])
    got_max = int(np.array([rec["max_abs"]], np.float32).view(np.uint32)[0])
    assert got_max == want["max_abs"], f"{what}: max_abs {got_max:#010x}, want {want['max_abs']:#010x}"
    assert int(rec["reserved"]) == 0, what
    for field, mag in (("sum", "sum_abs"), ("sum_sq", "sum_sq"), ("dist_sq", "dist_sq")):
        v = float(rec[field])
        assert np.isfinite(v), (what, field, v)
        if exact:
            assert Fraction(v) == want[field], f"{what}: {field} = {v!r}, want {float(want[field])!r} exactly"
        else:
            err, bound = abs(Fraction(v) - want[field]), 2 * want["m"] * EPS53 * want[mag]
            assert err <= bound, f"{what}: {field} = {v!r} is {float(err)!r} off, bound {float(bound)!r}"


class Regime:
    """Whole buffers of one kind of value: ``make(n, seed)`` gives an fp32 array."""

    def __init__(self, name, make, exact):
        self.name, self.make, self.exact = name, make, exact

    def __repr__(self):
        return self.name


K_MAX = 2 ** 18


def _scaled_integers(shift):
    def make(n, seed):
        rng = np.random.default_rng(7000 + seed)
        k = rng.integers(-K_MAX, K_MAX + 1, n)
        k[k == 0] = 1
        k[:2] = (K_MAX, -K_MAX)  # the bound of the exactness argument is reached
        return np.ldexp(k.astype(np.float64), shift).astype(np.float32)
    return make


def _uniform_power(e):
    def make(n, seed):
        rng = np.random.default_rng(7100 + seed)
        sign = np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)
        return np.ldexp(sign, e).astype(np.float32)
    return make


def _range_end(n, seed):
    rng = np.random.default_rng(7200 + seed)
    b = (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)) | \
        (rng.integers(253, 255, n).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 2 ** 23, n).astype(np.uint32)
    b[:2] = (FLT_MAX, FLT_MAX | SIGN)
    return b.view(np.float32)


# x = k 2^-149 (subnormals: their squares underflow in fp32) and k 2^104 (their
# squares overflow in fp32), |k| <= 2^18: n k^2 and n (k - k_ref)^2 stay below
# 2^53, so the three sums are exact in fp64 in any order.  The same for +-2^e.
REGIMES = (Regime("subnormal", _scaled_integers(-149), True), Regime("mid-range", _scaled_integers(104), True),
           Regime("min-sub", _uniform_power(-149), True), Regime("FLT_MIN", _uniform_power(-126), True),
           Regime("2^127", _uniform_power(127), True), Regime("range-end", _range_end, False))


def reduction_catalogue() -> List[Scenario]:
    """The wide catalogue of the reductions over the pair (x, ref): every entry
    of SWEEP in each, the signed zeros, and the pairs that the masks of
    ``cbx_buffer_stats`` tell apart.  In groups of three that a run of 3-float
    variables keeps together: the huge values share no variable with a mask
    pair, so that pair's record has a bound with teeth."""
    h, t = b32(0.75), b32(-0.3125)
    out = sweep(["x"]) + [("x=-FLT_MAX again", {"x": FLT_MAX | SIGN}), ("x=0.75", {"x": h})]
    out += sweep(["ref"]) + [("ref=-0.3125", {"ref": t}), ("ref=0.75", {"ref": h})]
    out += signed_zeros(["x", "ref"]) + [("x=ref=-0", {"x": NZERO, "ref": NZERO}), ("x=-0 again", {"x": NZERO})]
    out += [("x=+inf beside a finite ref", {"x": PINF, "ref": h}), ("x finite beside ref=+inf", {"x": h, "ref": PINF}),
            ("x=snan beside a finite ref", {"x": SNAN, "ref": t}),
            ("x finite beside ref=payload-nan", {"x": t, "ref": PAYLOAD_NAN}),
            ("x finite beside ref=-inf", {"x": t, "ref": NINF}), ("x == ref", {"x": h, "ref": h}),
            ("x=+min-sub ref=-min-sub", {"x": MIN_SUB, "ref": MIN_SUB | SIGN}),
            ("x=-min-sub ref=+min-sub", {"x": MIN_SUB | SIGN, "ref": MIN_SUB}),
            ("x == ref, both max-sub", {"x": MAX_SUB, "ref": MAX_SUB}),
            ("x=+FLT_MAX ref=-FLT_MAX", {"x": FLT_MAX, "ref": FLT_MAX | SIGN}),
            ("x=-FLT_MAX ref=+FLT_MAX", {"x": FLT_MAX | SIGN, "ref": FLT_MAX}),
            ("x == ref, both FLT_MAX", {"x": FLT_MAX, "ref": FLT_MAX}),
            ("every x of a variable NaN: 1", {"x": QNAN}), ("every x of a variable NaN: 2", {"x": PAYLOAD_NAN}),
            ("every x of a variable NaN: 3", {"x": SNAN}),
            ("every x of a variable -0: 1", {"x": NZERO}), ("every x of a variable -0: 2", {"x": NZERO, "ref": NZERO}),
            ("every x of a variable -0: 3", {"x": NZERO, "ref": PINF})]
    assert len(out) % 3 == 0
    return out


def stats_variables(L: int, n: int = N_RED) -> Tuple[Tuple[int, ...], int, int]:
    """The statistics tests' variable list for catalogues of up to ``L``
    entries, and where the two copies start: one float (every later variable
    starts off a float4), a large variable that holds the first copy on the
    aligned float4 path, ceil(L/3) variables of 3 floats whose every float
    takes the scalar path and which hold the second copy, and the remainder."""
    run = -(-L // 3)
    big = 4600
    variables = (1, big) + (3,) * run + (n - 1 - big - 3 * run,)
    assert variables[-1] > 0 and sum(variables) == n
    second = 1 + big
    first = 8
    while (second - first) % 4 != 1:
        first += 1
    return variables, first, second


def stats_pieces(variables: Sequence[int], tile: int = 4096) -> List[Tuple[int, int, int, bool]]:
    """The piece table of crossbow_amd/csrc/stats_plan.h restated: (lo, hi,
    variable, aligned) in offset order."""
    out, lo = [], 0
    for v, count in enumerate(variables):
        hi = lo + count
        a = lo
        while a < hi:
            b = min((a // tile + 1) * tile, hi)
            a4, b4 = (a + 3) // 4 * 4, b // 4 * 4
            cut = [(a, a4, False), (a4, b4, True), (b4, b, False)] if a4 < b4 else [(a, b, False)]
            out += [(x, y, v, al) for x, y, al in cut if x < y]
            a = b
        lo = hi
    return out


def apply_at(arrays: Dict[str, np.ndarray], scen: Sequence[Scenario], starts: Sequence[int]) -> List[Optional[str]]:
    """``apply`` with the copies' start offsets given (the statistics tests'
    second copy lies in the scalar run, not at the buffer's end)."""
    n = next(iter(arrays.values())).size
    labels: List[Optional[str]] = [None] * n
    views = {}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.size == n and a.flags.c_contiguous, name
        views[name] = a.view(np.uint32)
    for start in starts:
        assert 0 <= start and start + len(scen) <= n
        for k, (label, vals) in enumerate(scen):
            assert labels[start + k] is None, "the copies overlap"
            for name, v in vals.items():
                views[name][start + k] = v
            labels[start + k] = label
    return labels


def finite_gradient(a: Dict[str, Optional[np.ndarray]], seed: int = 900) -> Dict[str, Optional[np.ndarray]]:
    """The finite-g form of an ``optimiser_case``: every non-finite g is replaced
    by ordinary data; w and last keep theirs."""
    from oracle import oracle as O
    out = {k: (v.copy() if v is not None else None) for k, v in a.items()}
    bad = ~np.isfinite(out["g"])
    out["g"][bad] = O.fill_normal(out["g"].size, seed, 0.01)[bad]
    return out
