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


# ---- a context and its replica buffers (the GPU tests) ---------------------------------------
def context(n, momentum, wd, replicas=1, update_type=7, variables=None, mults=None, alpha=0.1):
    """A context of one device for the replica step (SMA by default), the learning rate fixed at LR."""
    from crossbow_amd import TheGPU
    variables = variables or [n]
    g = TheGPU()
    g.init([0])
    g.setModel(len(variables), 4 * n)
    for v, count in enumerate(variables):
        g.setModelVariable(v, 1, [count], 4 * count)
        if mults is not None:
            g.setModelVariableLearningRateMultiplier(v, 1, mults[v])
    g.setUpdateModelType(update_type)
    g.setEamsgdAlpha(alpha)
    g.setMomentum(momentum, 0)
    g.setWeightDecay(wd)
    g.setLearningRateDecayPolicyFixed(LR)
    g.setModelManager(replicas, 0)
    return g


def put(gpu, i, bufs):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    for kind, a in zip((BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF), bufs):
        if a is not None:
            gpu.replica_write(i, kind, a)


def get(gpu, i, momentum):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    return [gpu.replica_read(i, kind) if (kind != BUF_LAST or momentum > 0) else None
            for kind in (BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF)]


# ---- the CLIP step kernels on IEEE edge values ---------------------------------------------
def clipped_inputs(momentum, wd, finite, seed=300):
    """``E.optimiser_case`` at ``E.N_RED``, as is (g holds infinities and NaNs:
    K > 0) or in its finite-g form (K = 0, NaNs in w and last only), with a
    max_norm of a fifth of the exact norm: the step clips by a scale near 0.2,
    no power of two.  Returns (arrays, labels, S, K, c)."""
    from tests import edge_values as E
    a, labels = E.optimiser_case(momentum, wd, np.float32(-LR), seed=seed, n=E.N_RED)
    if finite:
        a = E.finite_gradient(a)
    S, K = exact_sum_sq(a["g"])
    c = float(np.float32(0.2 * math.sqrt(S)))
    assert 0 < c < float(np.finfo(np.float32).max) and (K == 0) == bool(finite)
    return a, labels, S, K, c


def clipped_expectation(a, S, K, c, skip, momentum, wd, variables=None, mults=None):
    """The oracle's outputs for ``clipped_inputs`` from a sum of squares ``S``
    (the exact one, or the device's once it has passed its own check).
    Returns (outputs by name, scale, flags); the inputs are left alone."""
    out = {k: (v.copy() if v is not None else None) for k, v in a.items()}
    scale, flags = decide(S, K, c, skip)
    bufs = [out["w"], out["g"], out["last"], out["s"]]
    step(bufs, scale, flags, momentum, wd, variables=variables, mults=mults)
    return out, scale, flags


# ---- the decision and the scale on exact sums (tests/test_reduction_edges.py) ------------
N_DECIDE = 8  # floats of the gradients below


def squares(S: int):
    """Integers below 2^23 whose squares sum to S, greedily: the largest square
    first.  Every square and every partial sum is exact in fp64 (S < 2^46), in
    any order."""
    out, r = [], int(S)
    assert 0 <= r < 2 ** 46
    while r:
        k = math.isqrt(r)
        out.append(k)
        r -= k * k
    return out


def gradient_of(S: int, n: int = N_DECIDE, flip: int = 0b10100101):
    """n floats (mixed signs, zeros of both signs behind them) whose squares
    sum to the integer S exactly."""
    ks = squares(S)
    assert len(ks) <= n and all(k < 2 ** 23 for k in ks), (S, ks)
    g = np.zeros(n, np.float32)
    g[:len(ks)] = ks
    sign = np.array([-1.0 if (flip >> i) & 1 else 1.0 for i in range(n)], np.float32)
    g *= sign  # a zero takes the sign too: -0
    assert sum(int(x) ** 2 for x in g.tolist()) == S
    return g


def scale_bits(c_bits: int, S: int) -> int:
    """The header's sequence (float)((double)c / sqrt((double)S)) with Python's
    correctly rounded sqrt and divide; the bits of the float."""
    c = float(np.array([c_bits], np.uint32).view(np.float32)[0])
    return int(np.array([c / math.sqrt(float(S))], np.float64).astype(np.float32).view(np.uint32)[0])


def midpoint_distance(c_bits: int, S: int):
    """How far, in ulps of the double, c / sqrt(S) as IEEE double evaluates it
    lies from the nearest midpoint of two adjacent floats: an exact integer."""
    c = float(np.array([c_bits], np.uint32).view(np.float32)[0])
    q = c / math.sqrt(float(S))
    low = int(np.array([q], np.float64).view(np.uint64)[0]) & (2 ** 29 - 1)
    assert 2.0 ** -126 <= q < 2.0 ** 127  # a normal float: 29 bits of the double are rounded away
    return low - 2 ** 28


def nudge_moves(c_bits: int, S: int):
    """(down, up): whether a quotient 1 double ulp lower, or higher, rounds to
    another float than the header's."""
    q = _f32(c_bits) / math.sqrt(float(S))
    want = np.float32(q)
    return tuple(bool(np.float32(np.nextafter(q, d)) != want) for d in (0.0, math.inf))


def search_hard_cases(seed: int, trials: int, chunk: int = 1 << 22):
    """Pairs (c, S) for which c / sqrt(S) in IEEE double lies within 1 double
    ulp of the midpoint of two adjacent floats: a sqrt or a divide 1 ulp off
    there moves the float.  c = a float-exact multiple of 2^-10 in [2^13, 2^14),
    S an integer in [2^20, 2^44) that ``squares`` splits into at most N_DECIDE
    terms.  About 7 hits per 10^9 trials, two in five of them exact ties (40 and 17 in
    the 5.6 * 10^9 trials behind HARD_CASES).  Returns
    [(bits of c, S, distance)]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range((trials + chunk - 1) // chunk):
        m = rng.integers(2 ** 23, 2 ** 24, chunk, dtype=np.int64)
        S = rng.integers(2 ** 20, 2 ** 44, chunk, dtype=np.int64)
        q = (m.astype(np.float64) * 2.0 ** -10) / np.sqrt(S.astype(np.float64))
        d = (q.view(np.uint64) & np.uint64(2 ** 29 - 1)).astype(np.int64) - 2 ** 28
        for k in np.nonzero(np.abs(d) <= 1)[0]:
            if len(squares(int(S[k]))) <= N_DECIDE:
                c_bits = int(np.array([float(m[k]) * 2.0 ** -10], np.float32).view(np.uint32)[0])
                out.append((c_bits, int(S[k]), int(d[k])))
    return out


# search_hard_cases(seed, 7 * 10^8) for seeds 1..8, in that order (5.6 * 10^9 trials, about
# six minutes on one core); not run at test time.  Every S exceeds c^2: the step clips.
HARD_CASES = (
    (0x465e721e, 17418051655997, 0), (0x46260e65, 1688547107531, 0),
    (0x4629ebed, 4785959415988, 1), (0x46782d4e, 10155753545070, 1), (0x464d49bc, 9948760735551, 0),
    (0x4635e9d3, 715503587311, 1), (0x4614eb4a, 9748546494373, 0), (0x4670aae8, 7214694657074, -1),
    (0x461e015e, 11626809888591, -1),
    (0x4670eb7a, 366762188752, -1), (0x466109fa, 6262014242649, 1), (0x4604c0bf, 1556738165937, -1),
    (0x46745700, 6721126724876, 0), (0x4614532c, 4264446443209, 0), (0x467d9f63, 13980567519474, 0),
    (0x462ac8de, 7390748368940, 0),
    (0x46516cfc, 5358083468343, 1), (0x465cb677, 5598028502292, 0), (0x4669c460, 7368826638695, 1),
    (0x46019911, 1449958605729, -1), (0x460e08fc, 10733280938838, -1), (0x4615ec04, 3088737324885, 0),
    (0x4635800a, 5577372580641, -1), (0x4636805a, 16664463281810, 0),
    (0x46697689, 13808940052312, 1), (0x46422e72, 5150419544383, -1), (0x4633f80f, 14713869723343, 0),
    (0x460bf5e5, 10618099756566, 1), (0x465ed0da, 12453563150578, 1), (0x46719124, 12403513465283, 0),
    (0x465c206f, 2384710744949, 0),
    (0x465c84de, 10541705691739, 1), (0x4614a808, 14944772851434, 1), (0x465767b5, 4706610209719, 0),
    (0x46532a59, 2507971353059, 0), (0x46587aad, 11502390420439, 1), (0x464de4e0, 7661135246638, 1),
    (0x4604f441, 11367868826418, 1),
    (0x466f2525, 1362627036558, 1), (0x4655266e, 12115105560226, 0),
)


def _f32_bits(x) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _f32(b: int) -> float:
    return float(np.array([b], np.uint32).view(np.float32)[0])


def decision_table(seed: int = 4242, random_pairs: int = 256):
    """[(label, bits of c, S)]: the boundaries of the decision S > c^2 and of
    the scale, then seeded random pairs.  ``gradient_of(S)`` yields S exactly."""
    c = 4096.0
    S_near = 3 * 2 ** 30 + 12345  # not a square: sqrt(S) lies strictly between two floats
    root = math.sqrt(S_near)
    below = float(np.nextafter(np.float32(root), np.float32(0))) if float(np.float32(root)) > root \
        else float(np.float32(root))
    assert below * below < S_near < float(np.nextafter(np.float32(below), np.float32(np.inf))) ** 2
    rows = [
        ("S == c^2: not clipped, scale 1", _f32_bits(c), int(c * c)),
        ("S == c^2 for an odd c", _f32_bits(4097.0), 4097 ** 2),
        ("S = c^2 - 1: not clipped", _f32_bits(c), int(c * c) - 1),
        ("S = c^2 + 1: clipped, the scale rounds to 1.0f", _f32_bits(c), int(c * c) + 1),
        ("c one float below sqrt(S)", _f32_bits(below), S_near),
        ("c one float above sqrt(S): not clipped", _f32_bits(np.nextafter(np.float32(below), np.float32(np.inf))),
         S_near),
        ("c = 0: clipping is off", 0, 12345),
        ("S = 0 from zeros of both signs", _f32_bits(c), 0),
        ("S = 0 and c = 0", 0, 0),
        ("c subnormal under an integer S", 0x00000001, 1),
        ("c = FLT_MAX: c^2 needs the double's range", 0x7F7FFFFF, 2 ** 45),
    ]
    rng = np.random.default_rng(seed)
    for k in range(random_pairs):
        while True:
            S = int(rng.integers(1, 2 ** 44)) >> int(rng.integers(0, 40))
            if len(squares(S)) <= N_DECIDE:
                break
        # a c of either side of sqrt(S), within a factor of 4, with a full mantissa
        cb = _f32_bits(math.sqrt(S) * 2.0 ** float(rng.uniform(-2, 2)))
        rows.append((f"random pair {k}", cb, max(S, 1)))
    return rows


if __name__ == "__main__":  # python -m tests.gradient_clip_common SEED TRIALS: prints rows of HARD_CASES
    import sys
    for row in search_hard_cases(int(sys.argv[1]), int(float(sys.argv[2]))):
        print("    (0x%08x, %d, %d)," % row, flush=True)
