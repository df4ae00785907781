"""Every step kernel against the oracle on IEEE edge values (run with -m gpu).

The inputs are ``oracle.fill_normal`` data with the scenarios of
tests/edge_values.py written in twice, at one small size (``E.N``): signed
zeros, subnormals, the ends of the fp32 range, infinities, NaNs, exact
cancellations, an fma tie.  tests/test_edge_values.py pins those inputs on the
CPU.  The expectation is the oracle (or tests/averaging_common.py) on the same
arrays, compared by DESIGN.md's edge-value contract:

* arithmetic outputs by ``E.assert_edge_equal``: where the reference is NaN the
  device is NaN, everywhere else the 32 bits are equal;
* what is a copy in the reference, bit for bit with NaN payloads
  (``assert_bitexact``): s after a task step, every buffer a call must leave
  alone, the sentinels behind caller-owned buffers, and after Phase D or a
  broadcast each w_i against the device's own new z.

alpha is 0.1, replica momentum 0.9 or off, weight decay 5e-4 or off, the
learning rates non-zero and distinct per replica: no scalar is an exact 0
unless its term is switched off as a whole (the alpha = 0 note).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import edge_values as E
from tests.helpers import assert_bitexact, make_gpu, upload
from tests.test_gpu_seam_step_and_optimise import CONFIGS as FUSED_CONFIGS
from tests.test_gpu_seam_step_and_optimise import DISCARD, Data, Guarded

pytestmark = pytest.mark.gpu

N, ALPHA, LR, WD = E.N, E.ALPHA, E.LR, E.WD
OPT_CONFIGS = E.OPT_CONFIGS


def _has(a, pattern):
    return bool(np.any(E.bits(a) == pattern))


def _check_guarded(gd: Guarded, want, name, labels, strict=False):
    host = gd.t.cpu().numpy()
    if strict:
        assert_bitexact(host[:gd.n], want, name)
    else:
        E.assert_edge_equal(host[:gd.n], want, name, labels)
    assert_bitexact(host[gd.n:], gd.sentinel, f"the floats behind {name}")
    return host[:gd.n]


# ---- A. the SMA barrier on a context ---------------------------------------------
def _read_state(g, R, last):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_LAST
    return (g.base_read(0, BUF_DATA), g.base_read(0, BUF_LAST) if last else None,
            [g.replica_read(i, BUF_DIFF) for i in range(R)], [g.replica_read(i, BUF_DATA) for i in range(R)])


def _compare_sma(got, before, want, labels, copied, what=""):
    """got = (z, last, s, w) read back; `copied`: the replicas that took z."""
    z, last, s, w = got
    E.assert_edge_equal(z, want.z[0], f"{what}z", labels)
    if want.last is not None:
        E.assert_edge_equal(last, want.last[0], f"{what}base last", labels)
    for i in range(want.size):
        E.assert_edge_equal(w[i], want.w[i], f"{what}w[{i}]", labels)
        assert_bitexact(s[i], before.s[i], f"{what}s[{i}] is not written")
        if i in copied:
            assert_bitexact(w[i], z, f"{what}w[{i}] is a copy of the device's z")


def _context_sma(R, momentum, copy, split=False, algo=0, config=None):
    st, labels = E.sma_case(R, momentum)
    g = make_gpu(N, R, ALPHA, momentum)
    try:
        if config:
            g.set_kernel_config(**config)
        if split:
            g.set_force_split(True)
        if algo:
            g.set_allreduce_algorithm(algo)
        upload(g, st)
        want = st.clone()
        if copy:
            g.set_replica_copy(1, True)
            want.copy[1] = 1
        assert g.lockAny() == R
        g.synchronise(0, 1, 0, False)
        g.unlockAny()
        g.wait()
        assert (O.sma_step(want) > 0) == copy
        _compare_sma(_read_state(g, R, momentum > 0), st, want, labels, range(R) if copy else ())
    finally:
        g.free()


@pytest.mark.parametrize("copy", [False, True], ids=["no-copy", "copy"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [3, 9], ids=["unrolled-3", "chunked-9"])
def test_sma_barrier_fused(R, momentum, copy):
    _context_sma(R, momentum, copy)


@pytest.mark.parametrize("copy", [False, True], ids=["no-copy", "copy"])
@pytest.mark.parametrize("algo", [0, 2], ids=["all-reduce", "reduce-scatter"])
def test_sma_barrier_split(algo, copy):
    from crossbow_amd._lib import ALLREDUCE_RSAG
    assert ALLREDUCE_RSAG == 2
    _context_sma(3, 0.9, copy, split=True, algo=algo)


def test_sma_barrier_fused_plain_loads_no_unroll():
    _context_sma(3, 0.9, True, config=dict(policy=0, unroll=1))


# ---- B. the same barrier through the seam ----------------------------------------
@pytest.mark.parametrize("copy", [False, True], ids=["no-copy", "copy"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [3, 9], ids=["unrolled-3", "chunked-9"])
def test_seam_sma_step(R, momentum, copy):
    import torch

    from crossbow_amd.seam import SmaPlan
    st, labels = E.sma_case(R, momentum)
    if copy:
        st.copy[1] = 1
    want = st.clone()
    z = Guarded(st.z[0], 1)
    last = Guarded(st.last[0], 2) if momentum > 0 else None
    w = [Guarded(a, 10 + i) for i, a in enumerate(st.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(st.s)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        got = plan.step([stream.cuda_stream], [z.ptr], [last.ptr] if last else None,
                        [(0, w[i].ptr, s[i].ptr, 1, int(st.copy[i])) for i in range(R)], ALPHA, momentum)
        stream.synchronize()
    assert got == (1 if O.sma_step(want) > 0 else 0) == int(copy)
    zd = _check_guarded(z, want.z[0], "z", labels)
    if last:
        _check_guarded(last, want.last[0], "base last", labels)
    for i in range(R):
        wd = _check_guarded(w[i], want.w[i], f"w[{i}]", labels)
        _check_guarded(s[i], st.s[i], f"s[{i}] is not written", labels, strict=True)
        if copy:
            assert_bitexact(wd, zd, f"w[{i}] is a copy of the device's z")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_seam_ssgd_step(momentum):
    import torch

    from crossbow_amd.seam import SmaPlan
    R, wpc = 3, 6
    st = O.make_state(N, 1, R, ALPHA, momentum)
    acc0 = O.fill_normal(N, 777, 0.01)
    arrays = {"z": st.z[0], "acc": acc0}
    if momentum > 0:
        arrays["last"] = st.last[0]
    labels = E.apply(arrays, E.ssgd_sync_scenarios(momentum > 0, wpc))
    st.locked[2] = 0  # a held replica keeps its weights
    want = st.clone()
    z = Guarded(st.z[0], 1)
    last = Guarded(st.last[0], 2) if momentum > 0 else None
    acc = Guarded(acc0, 3)
    w = [Guarded(a, 10 + i) for i, a in enumerate(st.w)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        plan.ssgd_step([stream.cuda_stream], [z.ptr], [last.ptr] if last else None, [acc.ptr],
                       [(0, w[i].ptr, int(st.locked[i])) for i in range(R)], momentum, wpc)
        stream.synchronize()
    O.ssgd_sync(want, [acc0], wpc)
    zd = _check_guarded(z, want.z[0], "z", labels)
    if last:
        _check_guarded(last, want.last[0], "base last", labels)
    _check_guarded(acc, np.zeros(N, np.float32), "acc is reset to +0", labels, strict=True)
    for i in (0, 1):
        assert_bitexact(_check_guarded(w[i], want.w[i], f"w[{i}]", labels), zd, f"w[{i}] is a copy of the device's z")
    _check_guarded(w[2], st.w[2], "w[2] is held", labels, strict=True)


# ---- C. the replica optimiser step -----------------------------------------------
def _optimiser_context(momentum, wd, policy=None, update_type=7, wpc=None, R=2):
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(1, 4 * N)
    g.setModelVariable(0, 1, [N], 4 * N)
    if wpc:
        g.setModelWorkPerClock(wpc)
    g.setUpdateModelType(update_type)
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, 0)
    g.setWeightDecay(wd)
    if policy == "exp":
        g.setLearningRateDecayPolicyExp(LR, 0.97)
    else:
        g.setLearningRateDecayPolicyFixed(LR)
    g.setModelManager(R, 0)
    return g


def _check_optimise(read, a0, want, labels, momentum, wd, what):
    """`read(name)` gives the device's w, g, last or s; a0 the inputs, want the oracle's outputs."""
    w_in = a0["w"]
    assert _has(w_in, E.SNAN) and _has(w_in, E.PAYLOAD_NAN)
    E.assert_edge_equal(read("w"), want["w"], f"{what}w", labels)
    assert_bitexact(read("s"), w_in, f"{what}s is a copy of the old w, signalling NaNs included")
    assert_bitexact(want["s"], w_in, "the oracle's s")
    if momentum > 0:
        E.assert_edge_equal(read("last"), want["last"], f"{what}last", labels)
    if momentum > 0 or wd > 0:
        E.assert_edge_equal(read("g"), want["g"], f"{what}g", labels)
    else:
        assert_bitexact(read("g"), a0["g"], f"{what}g is not written")


@pytest.mark.parametrize("config", list(OPT_CONFIGS))
def test_replica_optimise_context(config):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    momentum, wd = OPT_CONFIGS[config]
    kinds = {"w": BUF_DATA, "g": BUF_GRADIENT, "last": BUF_LAST, "s": BUF_DIFF}
    R, tasks = 2, [3, 8]
    twin = _optimiser_context(momentum, 0.0, "exp")  # asked for the rates only: the query may change host state
    try:
        rates = [twin.replica_learning_rate(i, tasks[i]) for i in range(R)]
    finally:
        twin.free()
    assert len(set(rates)) == R and all(r > 0 for r in rates)
    g = _optimiser_context(momentum, wd, "exp")
    try:
        for i in range(R):
            rate = np.float32(-rates[i])
            a, labels = E.optimiser_case(momentum, wd, rate, seed=300 + 10 * i)
            a0 = {k: (v.copy() if v is not None else None) for k, v in a.items()}
            for name, kind in kinds.items():
                if a[name] is not None:
                    g.replica_write(i, kind, a[name])
            g.replica_optimise(i, tasks[i])
            g.wait()
            O.sma_optimise(rate, momentum, wd, a["w"], a["g"], a["last"], a["s"])
            _check_optimise(lambda name: g.replica_read(i, kinds[name]), a0, a, labels, momentum, wd, f"replica {i} ")
    finally:
        g.free()


@pytest.mark.parametrize("config", list(OPT_CONFIGS))
def test_optimise_buffers_seam(config):
    import torch

    from crossbow_amd.seam import optimise_buffers
    momentum, wd = OPT_CONFIGS[config]
    stream = torch.cuda.Stream()
    for i, lr in enumerate(E.replica_rates(2)):
        rate = np.float32(-lr)
        a, labels = E.optimiser_case(momentum, wd, rate, seed=300 + 10 * i)
        a0 = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        dev = {k: Guarded(v, 20 + j) for j, (k, v) in enumerate(a.items()) if v is not None}
        torch.cuda.synchronize()
        optimise_buffers(stream.cuda_stream, dev["w"].ptr, dev["g"].ptr, dev["last"].ptr if momentum > 0 else None,
                         dev["s"].ptr, N, lr, momentum, wd)
        stream.synchronize()
        O.sma_optimise(rate, momentum, wd, a["w"], a["g"], a["last"], a["s"])
        _check_optimise(lambda name: dev[name].t.cpu().numpy()[:N], a0, a, labels, momentum, wd, f"rate {lr} ")
        for name, gd in dev.items():
            assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {name}")


# ---- D. per-variable rates ----------------------------------------------------------
# the middle variable holds the whole first copy of the scenarios and starts and ends off a float4
VARS = (3, 1500, N - 1503)
MULTS = (1.0, 0.5, 2.0)
VAR_CONFIGS = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0)}


def _variable_case(momentum, wd, only=None):
    from tests.test_optimise_plan import per_variable_step
    a, labels = E.optimiser_case(momentum, wd, np.float32(-LR), seed=340)
    a0 = {k: (v.copy() if v is not None else None) for k, v in a.items()}
    per_variable_step(LR, MULTS, momentum, wd, a["w"], a["g"], a["last"], a["s"], variables=VARS, only=only)
    return a0, a, labels


def _check_variables(read, a0, want, labels, momentum, wd, only):
    lo = 0
    for v, count in enumerate(VARS):
        sl = slice(lo, lo + count)
        lo += count
        stepped = only is None or v in only
        for name in ("w", "g", "last", "s"):
            if a0[name] is None:
                continue
            got = read(name)[sl]
            what = f"variable {v} {name}"
            if not stepped:
                assert_bitexact(got, a0[name][sl], f"{what} is not stepped")
            elif name == "s":
                assert_bitexact(got, a0["w"][sl], f"{what} is a copy of the old w")
            elif name == "g" and momentum == 0 and wd == 0:
                assert_bitexact(got, a0["g"][sl], f"{what} is not written")
            else:
                E.assert_edge_equal(got, want[name][sl], what, labels[sl])


def _variable_context(momentum, wd):
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(len(VARS), 4 * N)
    for v, count in enumerate(VARS):
        g.setModelVariable(v, 1, [count], 4 * count)
        g.setModelVariableLearningRateMultiplier(v, 1, MULTS[v])
    g.setUpdateModelType(7)
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, 0)
    g.setWeightDecay(wd)
    g.setLearningRateDecayPolicyFixed(LR)
    g.setModelManager(1, 0)
    return g


@pytest.mark.parametrize("door", ["whole-model", "middle-operator"])
@pytest.mark.parametrize("config", list(VAR_CONFIGS))
def test_variable_rates_context(config, door):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    momentum, wd = VAR_CONFIGS[config]
    kinds = {"w": BUF_DATA, "g": BUF_GRADIENT, "last": BUF_LAST, "s": BUF_DIFF}
    only = None if door == "whole-model" else {1}
    a0, want, labels = _variable_case(momentum, wd, only)
    g = _variable_context(momentum, wd)
    try:
        for name, kind in kinds.items():
            if a0[name] is not None:
                g.replica_write(0, kind, a0[name])
        if only is None:
            g.set_variable_learning_rates(True)
            g.replica_optimise(0, task=0)
        else:
            g.replica_optimise_variables(0, task=0, op=1)
        g.wait()
        _check_variables(lambda name: g.replica_read(0, kinds[name]), a0, want, labels, momentum, wd, only)
    finally:
        g.free()


@pytest.mark.parametrize("door", ["whole-range", "middle-variable"])
@pytest.mark.parametrize("config", list(VAR_CONFIGS))
def test_variable_rates_seam(config, door):
    import torch

    from crossbow_amd.seam import SmaPlan
    momentum, wd = VAR_CONFIGS[config]
    only = None if door == "whole-range" else {1}
    a0, want, labels = _variable_case(momentum, wd, only)
    dev = {k: Guarded(v, 30 + j) for j, (k, v) in enumerate(a0.items()) if v is not None}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        plan.set_variables(VARS, MULTS)
        first, count = (0, len(VARS)) if only is None else (1, 1)
        plan.optimise_variables(0, stream.cuda_stream, dev["w"].ptr, dev["g"].ptr,
                                dev["last"].ptr if momentum > 0 else None, dev["s"].ptr, LR, momentum, wd, first, count)
        stream.synchronize()
    _check_variables(lambda name: dev[name].t.cpu().numpy()[:N], a0, want, labels, momentum, wd, only)
    for name, gd in dev.items():
        assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {name}")


# ---- E. the task steps fused into the barrier -----------------------------------------
MASKS = {"all-step-R3": (3, None), "mixed-mask-R9": (9, (0, 3, 8))}


def _check_fused(read, d, d0, labels, steps, rmom, wd, keep, copied, what=""):
    """`read(kind, i)`: the device's buffer (kind in z, blast, w, s, g, r); d the
    mirror after the oracle's step, d0 before it."""
    st = d.st
    z = read("z", 0)
    E.assert_edge_equal(z, st.z[0], f"{what}z", labels)
    if st.last is not None:
        E.assert_edge_equal(read("blast", 0), st.last[0], f"{what}base last", labels)
    for i in range(st.size):
        w = read("w", i)
        E.assert_edge_equal(w, st.w[i], f"{what}w[{i}]", labels)
        if copied:
            assert_bitexact(w, z, f"{what}w[{i}] is a copy of the device's z")
        if steps[i] and keep:
            assert_bitexact(read("s", i), d0.st.w[i], f"{what}s[{i}] is a copy of the old w")
            assert_bitexact(st.s[i], d0.st.w[i], "the oracle's s")
        else:
            assert_bitexact(read("s", i), d0.st.s[i], f"{what}s[{i}] is not written")
        if steps[i] and keep and (rmom > 0 or wd > 0):
            E.assert_edge_equal(read("g", i), d.g[i], f"{what}g[{i}]", labels)
        else:
            assert_bitexact(read("g", i), d0.g[i], f"{what}g[{i}] is not written")
        if d.last[i] is not None:
            if steps[i]:
                E.assert_edge_equal(read("r", i), d.last[i], f"{what}last[{i}]", labels)
            else:
                assert_bitexact(read("r", i), d0.last[i], f"{what}last[{i}] is not written")


def _fused_data(R, rmom, wd, bmom, rates, steps):
    d = Data(N, R, rmom, bmom)
    labels = E.fused_case(d, rmom, wd, rates, steps)
    d0 = Data(N, R, rmom, bmom)
    E.fused_case(d0, rmom, wd, rates, steps)
    return d, d0, labels


def _seam_fused(config, flags, mask, copy=False):
    import torch

    from crossbow_amd.seam import SmaPlan
    from tests.test_gpu_seam_step_and_optimise import Buffers
    rmom, wd, bmom = FUSED_CONFIGS[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    rates = E.replica_rates(R)
    d, d0, labels = _fused_data(R, rmom, wd, bmom, rates, steps)
    if copy:
        d.st.copy[1] = 1
    buf = Buffers(d)
    with SmaPlan([0], N) as plan:
        got = buf.call(plan, steps, rates, wd, flags)
        buf.stream.synchronize()
    assert got == d.step(steps, rates, wd, keep=flags == 0) == int(copy)
    torch.cuda.synchronize()
    table = {"z": [buf.z], "blast": [buf.blast], "w": buf.w, "s": buf.s, "g": buf.g, "r": buf.last}
    _check_fused(lambda kind, i: table[kind][i].t.cpu().numpy()[:N], d, d0, labels, steps, rmom, wd, flags == 0, copy)
    for kind, gds in table.items():
        for i, gd in enumerate(gds):
            if gd is not None:
                assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {kind}[{i}]")


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(FUSED_CONFIGS))
def test_step_and_optimise_seam(config, mask, flags):
    _seam_fused(config, flags, mask)


def test_step_and_optimise_seam_with_a_copy_request():
    _seam_fused("mom-wd", 0, "all-step-R3", copy=True)


# One momentum serves the base model and the replicas of a context: the seam's
# "base-mom-only" (replica momentum off, base momentum on) has no context form, so
# the context runs weight decay alone in its place.
CONTEXT_FUSED = {"mom-wd": (0.9, WD), "plain": (0.0, 0.0), "wd-only": (0.0, WD)}


def _context_fused(config, flags, mask, copy=False):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    from tests.test_gpu_step_and_synchronise import _exp, _gpu, _rates
    momentum, wd = CONTEXT_FUSED[config]
    R, who = MASKS[mask]
    steps = [who is None or i in who for i in range(R)]
    tasks = [3 + 2 * i if steps[i] else -1 for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    assert len({r for r, s in zip(rates, steps) if s}) == sum(steps) and all(r > 0 for r, s in zip(rates, steps) if s)
    d, d0, labels = _fused_data(R, momentum, wd, momentum, rates, steps)
    gpu = _gpu(N, R, momentum, wd, _exp)
    try:
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            if d.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, d.last[i])
        if copy:
            gpu.set_replica_copy(1, True)
            d.st.copy[1] = 1
        assert gpu.lockAny() == R
        gpu.step_and_synchronise(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        assert d.step(steps, rates, wd, keep=flags == 0) == int(copy)
        kinds = {"w": BUF_DATA, "s": BUF_DIFF, "g": BUF_GRADIENT, "r": BUF_LAST}

        def read(kind, i):
            if kind in ("z", "blast"):
                return gpu.base_read(0, BUF_DATA if kind == "z" else BUF_LAST)
            return gpu.replica_read(i, kinds[kind])
        _check_fused(read, d, d0, labels, steps, momentum, wd, flags == 0, copy)
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("config", list(CONTEXT_FUSED))
def test_step_and_synchronise_context(config, mask, flags):
    _context_fused(config, flags, mask)


def test_step_and_synchronise_context_with_a_copy_request():
    _context_fused("mom-wd", 0, "all-step-R3", copy=True)


# ---- F. the elastic-averaging and Polyak-Ruppert barriers ----------------------------------
EA, PR = "elastic", "polyak"
AVERAGING = [(EA, False), (PR, False), (PR, True)]
AVERAGING_IDS = ["elastic", "polyak-no-copy", "polyak-copy"]


def _compare_averaging(z, last, s, w, st0, want, labels, model, copied):
    E.assert_edge_equal(z, want.z[0], "z", labels)
    if want.last is not None:
        if model == PR:
            E.assert_edge_equal(last, want.last[0], "base last", labels)
        else:
            assert_bitexact(last, st0.last[0], "base last is not written")
    for i in range(want.size):
        E.assert_edge_equal(w[i], want.w[i], f"w[{i}]", labels)
        assert_bitexact(s[i], st0.s[i], f"s[{i}] is not written")
        if i in copied:
            assert_bitexact(w[i], z, f"w[{i}] is a copy of the device's z")


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
@pytest.mark.parametrize("model,copy", AVERAGING, ids=AVERAGING_IDS)
def test_averaging_barriers_context(model, copy, split):
    from tests.test_gpu_averaging import _make
    R, momentum, clock = 3, 0.9, 3
    st, labels = E.averaging_case(R, momentum)
    g = _make(model, N, R, ALPHA, momentum)
    try:
        if split:
            g.set_force_split(True)
        upload(g, st)
        want = st.clone()
        if copy:
            g.set_replica_copy(1, True)
            want.copy[1] = 1
        assert g.lockAny() == R
        g.synchronise(0, clock, 0, False)
        g.unlockAny()
        g.wait()
        AV.step(want, model == PR, clock)
        z, last, s, w = _read_state(g, R, True)
        _compare_averaging(z, last, s, w, st, want, labels, model, (1,) if copy else ())
        assert g.replica_copy(1) == 0
    finally:
        g.free()


@pytest.mark.parametrize("model,copy", AVERAGING, ids=AVERAGING_IDS)
def test_averaging_barriers_seam(model, copy):
    import torch

    from crossbow_amd.seam import SmaPlan
    R, momentum, clock = 3, 0.9, 3
    st, labels = E.averaging_case(R, momentum)
    if copy:
        st.copy[1] = 1
    want = st.clone()
    z, last = Guarded(st.z[0], 1), Guarded(st.last[0], 2)
    w = [Guarded(a, 10 + i) for i, a in enumerate(st.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(st.s)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with SmaPlan([0], N) as plan:
        if model == PR:
            got = plan.polyak_step([stream.cuda_stream], [z.ptr], [last.ptr],
                                   [(0, w[i].ptr, 1, int(st.copy[i])) for i in range(R)], ALPHA, clock)
            assert got == AV.polyak_ruppert(want, clock) == int(copy)
        else:
            plan.elastic_step([stream.cuda_stream], [z.ptr], [(0, w[i].ptr, s[i].ptr, 1) for i in range(R)], ALPHA)
            AV.elastic_average(want)
        stream.synchronize()
    host = lambda gd: gd.t.cpu().numpy()[:N]  # noqa: E731
    _compare_averaging(host(z), host(last), [host(x) for x in s], [host(x) for x in w], st, want, labels, model,
                       (1,) if copy else ())
    for name, gd in [("z", z), ("last", last)] + [(f"w[{i}]", x) for i, x in enumerate(w)] + \
            [(f"s[{i}]", x) for i, x in enumerate(s)]:
        assert_bitexact(gd.t.cpu().numpy()[N:], gd.sentinel, f"the floats behind {name}")


# ---- G. the S-SGD and DEFAULT task steps and barriers ---------------------------------------
@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_ssgd_task_step_and_barrier(momentum, wd):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST
    R, wpc = 3, 6
    g = _optimiser_context(momentum, wd, update_type=1, wpc=wpc, R=R)
    try:
        # the task step: g = fma(wd, w, g), acc = fma(rate, g, acc)
        a, labels = E.optimiser_case(0.0, wd, np.float32(-LR), seed=500, extra=("acc",), last=False)
        a0 = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        g.replica_write(1, BUF_DATA, a["w"])
        g.replica_write(1, BUF_GRADIENT, a["g"])
        g.base_write(0, BUF_GRADIENT, a["acc"])
        g.replica_optimise(1, task=0)
        g.wait()
        O.ssgd_worker(np.float32(-LR), wd, a["w"], a["g"], a["acc"])
        E.assert_edge_equal(g.base_read(0, BUF_GRADIENT), a["acc"], "acc", labels)
        assert_bitexact(g.replica_read(1, BUF_DATA), a0["w"], "w is not written")
        if wd > 0:
            E.assert_edge_equal(g.replica_read(1, BUF_GRADIENT), a["g"], "g", labels)
        else:
            assert_bitexact(g.replica_read(1, BUF_GRADIENT), a0["g"], "g is not written")
        # the barrier: D = acc / wpc, D = fma(mu, last, D), z += D, acc = 0, every locked w = z
        st = O.make_state(N, 1, R, ALPHA, momentum)
        acc = O.fill_normal(N, 777, 0.01)
        arrays = {"z": st.z[0], "acc": acc}
        if momentum > 0:
            arrays["last"] = st.last[0]
        labels = E.apply(arrays, E.ssgd_sync_scenarios(momentum > 0, wpc))
        upload(g, st)
        g.base_write(0, BUF_GRADIENT, acc)
        assert g.lockAny() == R
        g.synchronise(0, 1, 0, False)
        g.unlockAny()
        g.wait()
        O.ssgd_sync(st, [acc], wpc)
        z = g.base_read(0, BUF_DATA)
        E.assert_edge_equal(z, st.z[0], "z", labels)
        if momentum > 0:
            E.assert_edge_equal(g.base_read(0, BUF_LAST), st.last[0], "base last", labels)
        assert_bitexact(g.base_read(0, BUF_GRADIENT), np.zeros(N, np.float32), "acc is reset to +0")
        for i in range(R):
            assert_bitexact(g.replica_read(i, BUF_DATA), z, f"w[{i}] is a copy of the device's z")
    finally:
        g.free()


@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_default_task_step_and_barrier(momentum, wd):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, UPDATE_DEFAULT
    R = 3
    g = _optimiser_context(momentum, wd, update_type=UPDATE_DEFAULT, R=R)
    try:
        a, labels = E.optimiser_case(momentum, wd, np.float32(-LR), seed=600, extra=("z",))
        a0 = {k: (v.copy() if v is not None else None) for k, v in a.items()}
        w_other = O.fill_normal(N, 650, 0.05)
        g.base_write(0, BUF_DATA, a["z"])
        g.replica_write(0, BUF_DATA, w_other)
        g.replica_write(1, BUF_DATA, a["w"])
        g.replica_write(1, BUF_GRADIENT, a["g"])
        if momentum > 0:
            g.replica_write(1, BUF_LAST, a["last"])
        g.replica_optimise(1, task=0)
        g.wait()
        O.default_task(np.float32(-LR), momentum, wd, a["w"], a["g"], a["last"], a["z"])
        z = g.base_read(0, BUF_DATA)
        E.assert_edge_equal(z, a["z"], "z", labels)
        E.assert_edge_equal(g.replica_read(1, BUF_DATA), a["w"], "w", labels)
        if momentum > 0:
            E.assert_edge_equal(g.replica_read(1, BUF_LAST), a["last"], "last", labels)
        if momentum > 0 or wd > 0:
            E.assert_edge_equal(g.replica_read(1, BUF_GRADIENT), a["g"], "g", labels)
        else:
            assert_bitexact(g.replica_read(1, BUF_GRADIENT), a0["g"], "g is not written")
        assert_bitexact(g.replica_read(0, BUF_DATA), w_other, "the other replica is not written")
        # the barrier copies the base model, edge values and all, into every locked replica
        assert g.lockAny() == R
        g.synchronise(0, 1, 0, False)
        g.unlockAny()
        g.wait()
        assert_bitexact(g.base_read(0, BUF_DATA), z, "z is not written by the barrier")
        for i in range(R):
            assert_bitexact(g.replica_read(i, BUF_DATA), z, f"w[{i}] is a copy of the device's z")
    finally:
        g.free()


# ---- H. the host-staged step -----------------------------------------------------------
@pytest.mark.parametrize("copy", [False, True], ids=["no-copy", "copy"])
@pytest.mark.parametrize("staging,split", [("zerocopy", False), ("zerocopy", True), ("dma", False)],
                         ids=["zerocopy-fused", "zerocopy-split", "dma"])
def test_staged_step(staging, split, copy):
    # zero-copy: sma_fused_staged_kernel, and with the split forced sma_accumulate_staged_kernel and
    # sma_apply_staged_kernel, on the pinned mirror; dma: the device kernels per bucket between copies
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_LAST
    from crossbow_amd._lib import STAGING_DMA, STAGING_ZEROCOPY
    R, momentum = 3, 0.9
    st, labels = E.sma_case(R, momentum)
    g = make_gpu(N, R, ALPHA, momentum)
    try:
        g.set_staging_mode(STAGING_ZEROCOPY if staging == "zerocopy" else STAGING_DMA)
        if split:
            g.set_force_split(True)
        g.base_host_view(0, BUF_DATA)[:] = st.z[0]
        g.base_host_view(0, BUF_LAST)[:] = st.last[0]
        for i in range(R):
            g.replica_host_view(i, BUF_DIFF)[:] = st.s[i]
            g.replica_host_view(i, BUF_DATA)[:] = st.w[i]
        assert_bitexact(g.replica_host_view(0, BUF_DIFF), st.s[0], "the mirror holds the inputs' bits")
        want = st.clone()
        if copy:
            g.set_replica_copy(1, True)
            want.copy[1] = 1
        assert g.lockAny() == R
        g.synchronise_staged(0, 1, 0, 3)
        g.unlockAny()
        g.wait()
        O.sma_step(want)
        copied = range(R) if copy else ()
        host = (g.base_host_view(0, BUF_DATA), g.base_host_view(0, BUF_LAST),
                [g.replica_host_view(i, BUF_DIFF) for i in range(R)],
                [g.replica_host_view(i, BUF_DATA) for i in range(R)])
        _compare_sma(host, st, want, labels, copied, "host mirror: ")
        _compare_sma(_read_state(g, R, True), st, want, labels, copied, "device: ")
    finally:
        g.free()
