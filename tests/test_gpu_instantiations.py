"""Every case of tests/instantiations.py against the oracle, bit for bit (run
with -m gpu).

A case is one call through a public door.  Seeded state goes up, the call is
made, and every buffer the call may touch is compared with the oracle
(``O.sma_step``, ``O.sma_optimise``, ``O.sma_accumulate``, ``O.default_task``,
``O.default_sync``, ``O.ssgd_worker``, ``O.ssgd_sync``, the averaging
restatement of tests/averaging_common.py); every buffer it must not touch is
compared with what was uploaded.  No tolerances.  Output-only buffers (the
snapshot of a stepping replica, acc and D of a split step) hold a sentinel
pattern before the call.

The cases that differ only in setters, `first`, flags and masks share one
context or plan; nothing is restored between cases, everything is uploaded
again.  Which instantiation a case reaches is tests/instantiations.py's claim,
pinned by profiles/instantiations/launched.json (tests/test_instantiations.py).

Not compared: acc and D of a split averaging step (the restatement has no
entry point for Phase A alone; DESIGN.md 4 says so); z, w and last are.

The clipped cases take ``gradient_clip_common.exact_gradient``: a gradient
whose sum of squares is exact in any order and whose scale is exactly 0.5, so
the clipped step is compared bit for bit like every other.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import gradient_clip_common as C
from tests import instantiations as I
from tests.helpers import Guarded, assert_bitexact, compare_states, download, upload

pytestmark = pytest.mark.gpu

ALPHA = 0.1
WD = 5e-4
MOMENTUM = 0.9
CLOCK = 2
DISCARD = 1  # CBX_STEP_DISCARD_TASK_OUTPUTS
WPC = 3
TASK_SIDE = ("optimise", "optimise_vars", "default_task", "ssgd_task", "ssgd", "default_sync")
R = I.CTX_REPLICAS


def _num_cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _group(c: I.Case) -> str:
    size = c.n if isinstance(c.n, str) else "small"
    key = [c.family, c.door, c.form, size]
    if c.door == "context":
        if c.family == "task_barrier":
            key.append(("mom" if c.rep_mom else "nomom") + ("-wd" if c.wd else ""))
        if c.family == "polyak":
            key.append("last" if c.base_mom else "nolast")
        if c.family in ("optimise", "optimise_vars", "default_task"):
            key.append(("mom" if c.rep_mom else "nomom") + ("-wd" if c.wd else ""))
        if c.family == "ssgd_task":
            key.append("wd" if c.wd else "nowd")
    return "-".join(key)


GROUPS: "OrderedDict[str, list]" = OrderedDict()
for _c in I.CASES:
    GROUPS.setdefault(_group(_c), []).append(_c)


# ---------------------------------------------------------------------------
# Inputs: one seeded state per (n, momentum), computed once and never changed.
# ---------------------------------------------------------------------------
_STATES = {}


def _base_state(n: int, momentum: float) -> O.SmaState:
    key = (n, momentum > 0)
    if key not in _STATES:
        # one replica more than the context has: the seam cases keep one outside the step
        _STATES[key] = O.make_state(n, 1, R + 1, ALPHA, momentum, threads=8 if n > 100_000 else 1)
    return _STATES[key]


_FILLS = {}


def _fill(n: int, seed: int, sigma: float) -> np.ndarray:
    key = (n, seed, sigma)
    if key not in _FILLS:
        _FILLS[key] = O.fill_normal(n, seed, sigma)
    return _FILLS[key]


def _sentinel(n: int, tag: int) -> np.ndarray:
    """Every kind of value, NaNs among them (as tests/helpers.py's Guarded)."""
    bits = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(0x7FC00000 + tag)
    return bits.view(np.float32)


def _state(n: int, replicas: int, momentum: float, with_last: bool) -> O.SmaState:
    """The first `replicas` replicas of the shared state, as fresh arrays."""
    b = _base_state(n, MOMENTUM if with_last else 0.0)
    return O.SmaState(1, replicas, n, ALPHA, momentum, [b.z[0].copy()],
                      [b.last[0].copy()] if b.last is not None else None,
                      [a.copy() for a in b.s[:replicas]], [a.copy() for a in b.w[:replicas]])


def _steps(c: I.Case, first: int, total: int):
    """Which replicas step: all, or every other one, of the participating."""
    part = list(range(first, total))
    if c.steps == "all":
        return set(part)
    if c.steps == "some":
        return set(part[::2])
    return set()


class Failures:
    def __init__(self, cus):
        self.cus, self.bad, self.ran = cus, [], 0

    def run(self, case, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{case.name()} -> {', '.join(I.expected_kernels(case, self.cus))}: {e}")

    def done(self):
        assert self.ran > 0
        assert not self.bad, f"{len(self.bad)} of {self.ran} cases differ from the oracle:\n" + "\n".join(self.bad[:40])


# ---------------------------------------------------------------------------
# The context door.
# ---------------------------------------------------------------------------
def _context(n, update_type, momentum, wd=0.0, elastic=False):
    import crossbow_amd
    g = crossbow_amd.TheGPU()
    g.init([0])
    try:
        g.setModel(1, 4 * n)
        g.setModelVariable(0, 1, [n], 4 * n)
        g.setUpdateModelType(update_type)
        if elastic:
            g.setElasticAverage(True)
        g.setEamsgdAlpha(ALPHA)
        g.setMomentum(momentum, 0)
        g.setWeightDecay(wd)
        g.setLearningRateDecayPolicyExp(0.05, 0.97)
        g.setModelWorkPerClock(WPC)
        g.setModelManager(R, 0)
    except Exception:
        g.free()
        raise
    return g


def _configure(g, c: I.Case):
    """The setters a case names; the defaults where it names none."""
    from crossbow_amd._abi import ALLREDUCE_RCCL, ALLREDUCE_RSAG
    if c.family in TASK_SIDE:
        block, bpc, unroll, waves = c.cfg if c.cfg is not None else I._main_cfg(c)
        assert bpc == 0 and c.policy == 1
        if c.family in ("ssgd", "default_sync"):
            g.set_barrier_kernel_config(block, unroll, waves)
        else:
            g.set_aux_kernel_config(block, unroll, waves)
        return
    block, bpc, unroll, waves = c.cfg if c.cfg is not None else I._main_cfg(c)
    if c.family == "sma":
        g.set_kernel_config(block, bpc, c.policy, unroll)
        g.set_kernel_occupancy(waves)
    else:
        assert bpc == 0
        g.set_kernel_config(64, 0, c.policy, 2)  # the policy is shared (context.hip:2079-2081)
        if c.family == "task_barrier":
            g.set_task_barrier_kernel_config(block, unroll, waves)
        else:
            g.set_averaging_kernel_config(block, unroll, waves)
    g.set_apply_kernel_config(*(c.apply_cfg if c.apply_cfg is not None else I.APPLY_CFG))
    g.set_force_split(c.form != "fused")
    g.set_allreduce_algorithm(ALLREDUCE_RSAG if c.form == "rsag" else ALLREDUCE_RCCL)


def _barrier(g, first, clock=CLOCK):
    g.lockAny()
    g.synchronise(first, clock, 0, False)
    g.unlockAny()
    g.wait()


def _set_copies(g, st):
    for i in range(R):
        g.set_replica_copy(i, bool(st.copy[i]))


def _sma_context_case(g, c: I.Case, n: int):
    from crossbow_amd import BUF_DIFF, BUF_GRADIENT
    _configure(g, c)
    g.setMomentum(MOMENTUM if c.base_mom else 0.0, 0)  # base momentum is read at the step (sync_steps.hip:1273)
    want = _state(n, R, MOMENTUM if c.base_mom else 0.0, with_last=True)
    first = R - c.nrep
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    upload(g, want)
    _set_copies(g, want)
    split = c.form != "fused"
    if split:
        g.base_write(0, BUF_GRADIENT, _sentinel(n, 1))
        g.base_write(0, BUF_DIFF, _sentinel(n, 2))
        if c.nrep > 0:
            acc, _ = O.sma_accumulate(ALPHA, want.z[0], want.s[first:], [a.copy() for a in want.w[first:]])
        else:
            acc = np.zeros(n, np.float32)  # sma.c:66
    _barrier(g, first)
    O.sma_step(want)
    compare_states(download(g, want), want)
    if split:
        assert_bitexact(g.base_read(0, BUF_GRADIENT), acc, "acc")
        assert_bitexact(g.base_read(0, BUF_DIFF), acc, "D (one rank: the all-reduce is the identity)")
    assert [g.replica_copy(i) for i in range(R)] == [0] * R, "copy flags after the step"


def _sma_staged_context_case(g, c: I.Case, n: int):
    """cbx_synchronise_staged (zero-copy): the host mirrors go in and come out, and the device ends as
    the host does.  Mirrors and device buffers start from the same state."""
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    split = c.form == "staged_split"
    g.set_force_split(split)
    g.setMomentum(MOMENTUM if c.base_mom else 0.0, 0)
    want = _state(n, R, MOMENTUM if c.base_mom else 0.0, with_last=True)
    first = R - c.nrep
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    upload(g, want)
    _set_copies(g, want)
    g.base_host_view(0, BUF_DATA)[:] = want.z[0]
    g.base_host_view(0, BUF_LAST)[:] = want.last[0]
    for i in range(R):
        g.replica_host_view(i, BUF_DIFF)[:] = want.s[i]
        g.replica_host_view(i, BUF_DATA)[:] = want.w[i]
    if split:
        g.base_write(0, BUF_GRADIENT, _sentinel(n, 1))
        if c.nrep > 0:
            acc, _ = O.sma_accumulate(ALPHA, want.z[0], want.s[first:], [a.copy() for a in want.w[first:]])
        else:
            acc = np.zeros(n, np.float32)  # sma.c:66
    g.lockAny()
    g.synchronise_staged(first, CLOCK, 0, 1)
    g.unlockAny()
    g.wait()
    O.sma_step(want)
    compare_states(download(g, want), want)
    assert_bitexact(g.base_host_view(0, BUF_DATA), want.z[0], "z, host mirror")
    assert_bitexact(g.base_host_view(0, BUF_LAST), want.last[0], "last, host mirror")
    for i in range(R):
        assert_bitexact(g.replica_host_view(i, BUF_DATA), want.w[i], f"w[{i}], host mirror")
        assert_bitexact(g.replica_host_view(i, BUF_DIFF), want.s[i], f"s[{i}], host mirror")
    if split:
        assert_bitexact(g.base_read(0, BUF_GRADIENT), acc, "acc")
    assert [g.replica_copy(i) for i in range(R)] == [0] * R, "copy flags after the step"


def _task_barrier_context_case(g, c: I.Case, n: int, momentum: float, wd: float):
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    _configure(g, c)
    assert c.base_mom <= (momentum > 0)
    g.setMomentum(MOMENTUM if c.base_mom else 0.0, 0)  # bmom is read at the call (context.hip:771)
    want = _state(n, R, MOMENTUM if c.base_mom else 0.0, with_last=momentum > 0)
    first = R - c.nrep
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    stepping = _steps(c, first, R)
    tasks = [3 + 2 * i if i in stepping else -1 for i in range(R)]
    rates = [g.replica_learning_rate(i, tasks[i]) if i in stepping else 0.0 for i in range(R)]
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(R)]
    rlast = [_fill(n, 5100 + i, 0.001).copy() if momentum > 0 else None for i in range(R)]
    for i in stepping:  # written only: s = w (sma.cu:71), or left alone under the discard flag
        want.s[i] = _sentinel(n, 100 + i).copy()
    upload(g, want)
    _set_copies(g, want)
    for i in range(R):
        g.replica_write(i, BUF_GRADIENT, grad[i])
        if rlast[i] is not None:
            g.replica_write(i, BUF_LAST, rlast[i])
    g.lockAny()
    g.step_and_synchronise(first, CLOCK, 0, tasks, None, 0 if c.keep else DISCARD)
    g.unlockAny()
    g.wait()
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    for i in sorted(stepping):
        O.sma_optimise(np.float32(-rates[i]), momentum, wd, want.w[i], grad[i], rlast[i], want.s[i])
    O.sma_step(want)
    for i, (s, gr) in kept.items():
        want.s[i], grad[i] = s, gr
    compare_states(download(g, want), want)
    for i in range(R):
        assert_bitexact(g.replica_read(i, BUF_GRADIENT), grad[i], f"g[{i}]")
        if rlast[i] is not None:
            assert_bitexact(g.replica_read(i, BUF_LAST), rlast[i], f"last[{i}]")
    assert [g.replica_copy(i) for i in range(R)] == [0] * R, "copy flags after the step"


def _averaging_context_case(g, c: I.Case, n: int, with_last: bool):
    _configure(g, c)
    polyak = c.family == "polyak"
    alpha = 0.0 if c.alpha0 else ALPHA
    g.setEamsgdAlpha(alpha)
    want = _state(n, R, MOMENTUM if with_last else 0.0, with_last=with_last)
    want.alpha = alpha
    first = R - c.nrep
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    upload(g, want)
    _set_copies(g, want)
    _barrier(g, first)
    AV.step(want, polyak, CLOCK)
    compare_states(download(g, want), want)
    assert [g.replica_copy(i) for i in range(R)] == [int(x) for x in want.copy], "copy flags after the step"


def _task_side_context_case(g, c: I.Case, n: int, momentum: float, wd: float):
    """One replica's task step (cbx_replica_optimise under SMA, DEFAULT or WORKER), or the S-SGD /
    DEFAULT barrier; every buffer of the context is compared."""
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    _configure(g, c)
    barrier = c.family in ("ssgd", "default_sync")
    base_momentum = MOMENTUM if (c.family == "ssgd" and c.base_mom) else 0.0
    if c.family == "ssgd":
        g.setMomentum(base_momentum, 0)  # read at the step (sync_steps.hip:1686)
    want = _state(n, R, base_momentum, with_last=momentum > 0)
    first = R - c.nrep if barrier else 0
    want.first = first
    i, task = 4, 7
    grad = [_fill(n, 5000 + k, 0.01).copy() for k in range(R)]
    rlast = [_fill(n, 5100 + k, 0.001).copy() if momentum > 0 else None for k in range(R)]
    acc = _fill(n, 5200, 0.01).copy()
    if c.family == "optimise":
        want.s[i] = _sentinel(n, 100 + i).copy()  # written only: s = w (sma.cu:71)
        scale, flags = np.float32(1.0), 0
        if c.clip:
            grad[i], S, max_norm = C.exact_gradient(n)
            scale, flags = C.decide(S, 0, max_norm, False)
            assert flags == C.CLIPPED and scale == np.float32(0.5)
        g.set_gradient_clip(max_norm if c.clip else 0.0, False)
    upload(g, want)
    for k in range(R):
        g.replica_write(k, BUF_GRADIENT, grad[k])
        if rlast[k] is not None:
            g.replica_write(k, BUF_LAST, rlast[k])
    g.base_write(0, BUF_GRADIENT, acc)
    if barrier:
        _barrier(g, first)
        if c.family == "ssgd":
            O.ssgd_sync(want, [acc], WPC)
        else:
            O.default_sync(want)
    else:
        rate = np.float32(-g.replica_learning_rate(i, task))
        g.replica_optimise(i, task)
        g.wait()
        if c.family == "optimise":
            if c.clip:
                grad[i] *= scale  # one fp32 multiply before weight decay (sma_kernels.hip:598-604)
            O.sma_optimise(rate, momentum, wd, want.w[i], grad[i], rlast[i], want.s[i])
        elif c.family == "default_task":
            O.default_task(rate, momentum, wd, want.w[i], grad[i], rlast[i], want.z[0])
        else:
            O.ssgd_worker(rate, wd, want.w[i], grad[i], acc)
    compare_states(download(g, want), want)
    assert_bitexact(g.base_read(0, BUF_GRADIENT), acc, "the base model's gradient (acc)")
    for k in range(R):
        assert_bitexact(g.replica_read(k, BUF_GRADIENT), grad[k], f"g[{k}]")
        if rlast[k] is not None:
            assert_bitexact(g.replica_read(k, BUF_LAST), rlast[k], f"last[{k}]")


def _variables_context_case(g, c: I.Case, momentum: float, wd: float):
    """cbx_replica_optimise with cbx_set_variable_learning_rates on: every variable of
    tests/test_optimise_plan.py's model with its own rate, clipped or not."""
    from tests.test_optimise_plan import M, V
    n = sum(V)
    assert n == I.N_VARS
    block, _, unroll, waves = c.cfg if c.cfg is not None else I._main_cfg(c)
    g.set_aux_kernel_config(block, unroll, waves)
    bufs = C.host(400, n, momentum)
    scale, flags, max_norm = np.float32(1.0), 0, 0.0
    if c.clip:
        bufs[1], S, max_norm = C.exact_gradient(n)
        scale, flags = C.decide(S, 0, max_norm, False)
        assert flags == C.CLIPPED and scale == np.float32(0.5)
    g.set_gradient_clip(max_norm, False)
    C.put(g, 0, bufs)
    g.replica_optimise(0, 3)
    g.wait()
    C.step(bufs, scale, flags, momentum, wd, variables=V, mults=M)
    for name, got, exp in zip(("w", "g", "last", "s"), C.get(g, 0, momentum), bufs):
        if exp is not None:
            assert_bitexact(got, exp, name)


def _run_context_group(cases, cus):
    from crossbow_amd import (UPDATE_DEFAULT, UPDATE_POLYAK_RUPPERT, UPDATE_SMA, UPDATE_SYNCHRONOUSEAMSGD,
                              UPDATE_WORKER)
    c0 = cases[0]
    n = c0.elements(cus)
    fails = Failures(cus)
    if c0.family == "sma":
        g = _context(n, UPDATE_SMA, MOMENTUM)
        staged = c0.form in ("staged", "staged_split")
        run = lambda c: (_sma_staged_context_case if staged else _sma_context_case)(g, c, n)  # noqa: E731
    elif c0.family == "task_barrier":
        momentum, wd = (MOMENTUM if c0.rep_mom else 0.0), (WD if c0.wd else 0.0)
        g = _context(n, UPDATE_SMA, momentum, wd)
        run = lambda c: _task_barrier_context_case(g, c, n, momentum, wd)  # noqa: E731
    elif c0.family == "optimise_vars":
        from tests.test_optimise_plan import M, V
        momentum, wd = (MOMENTUM if c0.rep_mom else 0.0), (WD if c0.wd else 0.0)
        g = C.context(n, momentum, wd, variables=list(V), mults=list(M))
        g.set_variable_learning_rates(True)
        run = lambda c: _variables_context_case(g, c, momentum, wd)  # noqa: E731
    elif c0.family in TASK_SIDE:
        # the S-SGD barrier's context has base->last and switches the momentum per case
        momentum = MOMENTUM if (c0.rep_mom or c0.family == "ssgd") else 0.0
        wd = WD if c0.wd else 0.0
        kind = {"optimise": UPDATE_SMA, "default_task": UPDATE_DEFAULT, "default_sync": UPDATE_DEFAULT,
                "ssgd_task": UPDATE_WORKER, "ssgd": UPDATE_WORKER}[c0.family]
        g = _context(n, kind, momentum, wd)
        run = lambda c: _task_side_context_case(g, c, n, momentum, wd)  # noqa: E731
    else:
        polyak = c0.family == "polyak"
        with_last = polyak and c0.base_mom
        g = _context(n, UPDATE_POLYAK_RUPPERT if polyak else UPDATE_SYNCHRONOUSEAMSGD, MOMENTUM if with_last else 0.0,
                     elastic=not polyak)
        run = lambda c: _averaging_context_case(g, c, n, with_last)  # noqa: E731
    try:
        for c in cases:
            assert c.elements(cus) == n
            fails.run(c, lambda: run(c))
    finally:
        g.free()
    fails.done()


# ---------------------------------------------------------------------------
# The seam door: buffers the caller owns, each followed by guard floats.
# ---------------------------------------------------------------------------
def _seam_layout(c: I.Case):
    """(replicas passed, first): one replica below `first` stays outside the step
    (at the large size only where nobody takes part, to keep the uploads small)."""
    if c.n == "seam_u2":
        return (max(c.nrep, 1), 0 if c.nrep else 1)
    return (c.nrep + 1, 1)


def _seam_case(plan, c: I.Case, n: int):
    import torch
    total, first = _seam_layout(c)
    polyak = c.family == "polyak"
    tb = c.family == "task_barrier"
    with_last = c.base_mom
    base_momentum = MOMENTUM if (c.base_mom and not polyak) else 0.0
    want = _state(n, total, base_momentum, with_last=with_last)
    want.first = first
    want.alpha = 0.0 if c.alpha0 else ALPHA
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    stepping = _steps(c, first, total) if tb else set()
    rmom = MOMENTUM if (tb and c.rep_mom) else 0.0
    wd = WD if (tb and c.wd) else 0.0
    rates = [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(total)]
    for i in stepping:
        want.s[i] = _sentinel(n, 100 + i).copy()
    z = Guarded(want.z[0], 1)
    blast = Guarded(want.last[0], 2) if want.last is not None else None
    w = [Guarded(a, 10 + i) for i, a in enumerate(want.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(want.s)]
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(total)] if tb else []
    rlast = [_fill(n, 5100 + i, 0.001).copy() if rmom > 0 else None for i in range(total)] if tb else []
    gg = [Guarded(a, 210 + i) for i, a in enumerate(grad)]
    gl = [Guarded(a, 310 + i) if a is not None else None for i, a in enumerate(rlast)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    streams, zp = [stream.cuda_stream], [z.ptr]
    lp = [blast.ptr] if blast is not None else None
    locked = [1] * total
    if c.family == "sma":
        got = plan.step(streams, zp, lp, [(0, w[i].ptr, s[i].ptr, locked[i], int(want.copy[i])) for i in range(total)],
                        ALPHA, base_momentum, first)
        exp = 1 if O.sma_step(want) > 0 else 0
    elif tb:
        reps = [(0, w[i].ptr, s[i].ptr, gg[i].ptr, gl[i].ptr if gl[i] is not None else None, locked[i],
                 int(want.copy[i]), int(i in stepping), rates[i]) for i in range(total)]
        got = plan.step_and_optimise(streams, zp, lp, reps, ALPHA, base_momentum, rmom, wd, first,
                                     0 if c.keep else DISCARD)
        kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
        for i in sorted(stepping):
            O.sma_optimise(np.float32(-rates[i]), rmom, wd, want.w[i], grad[i], rlast[i], want.s[i])
        exp = 1 if O.sma_step(want) > 0 else 0
        for i, (sv, gr) in kept.items():
            want.s[i], grad[i] = sv, gr
    elif polyak:
        got = plan.polyak_step(streams, zp, lp, [(0, w[i].ptr, locked[i], int(want.copy[i])) for i in range(total)],
                               want.alpha, CLOCK, first)
        exp = AV.polyak_ruppert(want, CLOCK)
    else:
        plan.elastic_step(streams, zp, [(0, w[i].ptr, None, locked[i]) for i in range(total)], want.alpha, first)
        got = exp = 0
        AV.elastic_average(want)
    stream.synchronize()
    assert got == exp, f"return value {got}, the oracle's {exp}"
    z.check(want.z[0], "z")
    if blast is not None:
        blast.check(want.last[0], "base last")
    for i in range(total):
        w[i].check(want.w[i], f"w[{i}]")
        s[i].check(want.s[i], f"s[{i}]")
        if tb:
            gg[i].check(grad[i], f"g[{i}]")
            if gl[i] is not None:
                gl[i].check(rlast[i], f"last[{i}]")


def _task_side_seam_case(plan, c: I.Case, n: int):
    """The seam's task steps (cbx_sma_optimise_buffers, cbx_ssgd_accumulate_buffers) and its S-SGD
    barrier (cbx_ssgd_plan_step) over guarded buffers of exactly n floats."""
    import torch

    from crossbow_amd.seam import optimise_buffers, ssgd_accumulate_buffers
    momentum = MOMENTUM if c.rep_mom else 0.0
    wd = WD if c.wd else 0.0
    lr = float(np.float32(0.05 / 1.37))
    stream = torch.cuda.Stream()
    if c.family == "ssgd":
        total, first = c.nrep + 1, 1
        base_momentum = MOMENTUM if c.base_mom else 0.0
        want = _state(n, total, base_momentum, with_last=c.base_mom)
        want.first = first
        acc = _fill(n, 5200, 0.01).copy()
        z, ga = Guarded(want.z[0], 1), Guarded(acc, 3)
        blast = Guarded(want.last[0], 2) if want.last is not None else None
        w = [Guarded(a, 10 + k) for k, a in enumerate(want.w)]
        torch.cuda.synchronize()
        plan.ssgd_step([stream.cuda_stream], [z.ptr], [blast.ptr] if blast is not None else None, [ga.ptr],
                       [(0, w[k].ptr, 1) for k in range(total)], base_momentum, WPC, first)
        stream.synchronize()
        O.ssgd_sync(want, [acc], WPC)
        z.check(want.z[0], "z")
        ga.check(acc, "acc")
        if blast is not None:
            blast.check(want.last[0], "base last")
        for k in range(total):
            w[k].check(want.w[k], f"w[{k}]")
        return
    base = _base_state(n, 0.0)
    hw, hg = base.w[2].copy(), _fill(n, 5002, 0.01).copy()
    scale, flags, max_norm = np.float32(1.0), 0, 0.0
    if c.clip:
        hg, S, max_norm = C.exact_gradient(n)
        scale, flags = C.decide(S, 0, max_norm, False)
        assert flags == C.CLIPPED and scale == np.float32(0.5)
    variables = c.family == "optimise_vars"
    if variables:
        from tests.test_optimise_plan import M, V
        assert n == sum(V) == I.N_VARS
        lr = C.LR
    hl = _fill(n, 5102, 0.001).copy() if momentum > 0 else None
    hs, hacc = _sentinel(n, 102).copy(), _fill(n, 5200, 0.01).copy()
    w, gg, s, ga = Guarded(hw, 10), Guarded(hg, 210), Guarded(hs, 110), Guarded(hacc, 3)
    gl = Guarded(hl, 310) if hl is not None else None
    torch.cuda.synchronize()
    lastp = gl.ptr if gl is not None else None
    if variables or c.clip:
        if variables:
            plan.set_variables(list(V), list(M))
        if c.clip:
            plan.optimise_clipped(0, 5, stream.cuda_stream, w.ptr, gg.ptr, lastp, s.ptr, lr, momentum, wd, max_norm,
                                  False, variables)
        else:
            plan.optimise_variables(0, stream.cuda_stream, w.ptr, gg.ptr, lastp, s.ptr, lr, momentum, wd, 0, len(V))
        C.step([hw, hg, hl, hs], scale, flags, momentum, wd, lr=lr, variables=V if variables else None,
               mults=M if variables else None)
    elif c.family == "optimise":
        optimise_buffers(stream.cuda_stream, w.ptr, gg.ptr, lastp, s.ptr, n, lr, momentum, wd)
        O.sma_optimise(np.float32(-lr), momentum, wd, hw, hg, hl, hs)
    else:
        ssgd_accumulate_buffers(stream.cuda_stream, w.ptr, gg.ptr, ga.ptr, n, lr, wd)
        O.ssgd_worker(np.float32(-lr), wd, hw, hg, hacc)
    stream.synchronize()
    w.check(hw, "w")
    gg.check(hg, "g")
    s.check(hs, "s")
    ga.check(hacc, "acc")
    if gl is not None:
        gl.check(hl, "last")


def _run_seam_group(cases, cus):
    from crossbow_amd.seam import SmaPlan
    fails = Failures(cus)
    plans = {}
    try:
        for c in cases:
            n = c.elements(cus)
            if n not in plans:
                plans[n] = SmaPlan([0], n)
            fails.run(c, lambda: (_task_side_seam_case if c.family in TASK_SIDE else _seam_case)(plans[n], c, n))
    finally:
        for p in plans.values():
            p.free()
    fails.done()


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_bitexact(group):
    cases = GROUPS[group]
    cus = _num_cus()
    for c in cases:
        I.expected_kernels(c, cus)  # the model must place every case on this device too
    if cases[0].door == "context":
        _run_context_group(cases, cus)
    else:
        _run_seam_group(cases, cus)
