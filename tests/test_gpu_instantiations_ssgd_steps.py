"""Every case of tests/instantiations_ssgd_steps.py against the oracle, bit for
bit (run with -m gpu): one call through ``cbx_step_and_synchronise_ssgd`` or
``cbx_ssgd_plan_step_and_optimise`` per case, so that every kernel
``libcrossbow_sma_ssgd_steps.so`` compiles runs against ``O.ssgd_worker`` and
``O.ssgd_sync``.  The base gradient is never zero on entry.

The inputs, the sentinels in output-only buffers and the sharing of one context
or plan per group are tests/test_gpu_instantiations.py's.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest

from oracle import oracle as O
from tests import instantiations as I
from tests import instantiations_ssgd_steps as IS
from tests.helpers import Guarded, assert_bitexact, compare_states, download, upload
from tests.test_gpu_instantiations import (ALPHA, CLOCK, DISCARD, MOMENTUM, WD, WPC, R, _configure, _context, _fill,
                                           _num_cus, _sentinel, _state, _steps)

pytestmark = pytest.mark.gpu


def _group(c: I.Case) -> str:
    key = [c.door]
    if c.door == "context":
        key.append(("mom" if c.base_mom else "nomom") + ("-wd" if c.wd else ""))
    else:
        key.append(str(c.n))
    return "-".join(key)


GROUPS: "OrderedDict[str, list]" = OrderedDict()
for _c in IS.CASES:
    GROUPS.setdefault(_group(_c), []).append(_c)


class Failures:
    def __init__(self, cus):
        self.cus, self.bad, self.ran = cus, [], 0

    def run(self, case, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{case.name()} -> {IS.expected_kernel(case, self.cus)}: {e}")

    def done(self):
        assert self.ran > 0
        assert not self.bad, f"{len(self.bad)} of {self.ran} cases differ from the oracle:\n" + "\n".join(self.bad[:40])


def _receivers_start_as_sentinels(want, stepping, wd, first, total, n):
    """A receiving replica's w is written only, unless it steps with weight decay."""
    for i in range(first, total):
        if not (i in stepping and wd > 0):
            want.w[i] = _sentinel(n, 300 + i).copy()


def _context_case(g, c: I.Case, n: int, momentum: float, wd: float):
    from crossbow_amd import BUF_GRADIENT
    _configure(g, c)
    want = _state(n, R, momentum, with_last=momentum > 0)  # the state's momentum is the base model's
    first = R - c.nrep
    want.first = first
    stepping = _steps(c, first, R)
    assert len(stepping) == IS.stepping_count(c)
    tasks = [3 + 2 * i if i in stepping else -1 for i in range(R)]
    rates = [g.replica_learning_rate(i, tasks[i]) if i in stepping else 0.0 for i in range(R)]
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(R)]
    acc = _fill(n, 5200, 0.01).copy()
    _receivers_start_as_sentinels(want, stepping, wd, first, R, n)
    upload(g, want)
    g.base_write(0, BUF_GRADIENT, acc)
    for i in range(R):
        g.replica_write(i, BUF_GRADIENT, grad[i])
    g.lockAny()
    g.step_and_synchronise_ssgd(first, CLOCK, 0, tasks, None, 0 if c.keep else DISCARD)
    g.unlockAny()
    g.wait()
    kept = {i: grad[i].copy() for i in stepping if not c.keep}
    for i in sorted(stepping):
        O.ssgd_worker(np.float32(-rates[i]), wd, want.w[i], grad[i], acc)
    O.ssgd_sync(want, [acc], WPC)
    grad = [kept.get(i, grad[i]) for i in range(R)]
    compare_states(download(g, want), want)
    assert_bitexact(g.base_read(0, BUF_GRADIENT), acc, "base gradient")
    for i in range(R):
        assert_bitexact(g.replica_read(i, BUF_GRADIENT), grad[i], f"g[{i}]")


def _seam_case(plan, c: I.Case, n: int):
    import torch
    total, first = c.nrep + 1, 1  # one replica below `first` stays outside the step
    bmom = MOMENTUM if c.base_mom else 0.0
    want = _state(n, total, bmom, with_last=c.base_mom)
    want.first = first
    stepping = _steps(c, first, total)
    assert len(stepping) == IS.stepping_count(c)
    wd = WD if c.wd and stepping else 0.0
    rates = [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(total)]
    _receivers_start_as_sentinels(want, stepping, wd, first, total, n)
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(total)]
    acc = _fill(n, 5200, 0.01).copy()
    z, ga = Guarded(want.z[0], 1), Guarded(acc, 3)
    last = Guarded(want.last[0], 2) if want.last is not None else None
    w = [Guarded(a, 10 + i) for i, a in enumerate(want.w)]
    gg = [Guarded(a, 210 + i) for i, a in enumerate(grad)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    # a replica that only joins passes no g
    reps = [(0, w[i].ptr, gg[i].ptr if i in stepping else None, 1, int(i in stepping), rates[i]) for i in range(total)]
    plan.ssgd_step_and_optimise([stream.cuda_stream], [z.ptr], [last.ptr] if last is not None else None, [ga.ptr], reps,
                                bmom, wd, WPC, first, 0 if c.keep else DISCARD)
    kept = {i: grad[i].copy() for i in stepping if not c.keep}
    for i in sorted(stepping):
        O.ssgd_worker(np.float32(-rates[i]), wd, want.w[i], grad[i], acc)
    O.ssgd_sync(want, [acc], WPC)
    stream.synchronize()
    z.check(want.z[0], "z")
    ga.check(acc, "acc")
    if last is not None:
        last.check(want.last[0], "last")
    for i in range(total):
        w[i].check(want.w[i], f"w[{i}]")
        gg[i].check(kept.get(i, grad[i]), f"g[{i}]")


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_bitexact(group):
    cases = GROUPS[group]
    cus = _num_cus()
    fails = Failures(cus)
    n = cases[0].elements(cus)
    if cases[0].door == "context":
        import crossbow_amd
        # a group's context has the base momentum and the stepping replicas' weight decay
        momentum, wd = (MOMENTUM if cases[0].base_mom else 0.0), (WD if cases[0].wd else 0.0)
        g = _context(n, crossbow_amd.UPDATE_WORKER, momentum, wd)
        try:
            for c in cases:
                fails.run(c, lambda: _context_case(g, c, n, momentum, wd))
        finally:
            g.free()
    else:
        from crossbow_amd.seam import SmaPlan
        with SmaPlan([0], n) as plan:
            for c in cases:
                fails.run(c, lambda: _seam_case(plan, c, n))
    fails.done()


def test_the_cases_reach_every_compiled_kernel_on_this_device():
    from tests.test_instantiations_ssgd_steps import compiled_kernels
    assert set(IS.case_names(_num_cus())) == compiled_kernels()
