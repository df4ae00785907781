"""Every case of tests/instantiations_elastic_steps.py against the oracle, bit
for bit (run with -m gpu): one call through ``cbx_step_and_synchronise_elastic``
or ``cbx_ea_plan_step_and_optimise`` per case, so that every kernel
``libcrossbow_sma_elastic_steps.so`` compiles runs against ``O.sma_optimise``
and ``tests.averaging_common.elastic_average``.

The inputs, the sentinels in output-only buffers and the sharing of one context
or plan per group are tests/test_gpu_instantiations.py's.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import instantiations as I
from tests import instantiations_elastic_steps as IE
from tests.helpers import Guarded, assert_bitexact, compare_states, download, upload
from tests.test_gpu_instantiations import (ALPHA, CLOCK, DISCARD, MOMENTUM, WD, R, _configure, _context, _fill, _num_cus,
                                           _sentinel, _state, _steps)

pytestmark = pytest.mark.gpu


def _group(c: I.Case) -> str:
    key = [c.door]
    if c.door == "context":
        key.append(("mom" if c.rep_mom else "nomom") + ("-wd" if c.wd else ""))
    else:
        key.append(str(c.n))
    return "-".join(key)


GROUPS: "OrderedDict[str, list]" = OrderedDict()
for _c in IE.CASES:
    GROUPS.setdefault(_group(_c), []).append(_c)


class Failures:
    def __init__(self, cus):
        self.cus, self.bad, self.ran = cus, [], 0

    def run(self, case, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{case.name()} -> {IE.expected_kernel(case, self.cus)}: {e}")

    def done(self):
        assert self.ran > 0
        assert not self.bad, f"{len(self.bad)} of {self.ran} cases differ from the oracle:\n" + "\n".join(self.bad[:40])


def _context_case(g, c: I.Case, n: int, momentum: float, wd: float):
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    _configure(g, c)
    want = _state(n, R, 0.0, with_last=momentum > 0)  # the base `last` exists with momentum and is left alone
    first = R - c.nrep
    want.first = first
    stepping = _steps(c, first, R)
    tasks = [3 + 2 * i if i in stepping else -1 for i in range(R)]
    rates = [g.replica_learning_rate(i, tasks[i]) if i in stepping else 0.0 for i in range(R)]
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(R)]
    rlast = [_fill(n, 5100 + i, 0.001).copy() if momentum > 0 else None for i in range(R)]
    for i in range(first, R):  # never read: written (s = w) by a stepping replica whose outputs are kept
        want.s[i] = _sentinel(n, 100 + i).copy()
    upload(g, want)
    for i in range(R):
        g.replica_write(i, BUF_GRADIENT, grad[i])
        if rlast[i] is not None:
            g.replica_write(i, BUF_LAST, rlast[i])
    g.lockAny()
    g.step_and_synchronise_elastic(first, CLOCK, 0, tasks, None, 0 if c.keep else DISCARD)
    g.unlockAny()
    g.wait()
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    for i in sorted(stepping):
        O.sma_optimise(np.float32(-rates[i]), momentum, wd, want.w[i], grad[i], rlast[i], want.s[i])
    AV.elastic_average(want)
    for i, (s, gr) in kept.items():
        want.s[i], grad[i] = s, gr
    compare_states(download(g, want), want)
    for i in range(R):
        assert_bitexact(g.replica_read(i, BUF_GRADIENT), grad[i], f"g[{i}]")
        if rlast[i] is not None:
            assert_bitexact(g.replica_read(i, BUF_LAST), rlast[i], f"last[{i}]")


def _seam_case(plan, c: I.Case, n: int):
    import torch
    total, first = c.nrep + 1, 1  # one replica below `first` stays outside the step
    want = _state(n, total, 0.0, with_last=False)
    want.first = first
    stepping = _steps(c, first, total)
    rmom = MOMENTUM if c.rep_mom and stepping else 0.0
    wd = WD if c.wd and stepping else 0.0
    rates = [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(total)]
    for i in range(first, total):
        want.s[i] = _sentinel(n, 100 + i).copy()
    z = Guarded(want.z[0], 1)
    w = [Guarded(a, 10 + i) for i, a in enumerate(want.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(want.s)]
    grad = [_fill(n, 5000 + i, 0.01).copy() for i in range(total)]
    rlast = [_fill(n, 5100 + i, 0.001).copy() if rmom > 0 else None for i in range(total)]
    gg = [Guarded(a, 210 + i) for i, a in enumerate(grad)]
    gl = [Guarded(a, 310 + i) if a is not None else None for i, a in enumerate(rlast)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    reps = [(0, w[i].ptr, s[i].ptr, gg[i].ptr, gl[i].ptr if gl[i] is not None else None, 1, int(i in stepping),
             rates[i]) for i in range(total)]
    plan.elastic_step_and_optimise([stream.cuda_stream], [z.ptr], reps, ALPHA, rmom, wd, first, 0 if c.keep else DISCARD)
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    for i in sorted(stepping):
        O.sma_optimise(np.float32(-rates[i]), rmom, wd, want.w[i], grad[i], rlast[i], want.s[i])
    AV.elastic_average(want)
    for i, (sv, gr) in kept.items():
        want.s[i], grad[i] = sv, gr
    stream.synchronize()
    z.check(want.z[0], "z")
    for i in range(total):
        w[i].check(want.w[i], f"w[{i}]")
        s[i].check(want.s[i], f"s[{i}]")
        gg[i].check(grad[i], f"g[{i}]")
        if gl[i] is not None:
            gl[i].check(rlast[i], f"last[{i}]")


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_case_bitexact(group):
    cases = GROUPS[group]
    cus = _num_cus()
    fails = Failures(cus)
    n = cases[0].elements(cus)
    if cases[0].door == "context":
        import crossbow_amd
        # a group's context has the stepping replicas' pair; cases in which nobody steps ride the plain one
        momentum, wd = (MOMENTUM if cases[0].rep_mom else 0.0), (WD if cases[0].wd else 0.0)
        g = _context(n, crossbow_amd.UPDATE_SYNCHRONOUSEAMSGD, momentum, wd, elastic=True)
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
    from tests.test_instantiations_elastic_steps import compiled_kernels
    assert set(IE.case_names(_num_cus())) == compiled_kernels()
