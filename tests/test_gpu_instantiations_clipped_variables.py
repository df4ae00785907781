"""Every case of tests/instantiations_clipped_variables.py against the oracle,
bit for bit (run with -m gpu): one call through
``cbx_step_and_synchronise_clipped_variables`` or
``cbx_sma_plan_step_and_optimise_clipped_variables`` per case, so that every
kernel ``libcrossbow_sma_clipped_variables.so`` compiles runs against
``tests.gradient_clip_common.decide`` and ``step(..., variables=, mults=)`` and
``O.sma_step``.

The stepping replicas take gradients whose S is exact in any order and whose
clipped scale is 0.5 (tests/test_gpu_step_and_synchronise_clipped.py's
``gradient``, as tests/test_gpu_instantiations_clipped.py), so no device value
enters an expectation; in id order they come out unclipped, clipped and
skipped, so every kernel meets all three.  The variables and multipliers of a
size are tests/instantiations_variables.py's (``variables_for``).  The inputs,
the sentinels in output-only buffers and the sharing of one context or plan per
group are tests/test_gpu_instantiations.py's.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests import instantiations as I
from tests import instantiations_clipped_variables as ICV
from tests import instantiations_variables as IV
from tests.helpers import Guarded, assert_bitexact, compare_states, download, upload
from tests.test_gpu_instantiations import (ALPHA, CLOCK, DISCARD, MOMENTUM, WD, R, _configure, _fill, _num_cus,
                                           _sentinel, _set_copies, _state, _steps)
from tests.test_gpu_instantiations_clipped import _gradients
from tests.test_gpu_instantiations_variables import _context

pytestmark = pytest.mark.gpu


def _group(c: I.Case) -> str:
    key = [c.door]
    if c.door == "context":
        key.append(("mom" if c.rep_mom else "nomom") + ("-wd" if c.wd else ""))
    else:
        key.append(str(c.n))
    return "-".join(key)


GROUPS: "OrderedDict[str, list]" = OrderedDict()
for _c in ICV.CASES:
    GROUPS.setdefault(_group(_c), []).append(_c)


class Failures:
    def __init__(self, cus):
        self.cus, self.bad, self.ran = cus, [], 0

    def run(self, case, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{case.name()} -> {ICV.expected_kernel(case, self.cus)}: {e}")

    def done(self):
        assert self.ran > 0
        assert not self.bad, f"{len(self.bad)} of {self.ran} cases differ from the oracle:\n" + "\n".join(self.bad[:40])


def _expected_steps(want, grad, rlast, stepping, rates, momentum, wd, max_norm, variables, mults):
    flags_of = {}
    for i in sorted(stepping):
        S, K = C.exact_sum_sq(grad[i])
        scale, flags = C.decide(S, K, max_norm, True)
        flags_of[i] = flags
        C.step([want.w[i], grad[i], rlast[i], want.s[i]], scale, flags, momentum, wd, lr=rates[i],
               variables=variables, mults=mults)
    return flags_of


def _context_case(g, c: I.Case, n: int, momentum: float, wd: float):
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    variables, mults = IV.variables_for(n)
    _configure(g, c)
    assert c.base_mom <= (momentum > 0)
    g.setMomentum(MOMENTUM if c.base_mom else 0.0, 0)  # bmom is read at the call
    max_norm = C.exact_gradient(n)[2]
    g.set_gradient_clip(max_norm, True)
    want = _state(n, R, MOMENTUM if c.base_mom else 0.0, with_last=momentum > 0)
    first = R - c.nrep
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    stepping = _steps(c, first, R)
    tasks = [3 + 2 * i if i in stepping else -1 for i in range(R)]
    rates = [g.replica_learning_rate(i, tasks[i]) if i in stepping else 0.0 for i in range(R)]
    grad, kinds = _gradients(n, stepping, R)
    rlast = [_fill(n, 5100 + i, 0.001).copy() if momentum > 0 else None for i in range(R)]
    for i in stepping:  # written only: s = w, or left alone under the discard flag
        want.s[i] = _sentinel(n, 100 + i).copy()
    upload(g, want)
    _set_copies(g, want)
    for i in range(R):
        g.replica_write(i, BUF_GRADIENT, grad[i])
        if rlast[i] is not None:
            g.replica_write(i, BUF_LAST, rlast[i])
    g.lockAny()
    g.step_and_synchronise_clipped_variables(first, CLOCK, 0, tasks, None, 0 if c.keep else DISCARD)
    g.unlockAny()
    g.wait()
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    flags_of = _expected_steps(want, grad, rlast, stepping, rates, momentum, wd, max_norm, variables, mults)
    assert all(bool(flags_of[i] & C.SKIPPED) == (kinds[i] == "skipped") for i in stepping)
    O.sma_step(want)
    for i, (s, gr) in kept.items():
        want.s[i], grad[i] = s, gr
    compare_states(download(g, want), want)
    for i in range(R):
        assert_bitexact(g.replica_read(i, BUF_GRADIENT), grad[i], f"g[{i}]")
        if rlast[i] is not None:
            assert_bitexact(g.replica_read(i, BUF_LAST), rlast[i], f"last[{i}]")
    assert [g.replica_copy(i) for i in range(R)] == [0] * R, "copy flags after the step"


def _seam_case(plan, c: I.Case, n: int):
    import torch
    variables, mults = IV.variables_for(n)
    total, first = c.nrep + 1, 1  # one replica below `first` stays outside the step
    want = _state(n, total, MOMENTUM if c.base_mom else 0.0, with_last=c.base_mom)
    want.first = first
    if c.copy:
        want.copy[first + c.nrep // 2] = 1
    stepping = _steps(c, first, total)
    rmom = MOMENTUM if c.rep_mom else 0.0
    wd = WD if c.wd else 0.0
    max_norm = C.exact_gradient(n)[2]
    rates = [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(total)]
    for i in stepping:
        want.s[i] = _sentinel(n, 100 + i).copy()
    z = Guarded(want.z[0], 1)
    blast = Guarded(want.last[0], 2) if want.last is not None else None
    w = [Guarded(a, 10 + i) for i, a in enumerate(want.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(want.s)]
    grad, kinds = _gradients(n, stepping, total)
    rlast = [_fill(n, 5100 + i, 0.001).copy() if rmom > 0 else None for i in range(total)]
    gg = [Guarded(a, 210 + i) for i, a in enumerate(grad)]
    gl = [Guarded(a, 310 + i) if a is not None else None for i, a in enumerate(rlast)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    reps = [(0, w[i].ptr, s[i].ptr, gg[i].ptr, gl[i].ptr if gl[i] is not None else None, 1, int(want.copy[i]),
             int(i in stepping), rates[i]) for i in range(total)]
    got = plan.step_and_optimise_clipped_variables(
        [stream.cuda_stream], [z.ptr], [blast.ptr] if blast is not None else None, reps, ALPHA,
        MOMENTUM if c.base_mom else 0.0, rmom, wd, first, 0 if c.keep else DISCARD, slots=list(range(total)),
        max_norm=max_norm, skip_nonfinite=True)
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    flags_of = _expected_steps(want, grad, rlast, stepping, rates, rmom, wd, max_norm, variables, mults)
    assert all(bool(flags_of[i] & C.SKIPPED) == (kinds[i] == "skipped") for i in stepping)
    exp = 1 if O.sma_step(want) > 0 else 0
    for i, (sv, gr) in kept.items():
        want.s[i], grad[i] = sv, gr
    stream.synchronize()
    assert got == exp, f"return value {got}, the oracle's {exp}"
    z.check(want.z[0], "z")
    if blast is not None:
        blast.check(want.last[0], "base last")
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
        momentum, wd = (MOMENTUM if cases[0].rep_mom else 0.0), (WD if cases[0].wd else 0.0)
        g = _context(n, momentum, wd)  # one operator per variable, the switch on
        try:
            for c in cases:
                fails.run(c, lambda: _context_case(g, c, n, momentum, wd))
        finally:
            g.free()
    else:
        from crossbow_amd.seam import SmaPlan
        variables, mults = IV.variables_for(n)
        with SmaPlan([0], n) as plan:
            plan.set_variables(list(variables), list(mults))
            for c in cases:
                fails.run(c, lambda: _seam_case(plan, c, n))
    fails.done()


def test_the_cases_reach_every_compiled_kernel_on_this_device():
    from tests.test_instantiations_clipped_variables import compiled_kernels
    assert set(ICV.case_names(_num_cus())) == compiled_kernels()
