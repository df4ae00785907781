"""Every case of tests/instantiations_elastic_policies.py against the oracle,
bit for bit (run with -m gpu): one call through
``cbx_step_and_synchronise_elastic_clipped_variables`` or
``cbx_ea_plan_step_and_optimise_clipped_variables`` per (policy, case), so that
every kernel ``libcrossbow_sma_elastic_policies.so`` compiles runs against the
host's step (``tests.test_optimise_plan.per_variable_step``, or
``tests.gradient_clip_common.decide`` and ``step``) and
``tests.averaging_common.elastic_average``.

Under the two clipped policies the stepping replicas take gradients whose S is
exact in any order and whose clipped scale is 0.5
(tests/test_gpu_instantiations_clipped.py's ``_gradients``), so no device value
enters an expectation; in id order they come out unclipped, clipped and
skipped.  The variables and multipliers of a size are
tests/instantiations_variables.py's (``variables_for``).  The inputs, the
sentinels in output-only buffers and the sharing of one context or plan per
group are tests/test_gpu_instantiations.py's.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest

from tests import averaging_common as AV
from tests import gradient_clip_common as C
from tests import instantiations as I
from tests import instantiations_elastic_policies as IP
from tests import instantiations_variables as IV
from tests.helpers import Guarded, assert_bitexact, compare_states, download, upload
from tests.test_gpu_instantiations import (ALPHA, CLOCK, DISCARD, MOMENTUM, WD, WPC, R, _configure, _fill, _num_cus,
                                           _sentinel, _state, _steps)
from tests.test_gpu_instantiations_clipped import _gradients
from tests.test_optimise_plan import per_variable_step

pytestmark = pytest.mark.gpu


def _group(p: str, c: I.Case) -> str:
    key = [p, c.door]
    if c.door == "context":
        key.append(("mom" if c.rep_mom else "nomom") + ("-wd" if c.wd else ""))
    else:
        key.append(str(c.n))
    return "-".join(key)


GROUPS: "OrderedDict[str, list]" = OrderedDict()
for _p, _c in IP.CASES:
    GROUPS.setdefault(_group(_p, _c), []).append((_p, _c))


class Failures:
    def __init__(self, cus):
        self.cus, self.bad, self.ran = cus, [], 0

    def run(self, policy, case, fn):
        self.ran += 1
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{policy} {case.name()} -> {IP.expected_kernel(policy, case, self.cus)}: {e}")

    def done(self):
        assert self.ran > 0
        assert not self.bad, f"{len(self.bad)} of {self.ran} cases differ from the oracle:\n" + "\n".join(self.bad[:40])


def _layout(policy, n):
    """(variables, multipliers) of the model, and what the expected step reads of them."""
    variables, mults = IV.variables_for(n)
    return variables, mults, (variables if IP.per_variable(policy) else None), (mults if IP.per_variable(policy) else None)


def _context(policy, n, momentum, wd):
    import crossbow_amd
    variables, mults, _, _ = _layout(policy, n)
    g = crossbow_amd.TheGPU()
    g.init([0])
    try:
        g.setModel(len(variables), 4 * n)
        for v, count in enumerate(variables):
            g.setModelVariable(v, 1, [count], 4 * count)
            g.setModelVariableLearningRateMultiplier(v, 1, mults[v])
        g.setUpdateModelType(crossbow_amd.UPDATE_SYNCHRONOUSEAMSGD)
        g.setElasticAverage(True)
        g.setEamsgdAlpha(ALPHA)
        g.setMomentum(momentum, 0)
        g.setWeightDecay(wd)
        g.setLearningRateDecayPolicyExp(0.05, 0.97)
        g.setModelWorkPerClock(WPC)
        g.setModelManager(R, 0)
        g.set_variable_learning_rates(IP.per_variable(policy))  # off: the multipliers are not read
        if IP.clips(policy):
            g.set_gradient_clip(C.exact_gradient(n)[2], True)
    except Exception:
        g.free()
        raise
    return g


def _expected(policy, want, grad, rlast, stepping, rates, momentum, wd, max_norm, variables, mults, kinds):
    """The stepping replicas' steps in id order, then the barrier."""
    for i in sorted(stepping):
        if IP.clips(policy):
            S, K = C.exact_sum_sq(grad[i])
            scale, flags = C.decide(S, K, max_norm, True)
            assert bool(flags & C.SKIPPED) == (kinds[i] == "skipped")
            C.step([want.w[i], grad[i], rlast[i], want.s[i]], scale, flags, momentum, wd, lr=rates[i],
                   variables=variables, mults=mults)
        else:
            per_variable_step(rates[i], mults, momentum, wd, want.w[i], grad[i], rlast[i], want.s[i],
                              variables=variables)
    AV.elastic_average(want)


def _inputs(policy, n, stepping, total, momentum):
    if IP.clips(policy):
        grad, kinds = _gradients(n, stepping, total)
    else:
        grad, kinds = [_fill(n, 5000 + i, 0.01).copy() for i in range(total)], {}
    rlast = [_fill(n, 5100 + i, 0.001).copy() if momentum > 0 else None for i in range(total)]
    return grad, kinds, rlast


def _context_case(g, policy, c: I.Case, n: int, momentum: float, wd: float):
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    _, _, variables, mults = _layout(policy, n)
    _configure(g, c)
    max_norm = C.exact_gradient(n)[2]
    want = _state(n, R, 0.0, with_last=momentum > 0)  # the base `last` exists with momentum and is left alone
    first = R - c.nrep
    want.first = first
    stepping = _steps(c, first, R)
    tasks = [3 + 2 * i if i in stepping else -1 for i in range(R)]
    rates = [g.replica_learning_rate(i, tasks[i]) if i in stepping else 0.0 for i in range(R)]
    grad, kinds, rlast = _inputs(policy, n, stepping, R, momentum)
    for i in range(first, R):  # never read: written (s = w) by a stepping replica whose outputs are kept
        want.s[i] = _sentinel(n, 100 + i).copy()
    upload(g, want)
    for i in range(R):
        g.replica_write(i, BUF_GRADIENT, grad[i])
        if rlast[i] is not None:
            g.replica_write(i, BUF_LAST, rlast[i])
    g.lockAny()
    g.step_and_synchronise_elastic_clipped_variables(first, CLOCK, 0, tasks, None, 0 if c.keep else DISCARD)
    g.unlockAny()
    g.wait()
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    with np.errstate(all="ignore"):
        _expected(policy, want, grad, rlast, stepping, rates, momentum, wd, max_norm, variables, mults, kinds)
    for i, (s, gr) in kept.items():
        want.s[i], grad[i] = s, gr
    compare_states(download(g, want), want)
    for i in range(R):
        assert_bitexact(g.replica_read(i, BUF_GRADIENT), grad[i], f"g[{i}]")
        if rlast[i] is not None:
            assert_bitexact(g.replica_read(i, BUF_LAST), rlast[i], f"last[{i}]")


def _seam_case(plan, policy, c: I.Case, n: int):
    import torch
    _, _, variables, mults = _layout(policy, n)
    total, first = c.nrep + 1, 1  # one replica below `first` stays outside the step
    want = _state(n, total, 0.0, with_last=False)
    want.first = first
    stepping = _steps(c, first, total)
    rmom = MOMENTUM if c.rep_mom and stepping else 0.0
    wd = WD if c.wd and stepping else 0.0
    max_norm = C.exact_gradient(n)[2]
    rates = [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(total)]
    for i in range(first, total):
        want.s[i] = _sentinel(n, 100 + i).copy()
    z = Guarded(want.z[0], 1)
    w = [Guarded(a, 10 + i) for i, a in enumerate(want.w)]
    s = [Guarded(a, 110 + i) for i, a in enumerate(want.s)]
    grad, kinds, rlast = _inputs(policy, n, stepping, total, rmom)
    gg = [Guarded(a, 210 + i) for i, a in enumerate(grad)]
    gl = [Guarded(a, 310 + i) if a is not None else None for i, a in enumerate(rlast)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    reps = [(0, w[i].ptr, s[i].ptr, gg[i].ptr, gl[i].ptr if gl[i] is not None else None, 1, int(i in stepping),
             rates[i]) for i in range(total)]
    plan.elastic_step_and_optimise_clipped_variables(
        [stream.cuda_stream], [z.ptr], reps, ALPHA, rmom, wd, first, 0 if c.keep else DISCARD,
        slots=list(range(total)) if IP.clips(policy) else None, max_norm=max_norm, skip_nonfinite=True,
        use_variables=IP.per_variable(policy))
    kept = {i: (want.s[i].copy(), grad[i].copy()) for i in stepping if not c.keep}
    with np.errstate(all="ignore"):
        _expected(policy, want, grad, rlast, stepping, rates, rmom, wd, max_norm, variables, mults, kinds)
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
    policy, first_case = cases[0]
    cus = _num_cus()
    fails = Failures(cus)
    n = first_case.elements(cus)
    if first_case.door == "context":
        # a group's context has the stepping replicas' pair; cases in which nobody steps ride the plain one
        momentum, wd = (MOMENTUM if first_case.rep_mom else 0.0), (WD if first_case.wd else 0.0)
        g = _context(policy, n, momentum, wd)
        try:
            for p, c in cases:
                fails.run(p, c, lambda: _context_case(g, p, c, n, momentum, wd))
        finally:
            g.free()
    else:
        from crossbow_amd.seam import SmaPlan
        variables, mults, _, _ = _layout(policy, n)
        with SmaPlan([0], n) as plan:
            if IP.per_variable(policy):
                plan.set_variables(list(variables), list(mults))
            for p, c in cases:
                fails.run(p, c, lambda: _seam_case(plan, p, c, n))
    fails.done()


def test_the_cases_reach_every_compiled_kernel_on_this_device():
    from tests.test_instantiations_elastic_policies import compiled_kernels
    assert set(IP.case_names(_num_cus())) == compiled_kernels()
