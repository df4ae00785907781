"""Which compiled kernel of ``libcrossbow_sma_elastic_steps.so`` does a call reach?

The object holds one kernel family, ``task_elastic_kernel``
(crossbow_amd/csrc/task_elastic_kernels.hip), behind the two doors
``cbx_step_and_synchronise_elastic`` (the context, through ``TheGPU``, under
update model 3 with ``set_elastic_average``) and
``cbx_ea_plan_step_and_optimise`` (the seam, through ``SmaPlan``).  This module
is the suite's account of it, in the manner of tests/instantiations_clipped.py:

``CASES``       one call each, with everything the dispatch looks at: the cases
                of the plain fused barrier (tests/instantiations.py) without
                base momentum.  The elastic barrier has none and reads no copy
                flag, so both are taken out of every case, not only out of the
                table: kept as a plain filter, the momentum rungs would go,
                since that table steps every replica with momentum only where
                the base model has it too.  Cases that then coincide are one.
                tests/test_gpu_instantiations_elastic_steps.py runs every one
                against the oracle, bit for bit.
``expected_kernel(case, num_cus)``
                the dispatch restated in Python.

There is no UNREACHABLE and no UNTESTED list: what no door reaches is not
compiled (tests/test_instantiations_elastic_steps.py holds the cases to an exact
cover of the object's host stubs).  Plain Python: no torch, no GPU.
"""
from __future__ import annotations

from dataclasses import replace
from typing import Dict, List, Tuple

from tests import instantiations as I

Case = I.Case
KERNEL = "task_elastic_kernel"


def expected_kernel(case: Case, num_cus: int) -> str:
    """launch_task_elastic and the ladders above it (task_elastic_kernels.hip)."""
    if case.family != "task_barrier":
        raise ValueError(case.family)
    if case.base_mom or case.copy:
        raise ValueError("the elastic barrier has no base momentum and no Phase D")
    if case.steps != "none" and case.nrep == 0:
        raise ValueError("nobody to step")
    block, bpc, unroll, waves = I._main_cfg(case)
    n4, tail, P = I.bulk_float4s(case, num_cus), I.has_tail(case, num_cus), I._policy(case)
    stepping = case.steps != "none"
    mom = case.rep_mom and stepping  # the first stepping replica's, else 0 (context.hip, sma_seam.hip)
    wd = case.wd and stepping
    if case.nrep > 0 and case.steps == "all":  # te_form: every participating replica steps
        R, mixed = I._ladder(case.nrep, range(1, I.K_CHUNK + 1)), False
    else:
        R, mixed = -1, True
    u = I.small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # te_u
    if block > 256:
        raise I.Refused(f"block {block}")
    if tail:
        if P != 1 or u != 1:
            raise I.Refused("a tail has policy 1 and unroll 1")  # task_elastic_compiled
    elif u not in (1, 2):
        raise I.Refused(f"unroll {u}")
    b = I._b
    return f"{KERNEL}<{R}, {b(mixed)}, {b(mom)}, {b(wd)}, {b(case.keep)}, {P}, {b(tail)}, {u}>"


def expected_kernels(case: Case, num_cus: int) -> Tuple[str, ...]:
    return (expected_kernel(case, num_cus),)


def _cases() -> List[Case]:
    seen, out = set(), []
    for c in I._task_barrier_cases():
        c = replace(c, base_mom=False, copy=False)
        if c.steps == "none":
            c = replace(c, rep_mom=False, wd=False)  # nobody's momentum or weight decay to be had
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CASES: List[Case] = _cases()


def case_names(num_cus: int) -> Dict[str, List[Case]]:
    """{instantiation: [cases that reach it]} over CASES."""
    out: Dict[str, List[Case]] = {}
    for c in CASES:
        out.setdefault(expected_kernel(c, num_cus), []).append(c)
    return out
