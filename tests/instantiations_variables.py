"""Which compiled kernel of ``libcrossbow_sma_variables.so`` does a call reach?

The object holds one kernel family, ``task_barrier_variables_kernel``
(crossbow_amd/csrc/task_barrier_variables_kernels.hip), behind the two doors
``cbx_step_and_synchronise_variables`` (the context, through ``TheGPU``) and
``cbx_sma_plan_step_and_optimise_variables`` (the seam, through ``SmaPlan``).
This module is the suite's account of it, in the manner of
tests/instantiations.py:

``CASES``       one call each, with everything the dispatch looks at: the cases
                of the plain fused barrier (tests/instantiations.py), whose
                ladders the launcher shares (task_barrier_launch.h), over a model of several
                variables (``variables_for``).
                tests/test_gpu_instantiations_variables.py runs every one
                against the oracle, bit for bit.
``expected_kernel(case, num_cus)``
                the dispatch restated in Python.

There is no UNREACHABLE and no UNTESTED list: what no door reaches is not
compiled (tests/test_instantiations_variables.py holds the cases to an exact
cover of the object's host stubs).  Plain Python: no torch, no GPU.

Line numbers are those of crossbow_amd/csrc at the commit that added this file.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from tests import instantiations as I

Case = I.Case
KERNEL = "task_barrier_variables_kernel"


def variables_for(n: int) -> Tuple[Tuple[int, ...], Tuple[float, ...]]:
    """The variables and multipliers of a case of ``n`` floats: the model of
    tests/test_optimise_plan.py where n is its size, else three variables with
    boundaries off the float4 grid (the third may be the only one of n < 3)."""
    from tests.test_optimise_plan import M, V
    if n == sum(V):
        return tuple(V), tuple(M)
    a = n // 3
    b = min(n - a, a + 1)
    return (a, b, n - a - b), (2.0, 0.5, 3.0)


def expected_kernel(case: Case, num_cus: int) -> str:
    """launch_task_barrier_variables: the ladders of task_barrier_launch.h, named by function, with what
    VariablesLauncher (task_barrier_variables_kernels.hip) says of a side object."""
    if case.family != "task_barrier":
        raise ValueError(case.family)
    block, bpc, unroll, waves = I._main_cfg(case)
    n4, tail, P = I.bulk_float4s(case, num_cus), I.has_tail(case, num_cus), I._policy(case)
    if case.steps != "none" and case.nrep == 0:
        raise ValueError("nobody to step")
    stepping = case.steps != "none"
    mom = case.rep_mom and stepping  # context.hip:796, sma_seam.hip:565: the first stepping replica's, else 0
    wd = case.wd and stepping
    # tb_form
    if case.nrep > 0 and case.steps == "all" and case.base_mom == mom:
        R, mixed, bmom = I._ladder(case.nrep, range(1, I.K_CHUNK + 1)), False, mom  # tb_form's switch
    else:
        R, mixed, bmom = -1, True, case.base_mom
    u = I.small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # tb_u
    if tail:
        if P != 1 or u != 1:
            raise I.Refused("a tail has policy 1 and unroll 1")  # task_barrier_compiled, kSideObject
        U = 1
    else:
        seam_only = mixed and not mom and bmom and wd  # VariablesLauncher::seam_only
        if u not in (1, 2) or (seam_only and (P != 1 or u != 1)):
            raise I.Refused(f"policy {P}, unroll {u}")  # tb_u, task_barrier_compiled
        U = u
    b = I._b
    return f"{KERNEL}<{R}, {b(mixed)}, {b(mom)}, {b(bmom)}, {b(wd)}, {b(case.keep)}, {P}, {b(tail)}, {U}>"


def expected_kernels(case: Case, num_cus: int) -> Tuple[str, ...]:
    return (expected_kernel(case, num_cus),)


def _cases() -> List[Case]:
    out = []
    for c in I._task_barrier_cases():
        n = c.n
        if c.door == "context":
            n = I.N_VARS  # the seven variables of tests/test_optimise_plan.py, padded to 24,576
        out.append(Case(**{**c.__dict__, "n": n}))
    return out


CASES: List[Case] = _cases()


def case_names(num_cus: int) -> Dict[str, List[Case]]:
    """{instantiation: [cases that reach it]} over CASES."""
    out: Dict[str, List[Case]] = {}
    for c in CASES:
        out.setdefault(expected_kernel(c, num_cus), []).append(c)
    return out
