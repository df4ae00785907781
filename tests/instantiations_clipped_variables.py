"""Which compiled kernel of ``libcrossbow_sma_clipped_variables.so`` does a call
reach?

The object holds one kernel family, ``task_barrier_clipped_variables_kernel``
(crossbow_amd/csrc/task_barrier_clipped_variables_kernels.hip), behind the two
doors ``cbx_step_and_synchronise_clipped_variables`` (the context, through
``TheGPU``, with ``cbx_set_gradient_clip`` on and a multiplier that is not 1)
and ``cbx_sma_plan_step_and_optimise_clipped_variables`` (the seam, through
``SmaPlan`` after ``set_variables``).  This module is the suite's account of
it, in the manner of tests/instantiations_clipped.py:

``CASES``       one call each, with everything the dispatch looks at: the cases
                of the plain fused barrier (tests/instantiations.py) in which a
                replica steps.  A call in which nobody steps has nothing to
                clip and launches the per-variable kernel (or the plain one),
                through either door.
                tests/test_gpu_instantiations_clipped_variables.py runs every
                one against the oracle, bit for bit.
``expected_kernel(case, num_cus)``
                the dispatch restated in Python.

There is no UNREACHABLE and no UNTESTED list: what no door reaches is not
compiled (tests/test_instantiations_clipped_variables.py holds the cases to an
exact cover of the object's host stubs).  Plain Python: no torch, no GPU.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from tests import instantiations as I

Case = I.Case
KERNEL = "task_barrier_clipped_variables_kernel"


def expected_kernel(case: Case, num_cus: int) -> str:
    """launch_task_barrier_clipped_variables and the ladders above it."""
    if case.family != "task_barrier":
        raise ValueError(case.family)
    if case.steps == "none" or case.nrep == 0:
        raise ValueError("nobody steps: the doors launch task_barrier_variables_kernel or task_barrier_kernel")
    block, bpc, unroll, waves = I._main_cfg(case)
    n4, tail, P = I.bulk_float4s(case, num_cus), I.has_tail(case, num_cus), I._policy(case)
    mom, wd = case.rep_mom, case.wd  # the first stepping replica's
    if case.steps == "all" and case.base_mom == mom:  # tb_form (task_barrier_launch.h)
        R, mixed, bmom = I._ladder(case.nrep, range(1, I.K_CHUNK + 1)), False, mom  # tb_form's switch
    else:
        R, mixed, bmom = -1, True, case.base_mom
    u = I.small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # tb_u
    if tail:
        if P != 1 or u != 1:
            raise I.Refused("a tail has policy 1 and unroll 1")
        U = 1
    else:
        # base momentum beside momentum-free steps: no context has it, the seam's shape only (the clipped
        # object's rule: weight decay does not narrow it, since a call in which nobody steps is no case)
        seam_only = mixed and not mom and bmom
        if u not in (1, 2) or (seam_only and (P != 1 or u != 1)):
            raise I.Refused(f"policy {P}, unroll {u}")
        U = u
    b = I._b
    return f"{KERNEL}<{R}, {b(mixed)}, {b(mom)}, {b(bmom)}, {b(wd)}, {b(case.keep)}, {P}, {b(tail)}, {U}>"


def expected_kernels(case: Case, num_cus: int) -> Tuple[str, ...]:
    return (expected_kernel(case, num_cus),)


CASES: List[Case] = [c for c in I._task_barrier_cases() if c.steps != "none" and c.nrep > 0]


def case_names(num_cus: int) -> Dict[str, List[Case]]:
    """{instantiation: [cases that reach it]} over CASES."""
    out: Dict[str, List[Case]] = {}
    for c in CASES:
        out.setdefault(expected_kernel(c, num_cus), []).append(c)
    return out
