"""Which compiled kernel of ``libcrossbow_sma_elastic_policies.so`` does a call reach?

The object holds three kernel families, one per step policy and compilation
unit: ``task_elastic_variables_kernel``, ``task_elastic_clipped_kernel`` and
``task_elastic_clipped_variables_kernel`` (the three
crossbow_amd/csrc/task_elastic_*_kernels.hip around task_elastic_policy_body.inc),
behind the two doors ``cbx_step_and_synchronise_elastic_clipped_variables`` (the
context, through ``TheGPU``, under update model 3 with ``set_elastic_average``)
and ``cbx_ea_plan_step_and_optimise_clipped_variables`` (the seam, through
``SmaPlan``).  Which family a call reaches is decided by what is on: gradient
clipping, per-variable rates, or both.  This module is the suite's account of
it, in the manner of tests/instantiations_elastic_steps.py:

``CASES``       (policy, case) pairs, one call each.  The cases are those of the
                plain fused elastic barrier (tests/instantiations_elastic_steps.py);
                the two clipped policies take the ones in which a replica steps,
                since a call in which nobody steps has nothing to clip and
                launches the per-variable or the plain kernel through either
                door.  tests/test_gpu_instantiations_elastic_policies.py runs
                every one against the oracle, bit for bit.
``expected_kernel(policy, case, num_cus)``
                the dispatch restated in Python.

There is no UNREACHABLE and no UNTESTED list: what no door reaches is not
compiled (tests/test_instantiations_elastic_policies.py holds the cases to an
exact, disjoint cover of the object's host stubs).  Plain Python: no torch, no GPU.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from tests import instantiations as I
from tests import instantiations_elastic_steps as IE

Case = I.Case
POLICIES = ("variables", "clipped", "clipped_variables")
KERNELS = {p: f"task_elastic_{p}_kernel" for p in POLICIES}


def clips(policy: str) -> bool:
    return policy in ("clipped", "clipped_variables")


def per_variable(policy: str) -> bool:
    return policy in ("variables", "clipped_variables")


def expected_kernel(policy: str, case: Case, num_cus: int) -> str:
    """launch_task_elastic_<policy> and the ladders above it (task_elastic_policy.h): te_form's, so the
    template arguments are those of the plain kernel the same call would reach with both features off."""
    if policy not in POLICIES:
        raise ValueError(policy)
    if clips(policy) and (case.steps == "none" or case.nrep == 0):
        raise ValueError("nobody steps: the doors launch task_elastic_variables_kernel or task_elastic_kernel")
    plain = IE.expected_kernel(case, num_cus)
    assert plain.startswith(IE.KERNEL + "<")
    return KERNELS[policy] + plain[len(IE.KERNEL):]


def _cases() -> List[Tuple[str, Case]]:
    out = []
    for p in POLICIES:
        for c in IE.CASES:
            if clips(p) and (c.steps == "none" or c.nrep == 0):
                continue
            out.append((p, c))
    return out


CASES: List[Tuple[str, Case]] = _cases()


def case_names(num_cus: int) -> Dict[str, List[Tuple[str, Case]]]:
    """{instantiation: [(policy, case) pairs that reach it]} over CASES."""
    out: Dict[str, List[Tuple[str, Case]]] = {}
    for p, c in CASES:
        out.setdefault(expected_kernel(p, c, num_cus), []).append((p, c))
    return out
