"""Which compiled kernel of ``libcrossbow_sma_ssgd_steps.so`` does a call reach?

The object holds one kernel family, ``task_ssgd_kernel``
(crossbow_amd/csrc/task_ssgd_kernels.hip), behind the two doors
``cbx_step_and_synchronise_ssgd`` (the context, through ``TheGPU``, under update
model WORKER) and ``cbx_ssgd_plan_step_and_optimise`` (the seam, through
``SmaPlan``).  This module is the suite's account of it, in the manner of
tests/instantiations_elastic_steps.py:

``CASES``       one call each, with everything the dispatch looks at, as
                tests/instantiations.py's ``Case`` of family "task_barrier":
                ``nrep`` receiving replicas, of which all, every other one or
                none step; ``base_mom`` the base model's momentum; ``wd`` and
                ``keep`` the stepping replicas' weight decay and the discard
                flag.  Replica momentum and copy flags play no part under
                WORKER and are off in every case.
                tests/test_gpu_instantiations_ssgd_steps.py runs every one
                against the oracle, bit for bit.
``expected_kernel(case, num_cus)``
                the dispatch restated in Python.

There is no UNREACHABLE and no UNTESTED list: what no door reaches is not
compiled (tests/test_instantiations_ssgd_steps.py holds the cases to an exact
cover of the object's host stubs).  Plain Python: no torch, no GPU.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

from tests import instantiations as I

Case = I.Case
KERNEL = "task_ssgd_kernel"


def stepping_count(case: Case) -> int:
    """How many of the case's receiving replicas step: all, every other one
    (tests/test_gpu_instantiations.py's ``_steps``), or none."""
    return {"all": case.nrep, "some": (case.nrep + 1) // 2, "none": 0}[case.steps]


def expected_kernel(case: Case, num_cus: int) -> str:
    """launch_task_ssgd and the ladders above it (task_ssgd_kernels.hip)."""
    if case.family != "task_barrier":
        raise ValueError(case.family)
    if case.rep_mom or case.copy:
        raise ValueError("replica momentum and copy flags play no part in the S-SGD barrier")
    nstep = stepping_count(case)
    if case.steps != "none" and nstep == 0:
        raise ValueError("nobody to step")
    block, bpc, unroll, waves = I._main_cfg(case)
    n4, tail, P = I.bulk_float4s(case, num_cus), I.has_tail(case, num_cus), I._policy(case)
    S = I._ladder(nstep, range(0, I.K_CHUNK + 1))  # ts_conf, ts_form
    wd = case.wd and nstep > 0     # the first stepping replica's, else 0 (context.hip, sma_seam.hip)
    keep = case.keep and wd        # without weight decay the step writes no g: one kernel
    u = I.small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # ts_u
    if block > 256:
        raise I.Refused(f"block {block}")
    if tail:
        if P != 1 or u != 1:
            raise I.Refused("a tail has policy 1 and unroll 1")  # task_ssgd_compiled
    elif u not in (1, 2):
        raise I.Refused(f"unroll {u}")
    b = I._b
    return f"{KERNEL}<{S}, {b(wd)}, {b(keep)}, {b(case.base_mom)}, {P}, {b(tail)}, {u}>"


def expected_kernels(case: Case, num_cus: int) -> Tuple[str, ...]:
    return (expected_kernel(case, num_cus),)


def _cases() -> List[Case]:
    out = []

    def both_doors(nrep, steps, base_mom, wd, keep, seam_n):
        for P in (0, 1):
            for U in (1, 2):
                out.append(Case("task_barrier", "context", I.N_CTX, nrep, base_mom=base_mom, steps=steps, wd=wd,
                                keep=keep, policy=P, cfg=I.TB_FORCED[U]))
        out.append(Case("task_barrier", "seam", seam_n, nrep, base_mom=base_mom, steps=steps, wd=wd, keep=keep))

    for base_mom in (False, True):
        for wd, keep in ((False, True), (True, True), (True, False)):
            # every receiving replica steps: the rungs 1..8 and the chunked form at 9
            for nrep in I.R_ALL[:-1]:
                both_doors(nrep, "all", base_mom, wd, keep, I.N_SEAM[nrep % 2])
                if nrep in (9, 8, 3):
                    out.append(Case("task_barrier", "seam", I.N_TAIL_ONLY, nrep, base_mom=base_mom, steps="all", wd=wd,
                                    keep=keep))
            # every other one steps, the others only join: 5 of 9, 2 of 4
            both_doors(9, "some", base_mom, wd, keep, I.N_SEAM[1])
            out.append(Case("task_barrier", "seam", I.N_TAIL_ONLY, 4, base_mom=base_mom, steps="some", wd=wd, keep=keep))
        # the discard flag without weight decay: the same kernel as kept
        both_doors(4, "all", base_mom, False, False, I.N_SEAM[0])
        # nobody steps: the barrier alone; nobody at all
        for nrep in (3, 0):
            both_doors(nrep, "none", base_mom, False, True, I.N_SEAM[0])
        # without a tail the seam launches the context's form (policy 1, unroll 1)
        out.append(Case("task_barrier", "seam", 2048, 4, base_mom=base_mom, steps="all", wd=True))
    # the default configuration (its ragged trip counts at a larger n are
    # tests/test_gpu_step_and_synchronise_ssgd.py::test_grid_stride_shape_bitexact's, not repeated here)
    out.append(Case("task_barrier", "context", I.N_CTX, 9, base_mom=True, steps="all", wd=True))
    return out


CASES: List[Case] = _cases()


def case_names(num_cus: int) -> Dict[str, List[Case]]:
    """{instantiation: [cases that reach it]} over CASES."""
    out: Dict[str, List[Case]] = {}
    for c in CASES:
        out.setdefault(expected_kernel(c, num_cus), []).append(c)
    return out
