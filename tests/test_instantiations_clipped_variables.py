"""The case table of tests/instantiations_clipped_variables.py against what
``libcrossbow_sma_clipped_variables.so`` compiles (CPU only: symbol names of
the host stubs, no device code is read): the compiled kernels are exactly the
instantiations the cases reach.  There is no list of unreachable or untested
kernels to hide behind: what no door reaches is not compiled."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from tests import instantiations as I
from tests import instantiations_clipped_variables as ICV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma_clipped_variables.so")


def compiled_kernels():
    tools = [[t, "-C", "--defined-only", LIB] for t in (shutil.which("nm"), "/opt/rocm/llvm/bin/llvm-nm") if t and os.path.exists(t)]
    if not tools:
        pytest.fail("neither binutils nm nor ROCm's llvm-nm is here")
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is not built (python __graft_entry__.py builds it)")
    out = subprocess.run(tools[0], check=True, capture_output=True, text=True).stdout
    return {I.normalise(line.split(None, 2)[2]) for line in out.splitlines() if I.STUB in line}


def test_exact_cover():
    compiled = compiled_kernels()
    reached = ICV.case_names(256)
    missing, surplus = sorted(compiled - set(reached)), sorted(set(reached) - compiled)
    print(f"compiled {len(compiled)}, reached {len(reached)} by {len(ICV.CASES)} cases")
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are reached by no case (a door that cannot reach a form must not compile it):\n  "
        + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} kernels a case expects are not compiled:\n  " +
        "\n  ".join(f"{k}  <- {reached[k][0].name()}" for k in surplus[:40]))
    assert not hasattr(ICV, "UNREACHABLE") and not hasattr(ICV, "UNTESTED")
    # 9 rungs x 8 all-step forms + 16 mixed forms, for (policy, unroll) in 2 x 2 without a tail and once with
    # one; less the 12 forms of base momentum beside momentum-free steps that only the seam's shape reaches
    assert len(compiled) == 88 * 5 - 12


def test_every_kernel_is_the_one_family():
    for k in compiled_kernels():
        assert re.fullmatch(ICV.KERNEL + r"<-?\d, (true|false), (true|false), (true|false), (true|false), "
                            r"(true|false), [01], (true|false), [12]>", k), k


def test_the_model_places_every_case_at_other_cu_counts():
    for cus in (64, 104, 228, 256, 304):
        for c in ICV.CASES:
            assert ICV.expected_kernel(c, cus) == ICV.expected_kernel(c, 256), (cus, c.name())


def test_the_ladders_are_the_plain_barriers():
    # the new launcher repeats launch_task_barrier's ladders: the same template arguments for every case
    for c in ICV.CASES:
        assert ICV.expected_kernel(c, 256) == I.expected_kernel(c, 256).replace("task_barrier_kernel", ICV.KERNEL), c.name()


def test_a_call_in_which_nobody_steps_is_no_case():
    c = next(c for c in I._task_barrier_cases() if c.steps == "none")
    with pytest.raises(ValueError):
        ICV.expected_kernel(c, 256)
