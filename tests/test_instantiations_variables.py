"""The case table of tests/instantiations_variables.py against what
``libcrossbow_sma_variables.so`` compiles (CPU only: symbol names of the host
stubs, no device code is read): the compiled kernels are exactly the
instantiations the cases reach.  There is no list of unreachable or untested
kernels to hide behind: what no door reaches is not compiled."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from tests import instantiations as I
from tests import instantiations_variables as IV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma_variables.so")


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
    reached = IV.case_names(256)
    missing, surplus = sorted(compiled - set(reached)), sorted(set(reached) - compiled)
    print(f"compiled {len(compiled)}, reached {len(reached)} by {len(IV.CASES)} cases")
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are reached by no case (a door that cannot reach a form must not compile it):\n  "
        + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} kernels a case expects are not compiled:\n  " +
        "\n  ".join(f"{k}  <- {reached[k][0].name()}" for k in surplus[:40]))
    assert not hasattr(IV, "UNREACHABLE") and not hasattr(IV, "UNTESTED")
    # 9 rungs x 8 all-step forms + 16 mixed forms, for (policy, unroll) in 2 x 2 without a tail and once with
    # one; less the 6 forms of base momentum beside momentum-free weight-decayed steps that only the seam reaches
    assert len(compiled) == 88 * 5 - 6


def test_every_kernel_is_the_one_family():
    for k in compiled_kernels():
        assert re.fullmatch(IV.KERNEL + r"<-?\d, (true|false), (true|false), (true|false), (true|false), "
                            r"(true|false), [01], (true|false), [12]>", k), k


def test_the_model_places_every_case_at_other_cu_counts():
    for cus in (64, 104, 228, 256, 304):
        for c in IV.CASES:
            assert IV.expected_kernel(c, cus) == IV.expected_kernel(c, 256), (cus, c.name())


def test_the_ladders_are_the_plain_barriers():
    # the new launcher repeats launch_task_barrier's ladders: the same template arguments for every case
    for c in IV.CASES:
        plain = I.expected_kernel(I.Case(**{**c.__dict__, "n": I.N_CTX}) if c.door == "context" else c, 256)
        assert IV.expected_kernel(c, 256) == plain.replace("task_barrier_kernel", IV.KERNEL), c.name()


def test_variables_of_every_case_tile_it():
    for c in IV.CASES:
        n = c.elements(256)
        variables, mults = IV.variables_for(n)
        assert sum(variables) == n and len(variables) == len(mults) and min(variables) >= 0, c.name()
        assert any(m != 1.0 for m in mults)
