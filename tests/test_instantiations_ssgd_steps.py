"""The case table of tests/instantiations_ssgd_steps.py against what
``libcrossbow_sma_ssgd_steps.so`` compiles (CPU only: symbol names of the host
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
from tests import instantiations_ssgd_steps as IS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma_ssgd_steps.so")


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
    reached = IS.case_names(256)
    missing, surplus = sorted(compiled - set(reached)), sorted(set(reached) - compiled)
    print(f"compiled {len(compiled)}, reached {len(reached)} by {len(IS.CASES)} cases")
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are reached by no case (a door that cannot reach a form must not compile it):\n  "
        + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} kernels a case expects are not compiled:\n  " +
        "\n  ".join(f"{k}  <- {reached[k][0].name()}" for k in surplus[:40]))
    assert not hasattr(IS, "UNREACHABLE") and not hasattr(IS, "UNTESTED")
    # (9 stepping counts x {no weight decay, weight decay kept, weight decay discarded} + nobody stepping) x base
    # momentum on or off, for (policy, unroll) in 2 x 2 without a tail and once with one
    assert len(compiled) == (9 * 3 + 1) * 2 * 5


def test_every_kernel_is_the_one_family():
    for k in compiled_kernels():
        m = re.fullmatch(IS.KERNEL + r"<(-?\d), (true|false), (true|false), (true|false), ([01]), (true|false), ([12])>", k)
        assert m, k
        S, wd, keep, _, P, tail, U = m.groups()
        assert not (keep == "true" and wd == "false"), k  # without weight decay kept and discarded are one kernel
        assert not (S == "0" and wd == "true"), k           # nobody steps: nobody's weight decay
        assert tail == "false" or (P, U) == ("1", "1"), k   # the seam's shape


def test_the_model_places_every_case_at_other_cu_counts():
    for cus in (64, 104, 228, 256, 304):
        for c in IS.CASES:
            assert IS.expected_kernel(c, cus) == IS.expected_kernel(c, 256), (cus, c.name())


def test_the_ladder():
    def of(nrep, steps, **kw):
        return IS.expected_kernel(I.Case("task_barrier", "context", I.N_CTX, nrep, steps=steps, cfg=I.TB_FORCED[1], **kw), 256)
    # the stepping count picks the rung, not the receiving count: 5 of 9 step
    assert of(9, "some", wd=True).startswith(IS.KERNEL + "<5, true, true, false")
    assert of(9, "all", wd=True).startswith(IS.KERNEL + "<-1, true, true, false")
    assert of(8, "all", base_mom=True).startswith(IS.KERNEL + "<8, false, false, true")
    # nobody steps: the barrier alone, whatever the replicas' weight decay
    assert of(3, "none", wd=True) == of(3, "none") == of(0, "none")
    # the discard flag selects another kernel only with weight decay
    assert of(4, "all", keep=False) == of(4, "all")
    assert of(4, "all", wd=True, keep=False) != of(4, "all", wd=True)
    with pytest.raises(ValueError):
        of(4, "all", rep_mom=True)
    with pytest.raises(ValueError):
        of(4, "all", copy=True)


def test_the_cases_are_disjoint_from_the_other_objects_families():
    assert all(IS.expected_kernel(c, 256).startswith(IS.KERNEL + "<") for c in IS.CASES)
    assert len(set(IS.CASES)) == len(IS.CASES)
