"""The case table of tests/instantiations_elastic_policies.py against what
``libcrossbow_sma_elastic_policies.so`` compiles (CPU only: symbol names of the
host stubs, no device code is read): the compiled kernels are exactly the
instantiations the cases reach, policy by policy.  There is no list of
unreachable or untested kernels to hide behind: what no door reaches is not
compiled."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from tests import instantiations as I
from tests import instantiations_elastic_policies as IP
from tests import instantiations_elastic_steps as IE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma_elastic_policies.so")


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
    reached = IP.case_names(256)
    missing, surplus = sorted(compiled - set(reached)), sorted(set(reached) - compiled)
    print(f"compiled {len(compiled)}, reached {len(reached)} by {len(IP.CASES)} cases")
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are reached by no case (a door that cannot reach a form must not compile it):\n  "
        + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} kernels a case expects are not compiled:\n  " +
        "\n  ".join(f"{k}  <- {reached[k][0][0]} {reached[k][0][1].name()}" for k in surplus[:40]))
    assert not hasattr(IP, "UNREACHABLE") and not hasattr(IP, "UNTESTED")
    # per policy: (9 rungs + the mixed form) x 4 pairs of (momentum, weight decay) x kept or discarded, for
    # (policy, unroll) in 2 x 2 without a tail and once with one
    assert len(compiled) == 3 * 10 * 4 * 2 * 5


def test_the_cover_is_disjoint_policy_by_policy():
    compiled = compiled_kernels()
    by_policy = {p: {k for k in compiled if k.startswith(IP.KERNELS[p] + "<")} for p in IP.POLICIES}
    assert sum(len(v) for v in by_policy.values()) == len(compiled)
    for p in IP.POLICIES:
        reached = {IP.expected_kernel(q, c, 256) for q, c in IP.CASES if q == p}
        assert reached == by_policy[p], p
        assert len(reached) == 400, p
        # a policy's forms are the plain kernel's, argument list by argument list
        assert {k[len(IP.KERNELS[p]):] for k in reached} == {k[len(IE.KERNEL):] for k in IE.case_names(256)}, p


def test_every_kernel_is_one_of_the_three_families():
    names = "|".join(IP.KERNELS[p] for p in IP.POLICIES)
    for k in compiled_kernels():
        assert re.fullmatch(r"(%s)<-?\d, (true|false), (true|false), (true|false), (true|false), [01], "
                            r"(true|false), [12]>" % names, k), k


def test_the_model_places_every_case_at_other_cu_counts():
    for cus in (64, 104, 228, 256, 304):
        for p, c in IP.CASES:
            assert IP.expected_kernel(p, c, cus) == IP.expected_kernel(p, c, 256), (cus, p, c.name())


def test_the_clipped_policies_have_no_case_in_which_nobody_steps():
    assert any(c.steps == "none" for p, c in IP.CASES if p == "variables")
    assert all(c.steps != "none" and c.nrep > 0 for p, c in IP.CASES if IP.clips(p))
    with pytest.raises(ValueError):
        IP.expected_kernel("clipped", next(c for c in IE.CASES if c.steps == "none"), 256)
    # every plain elastic case is a case of the per-variable policy, and every stepping one of the other two
    assert [c for p, c in IP.CASES if p == "variables"] == IE.CASES
    for p in ("clipped", "clipped_variables"):
        assert [c for q, c in IP.CASES if q == p] == [c for c in IE.CASES if c.steps != "none" and c.nrep > 0]
