"""The case table of tests/instantiations_elastic_steps.py against what
``libcrossbow_sma_elastic_steps.so`` compiles (CPU only: symbol names of the
host stubs, no device code is read): the compiled kernels are exactly the
instantiations the cases reach.  There is no list of unreachable or untested
kernels to hide behind: what no door reaches is not compiled."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from tests import instantiations as I
from tests import instantiations_elastic_steps as IE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma_elastic_steps.so")


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
    reached = IE.case_names(256)
    missing, surplus = sorted(compiled - set(reached)), sorted(set(reached) - compiled)
    print(f"compiled {len(compiled)}, reached {len(reached)} by {len(IE.CASES)} cases")
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are reached by no case (a door that cannot reach a form must not compile it):\n  "
        + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} kernels a case expects are not compiled:\n  " +
        "\n  ".join(f"{k}  <- {reached[k][0].name()}" for k in surplus[:40]))
    assert not hasattr(IE, "UNREACHABLE") and not hasattr(IE, "UNTESTED")
    # (9 rungs + the mixed form) x 4 pairs of (momentum, weight decay) x kept or discarded, for (policy, unroll)
    # in 2 x 2 without a tail and once with one
    assert len(compiled) == 10 * 4 * 2 * 5


def test_every_kernel_is_the_one_family():
    for k in compiled_kernels():
        assert re.fullmatch(IE.KERNEL + r"<-?\d, (true|false), (true|false), (true|false), (true|false), [01], "
                            r"(true|false), [12]>", k), k


def test_the_model_places_every_case_at_other_cu_counts():
    for cus in (64, 104, 228, 256, 304):
        for c in IE.CASES:
            assert IE.expected_kernel(c, cus) == IE.expected_kernel(c, 256), (cus, c.name())


def test_the_cases_are_the_plain_barriers_without_base_momentum():
    plain = I._task_barrier_cases()
    assert all(not c.base_mom and not c.copy for c in IE.CASES)
    # every plain case without base momentum and without a copy request that steps is a case here as it stands
    for c in plain:
        if not c.base_mom and not c.copy and c.steps != "none":
            assert c in IE.CASES, c.name()
    # and every case here is a plain case with the two taken out
    keys = {(c.door, c.n, c.nrep, c.steps, c.rep_mom and c.steps != "none", c.wd and c.steps != "none", c.keep,
             c.policy, c.cfg) for c in plain}
    for c in IE.CASES:
        assert (c.door, c.n, c.nrep, c.steps, c.rep_mom, c.wd, c.keep, c.policy, c.cfg) in keys, c.name()


def test_the_unrolled_path_does_not_hang_on_base_momentum():
    # task_barrier_launch.h takes its unrolled path on bmom == MOM; this ladder on "every replica steps" alone
    c = next(c for c in IE.CASES if c.steps == "all" and c.rep_mom and c.nrep == 4 and c.door == "context")
    assert IE.expected_kernel(c, 256).startswith(IE.KERNEL + "<4, false, true, ")
    with pytest.raises(ValueError):
        IE.expected_kernel(next(c for c in I._task_barrier_cases() if c.base_mom), 256)
