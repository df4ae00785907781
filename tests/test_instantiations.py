"""The case table of tests/instantiations.py against what the library compiles
(CPU only: symbol names of the host stubs, no device code is read).

* exact cover: the compiled kernels are exactly the instantiations the cases
  reach, plus UNREACHABLE, ELSEWHERE and the two UNTESTED copy kernels, and the
  lists are disjoint;
* the record of what a GPU run of tests/test_gpu_instantiations.py launched
  (profiles/instantiations/launched.json) agrees with the model.
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess

import pytest

from tests import instantiations as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "crossbow_amd", "libcrossbow_sma.so")
RECORD = os.path.join(ROOT, "profiles", "instantiations", "launched.json")
STUB = I.STUB


normalise = I.normalise


def compiled_kernels():
    tools = [[t, "-C", "--defined-only", LIB] for t in (shutil.which("nm"), "/opt/rocm/llvm/bin/llvm-nm") if t and os.path.exists(t)]
    if not tools:
        pytest.fail("neither binutils nm nor ROCm's llvm-nm is here")
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is not built (python __graft_entry__.py builds it)")
    out = subprocess.run(tools[0], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        if STUB not in line:
            continue
        names.add(normalise(line.split(None, 2)[2]))
    return names


@pytest.fixture(scope="module")
def compiled():
    return compiled_kernels()


def test_normalise():
    assert normalise("void cbx::(anonymous namespace)::__device_stub__sma_fused_kernel<-1, true, false, 1, true, 2>"
                     "(cbx::SmaArgs)") == "sma_fused_kernel<-1, true, false, 1, true, 2>"
    assert normalise("cbx::__device_stub__delay_kernel(unsigned long)") == "delay_kernel"
    assert normalise("void cbx::(anonymous namespace)::copy_kernel<1>(float __vector(4)*, float __vector(4) const*, long)"
                     ) == "copy_kernel<1>"
    assert normalise("void cbx::(anonymous namespace)::task_barrier_kernel<5,false,true,true,false,true,1,false,2>"
                     "(cbx::TaskBarrierArgs) [clone .kd]") == "task_barrier_kernel<5, false, true, true, false, true, 1, false, 2>"


def test_exact_cover(compiled):
    reached = set(I.case_names(256))
    sets = {"CASES": reached, "UNREACHABLE": set(I.UNREACHABLE), "ELSEWHERE": set(I.ELSEWHERE), "UNTESTED": set(I.UNTESTED)}
    names = list(sets)
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            both = sets[names[a]] & sets[names[b]]
            assert not both, f"{names[a]} and {names[b]} both list {sorted(both)[:10]} ({len(both)})"
    listed = set().union(*sets.values())
    missing, surplus = sorted(compiled - listed), sorted(listed - compiled)
    print(f"compiled {len(compiled)}: " + ", ".join(f"{k} {len(v)}" for k, v in sets.items()))
    assert not missing and not surplus, (
        f"{len(missing)} compiled kernels are in no list (a new instantiation needs a case):\n  " + "\n  ".join(missing[:40]) +
        f"\n{len(surplus)} listed kernels are not compiled (a case or a list names a kernel that does not exist):\n  " +
        "\n  ".join(f"{k}  <- {I.case_names(256)[k][0].name()}" if k in reached else k for k in surplus[:40]))
    assert len(compiled) == sum(len(v) for v in sets.values())


def test_every_reason_cites_a_line():
    for name, why in I.UNREACHABLE.items():
        assert re.search(r"\.(hip|h):\d+", why), f"UNREACHABLE[{name}] cites no source line: {why}"
    for name, why in I.ELSEWHERE.items():
        tests = re.findall(r"tests/[a-z_]+\.py", why)
        assert tests, f"{name}: no test named in {why!r}"
        for t in tests:
            assert os.path.exists(os.path.join(ROOT, t)), f"{name}: {t} does not exist"
        for t, fn in re.findall(r"(tests/[a-z_]+\.py)::([a-z_0-9]+)", why):
            with open(os.path.join(ROOT, t)) as f:
                assert f"def {fn}(" in f.read(), f"{name}: {t} has no {fn}"
    assert sorted(I.UNTESTED) == ["copy_kernel<0>", "copy_kernel<1>"], "a kernel no test runs needs a test, not this list"
    assert set(I.INCIDENTAL) <= set(I.ELSEWHERE)


def test_the_model_places_every_case_at_other_cu_counts():
    # the ladders do not depend on the device; the shapes that do (small_launch_shape) must still resolve
    for cus in (64, 104, 228, 256, 304):
        for c in I.CASES:
            for k in I.expected_kernels(c, cus):
                assert re.fullmatch(r"[a-z_]+<[-0-9a-z, ]+>", k), k
    # the cases whose point is the shape keep it on every device
    for cus in (64, 104, 228, 256, 304):
        for c in I.CASES:
            if c.n == "seam_u2":
                assert I.expected_kernel(c, cus).endswith("true, 2>"), (cus, c.name())
                smaller = I.Case(**{**c.__dict__, "n": c.elements(cus) - 4 * I.K_TAIL_QUANTUM4})
                assert I.expected_kernel(smaller, cus).endswith("true, 1>"), "seam_u2 is the smallest such n"
            if c.n == "ragged" and c.cfg is None:
                n4 = I.bulk_float4s(c, cus)
                assert 8 * cus * 64 < n4 < 16 * cus * 64, (cus, n4)


def test_trace_record_agrees_with_the_model():
    if not os.path.exists(RECORD):
        # the record is committed beside this test: its absence is a failure, not a skip
        pytest.fail("profiles/instantiations/launched.json is missing: record a profiler run of "
                    "tests/test_gpu_instantiations.py again (scripts/instantiations_from_trace.py)")
    with open(RECORD) as f:
        rec = json.load(f)
    cus = int(rec["num_cus"])
    launched = {normalise(k) for k in rec["kernels"]}
    # the record lists this library's kernels only (scripts/instantiations_from_trace.py)
    want = set(I.case_names(cus))
    # beside the cases' own kernels only the norm pass in front of a clipped step may run: a G > 1
    # form, an UNREACHABLE or an UNTESTED kernel in a one-rank run is reported
    got = launched - set(I.INCIDENTAL)
    assert got == want, (f"launched but not expected: {sorted(got - want)[:20]}\n"
                         f"expected but not launched: {sorted(want - got)[:20]}")
