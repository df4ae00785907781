"""``cbx_step_and_synchronise_clipped_variables`` and
``cbx_sma_plan_step_and_optimise_clipped_variables`` without a GPU: both are
declared in the header, bound in ``crossbow_amd._abi`` and exported by the
built library; each has the parameter list of the call it extends
(``cbx_step_and_synchronise``, ``cbx_sma_plan_step_and_optimise_clipped``);
``thegpu.py`` and ``seam.py`` expose them; a NULL context or plan is an error,
not a crash; and their kernels live in a shared object of their own that every
build takes and that no other object defines."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT, SEAM = "cbx_step_and_synchronise_clipped_variables", "cbx_sma_plan_step_and_optimise_clipped_variables"
EXTENDS = {CONTEXT: "cbx_step_and_synchronise", SEAM: "cbx_sma_plan_step_and_optimise_clipped"}
SOURCE = "crossbow_amd/csrc/task_barrier_clipped_variables_kernels.hip"
KERNEL = "task_barrier_clipped_variables_kernel"


def _header():
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        return f.read()


def _declared(name):
    m = re.search(r"int %s \(([^;]*)\);" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def test_the_symbols_are_declared_bound_and_exported():
    from crossbow_amd import _abi, _lib
    lib = _lib.load()
    header = _header()
    for name in (CONTEXT, SEAM):
        assert f"int {name} (" in header, name
        assert name in _abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1], name
        assert getattr(lib, name).restype == ctypes.c_int
    assert "#define CBX_ABI_VERSION 1" in header


def test_each_call_has_the_parameters_of_the_call_it_extends():
    from crossbow_amd import _abi
    for name, base in EXTENDS.items():
        assert _declared(name) == _declared(base), name
        assert _abi.SIGNATURES[name] == _abi.SIGNATURES[base], name
    # and the context call those of the other two fused calls as well
    assert _declared(CONTEXT) == _declared("cbx_step_and_synchronise_clipped") == \
        _declared("cbx_step_and_synchronise_variables")


def test_the_python_wrappers_expose_the_calls():
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.thegpu import TheGPU
    assert list(inspect.signature(TheGPU.step_and_synchronise_clipped_variables).parameters) == \
        list(inspect.signature(TheGPU.step_and_synchronise).parameters)
    assert list(inspect.signature(SmaPlan.step_and_optimise_clipped_variables).parameters) == \
        list(inspect.signature(SmaPlan.step_and_optimise_clipped).parameters)


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_clipped_variables(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = lib.cbx_sma_plan_step_and_optimise_clipped_variables(None, None, None, None, 0, None, None, None, None, None,
                                                              None, None, None, None, None, 1.0, 0, 0.1, 0.9, 0.9,
                                                              0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own_in_every_build():
    from crossbow_amd import build
    assert build.CLIPPED_VARIABLES_SOURCES == ("task_barrier_clipped_variables_kernels.hip",)
    assert "task_barrier_clipped_variables_kernels.hip" not in \
        build.SOURCES + build.VARIABLES_SOURCES + build.CLIPPED_SOURCES
    assert os.path.basename(build.CLIPPED_VARIABLES_LIB) == "libcrossbow_sma_clipped_variables.so"
    assert os.path.exists(build.CLIPPED_VARIABLES_LIB), "python __graft_entry__.py builds it"
    # the library names it as a dependency found beside itself
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_clipped_variables.so" in blob and b"$ORIGIN" in blob
    # the one staleness check covers it
    assert os.path.join(build.CSRC, "task_barrier_clipped_variables_kernels.hip") in build._deps()
    # and the text the four barrier kernels share
    for shared in ("task_barrier_step.h", "task_barrier_body.inc", "task_barrier_launch.h", "clip_internal.h",
                   "optimise_plan.h"):
        assert os.path.join(build.CSRC, shared) in build._deps(), shared
    for script in ("scripts/build_sanitized.sh", "scripts/build_fake_rccl.sh", "__graft_entry__.py"):
        with open(os.path.join(ROOT, script)) as f:
            assert SOURCE in f.read(), script


def test_none_of_the_other_three_objects_defines_the_new_kernel():
    from crossbow_amd import build
    tool = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    own, main, variables, clipped = (subprocess.run([tool, "-C", "--defined-only", lib], check=True,
                                                    capture_output=True, text=True).stdout
                                     for lib in (build.CLIPPED_VARIABLES_LIB, build.LIB, build.VARIABLES_LIB,
                                                 build.CLIPPED_LIB))
    for other in (main, variables, clipped):
        assert KERNEL not in other and "launch_task_barrier_clipped_variables" not in other
    assert KERNEL in own and "launch_task_barrier_clipped_variables" in own
    # and it holds neither of the kernels the other side objects hold
    assert "task_barrier_clipped_kernel" not in own and "task_barrier_variables_kernel" not in own
    assert len(build.code_object_digest(build.CLIPPED_VARIABLES_LIB)) == 64
