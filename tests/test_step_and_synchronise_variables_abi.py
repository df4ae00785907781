"""``cbx_step_and_synchronise_variables`` and
``cbx_sma_plan_step_and_optimise_variables`` without a GPU: both are declared
in the header, bound in ``crossbow_amd._abi`` and exported by the built library
with the signatures of the calls they extend; ``thegpu.py`` and ``seam.py``
expose them; a NULL context or plan, or a machine without a device, is an
error, not a crash; their kernels live in a shared object of their own that
every build takes; and the padded chunk table (build_padded_optimise_plan,
optimise_plan.h) is checked by a stand-alone program under ASan + UBSan."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"cbx_step_and_synchronise_variables": "cbx_step_and_synchronise",
         "cbx_sma_plan_step_and_optimise_variables": "cbx_sma_plan_step_and_optimise"}


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
    for name, plain in PAIRS.items():
        assert f"int {name} (" in header, name
        assert name in _abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1], name
        assert getattr(lib, name).restype == ctypes.c_int
        # the parameters are those of the call it extends, in the header and in the binding
        assert _declared(name) == _declared(plain), name
        assert _abi.SIGNATURES[name] == _abi.SIGNATURES[plain], name
    assert "#define CBX_ABI_VERSION 1" in header


def test_the_python_wrappers_expose_the_calls():
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.thegpu import TheGPU
    assert list(inspect.signature(TheGPU.step_and_synchronise_variables).parameters) == \
        list(inspect.signature(TheGPU.step_and_synchronise).parameters)
    assert list(inspect.signature(SmaPlan.step_and_optimise_variables).parameters) == \
        list(inspect.signature(SmaPlan.step_and_optimise).parameters)


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_variables(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = lib.cbx_sma_plan_step_and_optimise_variables(None, None, None, None, 0, None, None, None, None, None, None,
                                                      None, None, None, 0.1, 0.9, 0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_without_a_device_both_fail_loudly():
    # Where no device is visible neither handle can be made, and the calls on what is left
    # raise; where one is visible the same objects, freed again, raise all the same.
    import pytest

    from crossbow_amd import CbxError, TheGPU
    from crossbow_amd.seam import SmaPlan
    g = TheGPU()
    try:
        g.init([0])
    except CbxError:
        pass
    g.free()
    with pytest.raises(CbxError):
        g.step_and_synchronise_variables(0, 1, 0, [], None, 0)
    try:
        plan = SmaPlan([0], 1027)
    except CbxError:
        return
    plan.free()
    with pytest.raises(CbxError):
        plan.step_and_optimise_variables([None], [None], None, [], 0.1, 0.0, 0.0, 0.0)


def test_the_kernels_are_a_shared_object_of_their_own_in_every_build():
    from crossbow_amd import build
    assert build.VARIABLES_SOURCES == ("task_barrier_variables_kernels.hip",)
    assert "task_barrier_variables_kernels.hip" not in build.SOURCES
    assert os.path.basename(build.VARIABLES_LIB) == "libcrossbow_sma_variables.so"
    assert os.path.exists(build.VARIABLES_LIB), "python __graft_entry__.py builds it"
    # the library names it as a dependency found beside itself
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_variables.so" in blob and b"$ORIGIN" in blob
    # the staleness check covers both libraries
    deps = build._deps()
    assert os.path.join(build.CSRC, "task_barrier_variables_kernels.hip") in deps
    # and the text the three barrier kernels share
    for shared in ("task_barrier_step.h", "task_barrier_body.inc", "task_barrier_launch.h", "optimise_plan.h"):
        assert os.path.join(build.CSRC, shared) in deps, shared
    for script in ("build_sanitized.sh", "build_fake_rccl.sh"):
        with open(os.path.join(ROOT, "scripts", script)) as f:
            assert "crossbow_amd/csrc/task_barrier_variables_kernels.hip" in f.read(), script
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "crossbow_amd/csrc/task_barrier_variables_kernels.hip" in f.read()


def test_the_device_code_of_the_main_library_holds_no_new_kernel():
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    from crossbow_amd import build
    import shutil
    tool = shutil.which("nm") or nm
    main = subprocess.run([tool, "-C", "--defined-only", build.LIB], check=True, capture_output=True, text=True).stdout
    own = subprocess.run([tool, "-C", "--defined-only", build.VARIABLES_LIB], check=True, capture_output=True,
                         text=True).stdout
    assert "task_barrier_variables_kernel" not in main
    assert "task_barrier_variables_kernel" in own and "launch_task_barrier_variables" in own
    assert len(build.code_object_digest(build.LIB)) == 64 and len(build.code_object_digest(build.VARIABLES_LIB)) == 64


def test_padded_chunk_table_under_asan_and_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "padded_optimise_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "crossbow_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "padded_optimise_plan_test.cpp")],
                       check=True, capture_output=True, timeout=240)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.startswith("ok "), p.stdout
