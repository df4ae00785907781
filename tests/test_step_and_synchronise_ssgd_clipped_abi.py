"""The four entry points of synchronous SGD with gradient clipping without a GPU: declared, bound and
exported alike; kernels in a shared object of their own; a NULL context or plan is an error."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cbx_replica_accumulate_clipped", "cbx_step_and_synchronise_ssgd_clipped",
         "cbx_ssgd_plan_accumulate_clipped", "cbx_ssgd_plan_step_and_optimise_clipped")
OWN = ("task_ssgd_clipped_kernel", "ssgd_accumulate_clipped_kernel", "launch_task_ssgd_clipped",
       "launch_ssgd_accumulate_clipped")


def _declared(name):
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        m = re.search(r"int %s \(([^;]*)\);" % name, f.read())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def _ctype_of(arg: str):
    """The ctypes type _abi binds for one declared C parameter; `w` is a device buffer, an address like g and acc."""
    from crossbow_amd import _abi
    kind = arg.rsplit(" ", 1)[0].replace(" ", "") + "*" * arg.rsplit(" ", 1)[1].count("*")
    return {"int": _abi._I, "float": _abi._F, "unsigned": ctypes.c_uint, "constint*": _abi._IP,
            "constfloat*": _abi._P if arg.endswith("*w") else _abi._FP, "cbx_context*": _abi._P,
            "cbx_sma_plan*": _abi._P, "void*const*": _abi._PP, "float*const*": _abi._PP, "void*": _abi._P,
            "float*": _abi._P}[kind]


@pytest.mark.parametrize("name", CALLS)
def test_declared_bound_and_exported(name):
    from crossbow_amd import _abi, _lib
    fn = getattr(_lib.load(), name)
    assert fn.argtypes == _abi.SIGNATURES[name][1] and fn.restype == ctypes.c_int
    assert [_ctype_of(a) for a in _declared(name)] == _abi.SIGNATURES[name][1]


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    for rc in (lib.cbx_replica_accumulate_clipped(None, 0, 0, None),
               lib.cbx_step_and_synchronise_ssgd_clipped(None, 0, 1, 0, (ctypes.c_int * 1)(0), None, 0),
               lib.cbx_ssgd_plan_accumulate_clipped(None, 0, 0, None, None, None, None, 0.1, 0.0, 1.0, 1),
               lib.cbx_ssgd_plan_step_and_optimise_clipped(None, None, None, None, None, 0, None, None, None, None,
                                                           None, None, None, 1.0, 1, 0.9, 0.0, 1, 0, 0)):
        assert rc == _lib.CBX_ERR_INVALID and b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own():
    from crossbow_amd import build
    assert build.SSGD_CLIPPED_SOURCES == ("task_ssgd_clipped_kernels.hip",)
    with open(build.LIB, "rb") as f:
        assert os.path.basename(build.SSGD_CLIPPED_LIB).encode() == b"libcrossbow_sma_ssgd_clipped.so" in f.read()
    assert os.path.join(build.CSRC, "task_ssgd_clipped_internal.h") in build._deps()
    for script in ("scripts/build_sanitized.sh", "scripts/build_fake_rccl.sh", "__graft_entry__.py"):
        with open(os.path.join(ROOT, script)) as f:
            assert "crossbow_amd/csrc/task_ssgd_clipped_kernels.hip" in f.read(), script
    others = (build.LIB, build.VARIABLES_LIB, build.CLIPPED_LIB, build.CLIPPED_VARIABLES_LIB, build.ELASTIC_STEPS_LIB,
              build.SSGD_STEPS_LIB, build.ELASTIC_POLICIES_LIB)
    tool = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    own, *theirs = (subprocess.run([tool, "-C", "--defined-only", lib], check=True, capture_output=True,
                                   text=True).stdout for lib in (build.SSGD_CLIPPED_LIB,) + others)
    for name in OWN:
        assert name in own and not any(name in other for other in theirs), name
    assert "task_ssgd_kernel" not in own and "ssgd_accumulate_kernel" not in own  # nor the others' kernels in it
    assert build.code_object_digest(build.SSGD_CLIPPED_LIB) not in {build.code_object_digest(lib) for lib in others}
