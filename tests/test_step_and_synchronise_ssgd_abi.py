"""``cbx_step_and_synchronise_ssgd`` and ``cbx_ssgd_plan_step_and_optimise``
without a GPU: both are declared in the header, bound in ``crossbow_amd._abi``
with matching argument lists and exported by the built library; ``thegpu.py``
and ``seam.py`` expose them; a NULL context or plan is an error, not a crash;
and their kernels live in a shared object of their own that every build takes
and that no other object defines."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT, SEAM = "cbx_step_and_synchronise_ssgd", "cbx_ssgd_plan_step_and_optimise"
SOURCE = "crossbow_amd/csrc/task_ssgd_kernels.hip"
KERNEL = "task_ssgd_kernel"


def _header():
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        return f.read()


def _declared(name):
    m = re.search(r"int %s \(([^;]*)\);" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def _names(name):
    return [a.rsplit(" ", 1)[1].lstrip("*") for a in _declared(name)]


def _ctype_of(arg: str):
    """The ctypes type _abi binds for one declared C parameter."""
    from crossbow_amd import _abi
    kind = arg.rsplit(" ", 1)[0].replace(" ", "") + "*" * arg.rsplit(" ", 1)[1].count("*")
    return {"int": _abi._I, "float": _abi._F, "unsigned": ctypes.c_uint, "constint*": _abi._IP,
            "constfloat*": _abi._FP, "cbx_context*": _abi._P, "cbx_sma_plan*": _abi._P, "void*const*": _abi._PP,
            "float*const*": _abi._PP}[kind]


def _others():
    from crossbow_amd import build
    return (build.LIB, build.VARIABLES_LIB, build.CLIPPED_LIB, build.CLIPPED_VARIABLES_LIB, build.ELASTIC_STEPS_LIB)


def test_the_symbols_are_declared_bound_and_exported():
    from crossbow_amd import _abi, _lib
    lib = _lib.load()
    header = _header()
    for name in (CONTEXT, SEAM):
        assert f"int {name} (" in header, name
        assert name in _abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1], name
        assert getattr(lib, name).restype == ctypes.c_int
        # the bound argument list is the declared one, parameter by parameter
        assert [_ctype_of(a) for a in _declared(name)] == _abi.SIGNATURES[name][1], name
    assert "#define CBX_ABI_VERSION 1" in header


def test_the_context_call_has_the_parameters_of_the_call_it_stands_beside():
    from crossbow_amd import _abi
    assert _declared(CONTEXT) == _declared("cbx_step_and_synchronise")
    assert _abi.SIGNATURES[CONTEXT] == _abi.SIGNATURES["cbx_step_and_synchronise"]


def test_the_seam_call_is_the_plain_ssgd_step_plus_the_task_steps_arguments():
    names, base = _names(SEAM), _names("cbx_ssgd_plan_step")
    assert [n for n in names if n not in ("g", "step", "learning_rate", "weight_decay", "flags")] == base
    assert names == ["plan", "streams", "z", "last", "acc", "nreplicas", "replica_device", "w", "g", "locked", "step",
                     "learning_rate", "momentum", "weight_decay", "wpc", "first", "flags"]


def test_the_header_states_the_order_of_the_accumulator():
    doc = _header().split("int %s (" % CONTEXT)[0].rsplit("/*", 1)[1]
    assert "ascending id order" in doc.lower() and "not assumed zero" in doc


def test_the_python_wrappers_expose_the_calls():
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.thegpu import TheGPU
    assert list(inspect.signature(TheGPU.step_and_synchronise_ssgd).parameters) == \
        list(inspect.signature(TheGPU.step_and_synchronise).parameters)
    assert list(inspect.signature(SmaPlan.ssgd_step_and_optimise).parameters) == \
        ["self", "streams", "z", "last", "acc", "replicas", "momentum", "weight_decay", "wpc", "first", "flags"]


def test_there_is_no_jni_native_for_it():
    with open(os.path.join(ROOT, "crossbow_amd", "csrc", "jni", "TheGPU_jni.c")) as f:
        assert CONTEXT not in f.read()


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_ssgd(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = lib.cbx_ssgd_plan_step_and_optimise(None, None, None, None, None, 0, None, None, None, None, None, None, 0.9,
                                             0.0, 1, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own_in_every_build():
    from crossbow_amd import build
    assert build.SSGD_STEPS_SOURCES == ("task_ssgd_kernels.hip",)
    assert "task_ssgd_kernels.hip" not in (build.SOURCES + build.VARIABLES_SOURCES + build.CLIPPED_SOURCES +
                                           build.CLIPPED_VARIABLES_SOURCES + build.ELASTIC_STEPS_SOURCES)
    assert os.path.basename(build.SSGD_STEPS_LIB) == "libcrossbow_sma_ssgd_steps.so"
    assert os.path.exists(build.SSGD_STEPS_LIB), "python __graft_entry__.py builds it"
    # the library names it as a dependency found beside itself
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_ssgd_steps.so" in blob and b"$ORIGIN" in blob
    # the one staleness check covers it, and the header that only it and the two doors read
    assert os.path.join(build.CSRC, "task_ssgd_kernels.hip") in build._deps()
    assert os.path.join(build.CSRC, "task_ssgd_internal.h") in build._deps()
    for script in ("scripts/build_sanitized.sh", "scripts/build_fake_rccl.sh", "__graft_entry__.py"):
        with open(os.path.join(ROOT, script)) as f:
            assert SOURCE in f.read(), script


def test_none_of_the_other_five_objects_defines_the_new_kernel():
    from crossbow_amd import build
    tool = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    own, *others = (subprocess.run([tool, "-C", "--defined-only", lib], check=True, capture_output=True,
                                   text=True).stdout for lib in (build.SSGD_STEPS_LIB,) + _others())
    for other in others:
        assert KERNEL not in other and "launch_task_ssgd" not in other
    assert KERNEL in own and "launch_task_ssgd" in own
    # and it holds none of the kernels the other objects hold
    for theirs in ("task_barrier", "task_elastic", "averaging_kernel", "ssgd_apply_kernel", "ssgd_accumulate_kernel"):
        assert theirs not in own, theirs


def test_the_new_object_has_a_code_object_digest_of_its_own():
    from crossbow_amd import build
    digest = build.code_object_digest(build.SSGD_STEPS_LIB)
    assert re.fullmatch(r"[0-9a-f]{64}", digest), digest
    assert digest not in {build.code_object_digest(lib) for lib in _others()}


def test_the_kernel_arguments_stay_under_the_limit():
    # TaskSsgdArgs: three pointer lists and one of floats at kMaxReplicas = 64, three base pointers and the scalars
    with open(os.path.join(ROOT, "crossbow_amd", "csrc", "task_ssgd_internal.h")) as f:
        text = f.read()
    assert "static_assert(sizeof(TaskSsgdArgs) < 4096" in text
    assert 64 * (3 * 8 + 4) + 3 * 8 + 8 + 6 * 4 + 2 * 8 + 8 < 4096
