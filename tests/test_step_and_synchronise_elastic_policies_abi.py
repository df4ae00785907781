"""``cbx_step_and_synchronise_elastic_clipped_variables`` and
``cbx_ea_plan_step_and_optimise_clipped_variables`` without a GPU: both are
declared in the header, bound in ``crossbow_amd._abi`` with matching argument
lists and exported by the built library; ``thegpu.py`` and ``seam.py`` expose
them; a NULL context or plan is an error, not a crash; and their kernels live in
a shared object of their own that every build takes and that no other object
defines."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT = "cbx_step_and_synchronise_elastic_clipped_variables"
SEAM = "cbx_ea_plan_step_and_optimise_clipped_variables"
SOURCES = ("task_elastic_clipped_variables_kernels.hip", "task_elastic_clipped_kernels.hip",
           "task_elastic_variables_kernels.hip")
KERNELS = ("task_elastic_variables_kernel", "task_elastic_clipped_kernel", "task_elastic_clipped_variables_kernel")
LAUNCHERS = ("launch_task_elastic_variables", "launch_task_elastic_clipped", "launch_task_elastic_clipped_variables")


def _header():
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        return f.read()


def _declared(name):
    m = re.search(r"int %s \(([^;]*)\);" % name, _header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def _ctype_of(arg: str):
    """The ctypes type _abi binds for one declared C parameter."""
    from crossbow_amd import _abi
    kind = arg.rsplit(" ", 1)[0].replace(" ", "") + "*" * arg.rsplit(" ", 1)[1].count("*")
    return {"int": _abi._I, "float": _abi._F, "unsigned": ctypes.c_uint, "constint*": _abi._IP,
            "constfloat*": _abi._FP, "cbx_context*": _abi._P, "cbx_sma_plan*": _abi._P, "void*const*": _abi._PP,
            "float*const*": _abi._PP}[kind]


def _other_libs(build):
    return (build.LIB, build.VARIABLES_LIB, build.CLIPPED_LIB, build.CLIPPED_VARIABLES_LIB, build.ELASTIC_STEPS_LIB,
            build.SSGD_STEPS_LIB)


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
    assert _declared(CONTEXT) == _declared("cbx_step_and_synchronise_elastic")
    assert _abi.SIGNATURES[CONTEXT] == _abi.SIGNATURES["cbx_step_and_synchronise"]


def test_the_seam_call_is_the_elastic_one_with_the_clip_and_the_switch():
    names = [a.rsplit(" ", 1)[1].lstrip("*") for a in _declared(SEAM)]
    base = [a.rsplit(" ", 1)[1].lstrip("*") for a in _declared("cbx_ea_plan_step_and_optimise")]
    added = ["slot", "max_norm", "skip_nonfinite", "use_variables"]
    assert [n for n in names if n not in added] == base
    at = names.index("learning_rate") + 1
    assert names[at:at + 4] == added and names[at + 4] == "alpha"
    # the clip's three are where cbx_sma_plan_step_and_optimise_clipped has them: behind the rates
    sma = [a.rsplit(" ", 1)[1].lstrip("*") for a in _declared("cbx_sma_plan_step_and_optimise_clipped")]
    at = sma.index("learning_rate") + 1
    assert sma[at:at + 3] == added[:3]


def test_the_python_wrappers_expose_the_calls():
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.thegpu import TheGPU
    assert list(inspect.signature(TheGPU.step_and_synchronise_elastic_clipped_variables).parameters) == \
        list(inspect.signature(TheGPU.step_and_synchronise_elastic).parameters)
    assert list(inspect.signature(SmaPlan.elastic_step_and_optimise_clipped_variables).parameters) == \
        list(inspect.signature(SmaPlan.elastic_step_and_optimise).parameters) + \
        ["slots", "max_norm", "skip_nonfinite", "use_variables"]


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert getattr(lib, CONTEXT)(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = getattr(lib, SEAM)(None, None, None, 0, None, None, None, None, None, None, None, None, None, 1.0, 0, 0, 0.1,
                            0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own_in_every_build():
    from crossbow_amd import build
    # one compilation unit per policy, none of them in another object's list
    assert sorted(build.ELASTIC_POLICIES_SOURCES) == sorted(SOURCES)
    every_other = (build.SOURCES + build.VARIABLES_SOURCES + build.CLIPPED_SOURCES + build.CLIPPED_VARIABLES_SOURCES +
                   build.ELASTIC_STEPS_SOURCES + build.SSGD_STEPS_SOURCES)
    assert not set(SOURCES) & set(every_other)
    assert os.path.basename(build.ELASTIC_POLICIES_LIB) == "libcrossbow_sma_elastic_policies.so"
    assert os.path.exists(build.ELASTIC_POLICIES_LIB), "python __graft_entry__.py builds it"
    # the library names it as a dependency found beside itself
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_elastic_policies.so" in blob and b"$ORIGIN" in blob
    # the one staleness check covers the sources and the shared text
    deps = build._deps()
    for name in SOURCES + ("task_elastic_policy.h", "task_elastic_policy_body.inc"):
        assert os.path.join(build.CSRC, name) in deps, name
    for script in ("scripts/build_sanitized.sh", "scripts/build_fake_rccl.sh", "__graft_entry__.py"):
        with open(os.path.join(ROOT, script)) as f:
            text = f.read()
        for name in SOURCES:
            assert "crossbow_amd/csrc/" + name in text, (script, name)


def test_none_of_the_six_other_objects_defines_the_new_kernels():
    from crossbow_amd import build
    tool = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    own, *others = (subprocess.run([tool, "-C", "--defined-only", lib], check=True, capture_output=True,
                                   text=True).stdout for lib in (build.ELASTIC_POLICIES_LIB,) + _other_libs(build))
    assert len(others) == 6
    for other in others:
        for name in KERNELS + LAUNCHERS:
            assert name not in other, name
    for name in KERNELS + LAUNCHERS:
        assert name in own, name
    # and it holds none of the kernels or launchers the other objects hold
    assert "task_barrier" not in own and "averaging_kernel" not in own and "task_ssgd" not in own
    assert "task_elastic_kernel" not in own and "launch_task_elastic(" not in own


def test_the_new_object_has_a_code_object_digest_of_its_own():
    from crossbow_amd import build
    digest = build.code_object_digest(build.ELASTIC_POLICIES_LIB)
    assert re.fullmatch(r"[0-9a-f]{64}", digest), digest
    assert digest not in {build.code_object_digest(lib) for lib in _other_libs(build)}
