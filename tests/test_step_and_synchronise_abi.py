"""``cbx_step_and_synchronise`` without a GPU: the call and its kernel-config
setter are declared in the header, bound in ``crossbow_amd._abi`` and exported
by the built library, argument for argument; the discard flag is ``1u``;
``thegpu.py`` exposes both; a NULL context is an error, not a crash."""
from __future__ import annotations

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cbx_step_and_synchronise", "cbx_set_task_barrier_kernel_config")


def _header():
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        return f.read()


def test_new_symbols_are_declared_bound_and_exported():
    from crossbow_amd import _abi, _lib
    header = _header()
    lib = _lib.load()
    for name in NEW:
        assert f"int {name} (" in header, name
        assert name in _abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1], name
    assert "#define CBX_ABI_VERSION 1" in header
    assert lib.cbx_abi_version() == 1


def test_signatures_match_the_header_argument_for_argument():
    from crossbow_amd import _abi
    header = _header()
    for name, nargs in zip(NEW, (7, 4)):
        m = re.search(r"int %s \(([^;]*)\);" % name, header)
        assert m, name
        declared = [a for a in m.group(1).split(",") if a.strip()]
        assert len(declared) == nargs == len(_abi.SIGNATURES[name][1]), (name, m.group(1))
    # const int *tasks, void *const *streams, unsigned flags
    import ctypes
    args = _abi.SIGNATURES["cbx_step_and_synchronise"][1]
    assert args[4] == ctypes.POINTER(ctypes.c_int) and args[5] == ctypes.POINTER(ctypes.c_void_p)
    assert args[6] == ctypes.c_uint


def test_the_discard_flag_is_1u():
    from crossbow_amd import _abi, _lib
    assert "#define CBX_STEP_DISCARD_TASK_OUTPUTS 1u" in _header()
    assert _abi.STEP_DISCARD_TASK_OUTPUTS == 1 and _lib.STEP_DISCARD_TASK_OUTPUTS == 1


def test_python_wrappers_expose_the_calls():
    import inspect

    from crossbow_amd.thegpu import TheGPU
    assert callable(TheGPU.step_and_synchronise) and callable(TheGPU.set_task_barrier_kernel_config)
    assert list(inspect.signature(TheGPU.step_and_synchronise).parameters) == [
        "self", "first", "clock", "autotune", "tasks", "streams", "flags"]
    assert list(inspect.signature(TheGPU.set_task_barrier_kernel_config).parameters) == [
        "self", "block", "unroll", "waves_per_cu"]


def test_null_context_is_an_error_not_a_crash():
    import ctypes

    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    assert lib.cbx_set_task_barrier_kernel_config(None, 64, 2, -1) == _lib.CBX_ERR_INVALID


def test_the_kernel_file_is_part_of_every_build_of_the_library():
    from crossbow_amd import build
    assert "task_barrier_kernels.hip" in build.SOURCES
    # the text it shares with the per-variable and the clipped kernel makes the library stale too
    for shared in ("task_barrier_step.h", "task_barrier_body.inc", "task_barrier_launch.h"):
        assert os.path.join(build.CSRC, shared) in build._deps(), shared
    for script in ("build_sanitized.sh", "build_fake_rccl.sh"):
        with open(os.path.join(ROOT, "scripts", script)) as f:
            assert "crossbow_amd/csrc/task_barrier_kernels.hip" in f.read(), script
