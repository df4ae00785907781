"""``cbx_step_and_synchronise_adaptive`` and ``cbx_sma_plan_step_and_optimise_adaptive`` without a GPU: a NULL
context or plan is an error, not a crash, and their kernels live in a shared object of their own that the
library finds beside itself."""
from __future__ import annotations

import ctypes
import glob
import os


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_adaptive(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = lib.cbx_sma_plan_step_and_optimise_adaptive(None, None, None, None, 0, None, None, None, None, None, None,
                                                     None, None, None, None, 0.05, 1e-9, 0, 0.1, 0.9, 0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own():
    from crossbow_amd import build
    assert os.path.basename(build.ADAPTIVE_STEPS_LIB) == "libcrossbow_sma_adaptive_steps.so"
    assert os.path.exists(build.ADAPTIVE_STEPS_LIB), "python __graft_entry__.py builds it"
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_adaptive_steps.so" in blob and b"$ORIGIN" in blob
    others = [p for p in glob.glob(os.path.join(build.PKG, "libcrossbow_sma*.so")) if p != build.ADAPTIVE_STEPS_LIB]
    assert build.code_object_digest(build.ADAPTIVE_STEPS_LIB) not in [build.code_object_digest(p) for p in others]
