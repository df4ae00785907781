"""``cbx_step_and_synchronise_ssgd_adaptive``, ``cbx_base_adaptive_stats`` and
``cbx_ssgd_plan_step_and_optimise_adaptive`` without a GPU: a NULL context or plan is an error, and their kernels are
a shared object of its own that the library finds."""
import ctypes
import os


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_ssgd_adaptive(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    out = (_lib.AdaptiveStats * 1)()
    assert lib.cbx_base_adaptive_stats(None, 0, out, 1) == _lib.CBX_ERR_INVALID
    rc = lib.cbx_ssgd_plan_step_and_optimise_adaptive(None, None, None, None, None, 0, None, None, None, None, None,
                                                      None, 0, 0.05, 1e-9, 0, 0.9, 0.0, 1, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernels_are_a_shared_object_of_their_own():
    from crossbow_amd import build
    assert os.path.basename(build.SSGD_ADAPTIVE_LIB) == "libcrossbow_sma_ssgd_adaptive.so"
    assert os.path.exists(build.SSGD_ADAPTIVE_LIB), "python __graft_entry__.py builds it"
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_ssgd_adaptive.so" in blob and b"$ORIGIN" in blob
