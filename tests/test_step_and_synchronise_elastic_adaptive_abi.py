"""``cbx_step_and_synchronise_elastic_adaptive`` and ``cbx_ea_plan_step_and_optimise_adaptive`` without a GPU: a
NULL context or plan is an error, and their kernel is a shared object of its own that the library finds."""
import ctypes
import glob
import os


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    tasks = (ctypes.c_int * 1)(0)
    assert lib.cbx_step_and_synchronise_elastic_adaptive(None, 0, 1, 0, tasks, None, 0) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
    rc = lib.cbx_ea_plan_step_and_optimise_adaptive(None, None, None, 0, None, None, None, None, None, None, None,
                                                    None, None, 0.05, 1e-9, 0, 0.1, 0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_the_kernel_is_a_shared_object_of_its_own():
    from crossbow_amd import build
    assert os.path.basename(build.ELASTIC_ADAPTIVE_LIB) == "libcrossbow_sma_elastic_adaptive.so"
    assert os.path.exists(build.ELASTIC_ADAPTIVE_LIB), "python __graft_entry__.py builds it"
    with open(build.LIB, "rb") as f:
        blob = f.read()
    assert b"libcrossbow_sma_elastic_adaptive.so" in blob and b"$ORIGIN" in blob
    others = [p for p in glob.glob(os.path.join(build.PKG, "libcrossbow_sma*.so")) if p != build.ELASTIC_ADAPTIVE_LIB]
    assert build.code_object_digest(build.ELASTIC_ADAPTIVE_LIB) not in [build.code_object_digest(p) for p in others]
