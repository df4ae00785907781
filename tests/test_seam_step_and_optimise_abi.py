"""``cbx_sma_plan_step_and_optimise`` without a GPU: the call is declared in the
header, bound in ``crossbow_amd._abi`` and exported by the built library,
argument for argument; ``seam.py`` exposes it; a NULL plan is an error, not a
crash."""
from __future__ import annotations

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cbx_sma_plan_step_and_optimise"


def _header():
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        return f.read()


def test_the_symbol_is_declared_bound_and_exported():
    from crossbow_amd import _abi, _lib
    lib = _lib.load()
    assert f"int {NAME} (" in _header()
    assert NAME in _abi.SIGNATURES
    assert getattr(lib, NAME).argtypes == _abi.SIGNATURES[NAME][1]
    assert getattr(lib, NAME).restype == ctypes.c_int


def test_the_signature_matches_the_header_argument_for_argument():
    from crossbow_amd import _abi
    m = re.search(r"int %s \(([^;]*)\);" % NAME, _header())
    assert m
    declared = [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]
    args = _abi.SIGNATURES[NAME][1]
    assert len(declared) == 20 == len(args), declared
    PP, IP, FP = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    kinds = {"cbx_sma_plan *": ctypes.c_void_p, "void *const *": PP, "float *const *": PP, "const int *": IP,
             "const float *": FP, "int ": ctypes.c_int, "float ": ctypes.c_float, "unsigned ": ctypes.c_uint}
    for text, bound in zip(declared, args):
        kind = next(k for k in kinds if text.startswith(k))
        assert kinds[kind] == bound, (text, bound)
    names = [re.split(r"[ *]", a)[-1] for a in declared]
    assert names == ["plan", "streams", "z", "last", "nreplicas", "replica_device", "w", "s", "g", "rlast", "locked",
                     "copy", "step", "learning_rate", "alpha", "momentum", "replica_momentum", "weight_decay", "first",
                     "flags"]


def test_the_python_wrapper_exposes_the_call():
    import inspect

    from crossbow_amd.seam import SmaPlan
    assert callable(SmaPlan.step_and_optimise)
    assert list(inspect.signature(SmaPlan.step_and_optimise).parameters) == [
        "self", "streams", "z", "last", "replicas", "alpha", "momentum", "replica_momentum", "weight_decay", "first",
        "flags"]


def test_a_null_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    rc = lib.cbx_sma_plan_step_and_optimise(None, None, None, None, 0, None, None, None, None, None, None, None, None,
                                            None, 0.1, 0.9, 0.9, 0.0, 0, 0)
    assert rc == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()
