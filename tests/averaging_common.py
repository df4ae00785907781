"""The CPU restatement of the elastic-averaging and Polyak-Ruppert barriers
(tests/native/averaging_ref.c) for the tests: a ctypes front end over
``oracle.SmaState``, whose inputs come from ``oracle.make_state``
(BASELINE.md 2.3).  Test infrastructure only.

tests/test_averaging_ref.py pins the restatement (an OpenBLAS replay of the
reference's call sequence, the semantics, the summation order) before the GPU
tests compare the library with it.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "libaveraging_ref.so")

_lib = None


def build() -> str:
    subprocess.run(["bash", os.path.join(ROOT, "scripts", "build_averaging_ref.sh")], check=True,
                   stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        fp = ctypes.POINTER(ctypes.c_float)
        fpp = ctypes.POINTER(fp)
        ip = ctypes.POINTER(ctypes.c_int)
        L.cbr_elastic_average.restype = None
        L.cbr_elastic_average.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, fpp, fpp, fpp,
                                          ip, ctypes.c_int, fp]
        L.cbr_polyak_ruppert.restype = ctypes.c_int
        L.cbr_polyak_ruppert.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_int,
                                         fpp, fpp, fpp, ip, ip, ctypes.c_int, fp]
        _lib = L
    return _lib


def _ip(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def elastic_average(st: O.SmaState) -> None:
    """One elastic-averaging step on z and w, in place.  With G = 1 the
    difference is taken from w, with G > 1 from s; last and copy are not
    touched (they are not even passed on)."""
    scratch = np.empty((st.G + 1) * st.n, np.float32)
    lib().cbr_elastic_average(st.G, st.size, st.n, st.alpha, O._fpp(st.z), O._fpp(st.s), O._fpp(st.w),
                              _ip(st.locked), st.first, O._fp(scratch))


def polyak_ruppert(st: O.SmaState, clock: int) -> int:
    """One Polyak-Ruppert step on z, w, last (where st.last exists) and the
    copy flags, in place.  Returns how many replicas took z."""
    assert clock >= 0
    scratch = np.empty((st.G + 1) * st.n, np.float32)
    lp = O._fpp(st.last) if st.last is not None else None
    return lib().cbr_polyak_ruppert(st.G, st.size, st.n, st.alpha, clock, O._fpp(st.z), lp, O._fpp(st.w),
                                    _ip(st.locked), _ip(st.copy), st.first, O._fp(scratch))


def step(st: O.SmaState, polyak: bool, clock: int = 0) -> None:
    if polyak:
        polyak_ruppert(st, clock)
    else:
        elastic_average(st)
