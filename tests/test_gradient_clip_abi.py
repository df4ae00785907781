"""Gradient clipping by global norm without a GPU: the new calls are declared
in the header, bound in ``crossbow_amd._abi`` and exported by the built
library; ``cbx_clip_stats`` is 48 bytes without padding; ``thegpu.py`` and
``seam.py`` expose the calls; NULL handles are errors, not crashes."""
from __future__ import annotations

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cbx_set_gradient_clip", "cbx_replica_clip_stats", "cbx_sma_plan_optimise_clipped",
       "cbx_sma_plan_clip_stats", "cbx_sma_plan_gradient_norm")


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
    for name in NEW:
        m = re.search(r"int %s \(([^;]*)\);" % name, header)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert nargs == len(_abi.SIGNATURES[name][1]), (name, m.group(1))


def test_clip_stats_is_48_bytes_without_padding():
    from crossbow_amd import _abi
    assert ctypes.sizeof(_abi.ClipStats) == 48
    offsets = {n: getattr(_abi.ClipStats, n).offset for n, _ in _abi.ClipStats._fields_}
    assert offsets == {"sum_sq": 0, "nonfinite": 8, "scale": 16, "flags": 20, "steps": 24, "clipped_steps": 32,
                       "skipped_steps": 40}
    # the header's struct, field for field and in that order
    m = re.search(r"typedef struct cbx_clip_stats \{(.*?)\} cbx_clip_stats;", _header(), re.S)
    assert m
    names = re.findall(r"(\w+);", m.group(1))
    assert names == [n for n, _ in _abi.ClipStats._fields_]
    assert (_abi.CLIP_CLIPPED, _abi.CLIP_SKIPPED) == (1, 2)
    assert "#define CBX_CLIP_CLIPPED 1u" in _header() and "#define CBX_CLIP_SKIPPED 2u" in _header()


def test_python_wrappers_expose_the_calls():
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.thegpu import TheGPU
    assert callable(TheGPU.set_gradient_clip) and callable(TheGPU.replica_clip_stats)
    assert callable(SmaPlan.optimise_clipped) and callable(SmaPlan.clip_stats) and callable(SmaPlan.gradient_norm)


def test_null_handles_are_errors_not_crashes():
    from crossbow_amd import _abi, _lib
    lib = _lib.load()
    out = _abi.ClipStats()
    assert lib.cbx_set_gradient_clip(None, 1.0, 0) == _lib.CBX_ERR_INVALID
    assert lib.cbx_replica_clip_stats(None, 0, ctypes.byref(out)) == _lib.CBX_ERR_INVALID
    assert lib.cbx_sma_plan_optimise_clipped(None, 0, 0, None, None, None, None, None, 0.1, 0.0, 0.0, 1.0, 0,
                                             0) == _lib.CBX_ERR_INVALID
    assert lib.cbx_sma_plan_clip_stats(None, 0, 0, None, ctypes.byref(out)) == _lib.CBX_ERR_INVALID
    assert lib.cbx_sma_plan_gradient_norm(None, 0, 0, None, None, 1.0, 0, -1, None, None) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_jni_shim_reads_the_environment_switches():
    with open(os.path.join(ROOT, "crossbow_amd", "csrc", "jni", "TheGPU_jni.c")) as f:
        src = f.read()
    assert 'getenv ("CBX_GRADIENT_CLIP")' in src
    assert '"CBX_SKIP_NONFINITE_GRADIENTS"' in src
    assert "cbx_set_gradient_clip (theGPU" in src
