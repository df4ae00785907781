"""The model-statistics additions to the C-ABI, without a GPU: the layout of
``cbx_buffer_stats`` in the header and in the ctypes binding, the new calls on
a NULL context, and the piece-table builder (crossbow_amd/csrc/stats_plan.h)
driven by a stand-alone program under ASan + UBSan."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZEOF_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "crossbow_sma.h"
_Static_assert (sizeof (cbx_buffer_stats) == 40, "cbx_buffer_stats must be 40 bytes");
int main (void) {
  printf ("%zu %zu %zu %zu %zu %zu %zu\n", sizeof (cbx_buffer_stats), offsetof (cbx_buffer_stats, sum),
          offsetof (cbx_buffer_stats, sum_sq), offsetof (cbx_buffer_stats, dist_sq),
          offsetof (cbx_buffer_stats, nonfinite), offsetof (cbx_buffer_stats, max_abs),
          offsetof (cbx_buffer_stats, reserved));
  return 0;
}
"""


def test_buffer_stats_is_40_bytes_in_c_and_in_ctypes():
    from crossbow_amd import _abi
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizeof.c"), os.path.join(d, "sizeof")
        with open(src, "w") as f:
            f.write(SIZEOF_C)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src],
                       check=True, capture_output=True, timeout=120)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    c_layout = [int(x) for x in out]
    assert c_layout == [40, 0, 8, 16, 24, 32, 36]
    S = _abi.BufferStats
    assert ctypes.sizeof(S) == 40
    assert [S.sum.offset, S.sum_sq.offset, S.dist_sq.offset, S.nonfinite.offset, S.max_abs.offset,
            S.reserved.offset] == c_layout[1:]
    dt = np.dtype(_abi.BUFFER_STATS_FIELDS)
    assert dt.itemsize == 40
    assert [dt.fields[n][1] for n in dt.names] == c_layout[1:]
    assert list(dt.names) == [f[0] for f in S._fields_]


def test_new_calls_on_a_null_context_are_errors_not_crashes():
    from crossbow_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int(7)
    one = (_lib.BufferStats * 1)()
    f = ctypes.c_float(0)
    ll = ctypes.c_longlong(0)
    assert lib.cbx_model_variable_count(None, ctypes.byref(n)) == _lib.CBX_ERR_INVALID
    assert lib.cbx_model_variable_info(None, 0, ctypes.byref(n), ctypes.byref(n), ctypes.byref(ll),
                                       ctypes.byref(ll)) == _lib.CBX_ERR_INVALID
    assert lib.cbx_model_stats(None, _lib.BUF_DATA, one, one, None, None) == _lib.CBX_ERR_INVALID
    assert lib.cbx_model_stats_last_ms(None, 0, ctypes.byref(f), ctypes.byref(f)) == _lib.CBX_ERR_INVALID
    assert lib.cbx_set_checkpoint_guard(None, 1) == _lib.CBX_ERR_INVALID
    assert lib.cbx_sma_plan_buffer_stats(None, 0, None, None, None, 0, None, 0, one, one, None,
                                         None) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_piece_table_builder_under_asan_and_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stats_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "crossbow_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "stats_plan_test.cpp")],
                       check=True, capture_output=True, timeout=240)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.startswith("ok "), p.stdout
