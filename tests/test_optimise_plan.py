"""The per-variable replica step without a GPU: the chunk-table builder
(crossbow_amd/csrc/optimise_plan.h) driven by a stand-alone program under
ASan + UBSan, the new calls on a NULL context or plan, and the reference the
GPU tests use (the oracle's replica step called once per variable on slices of
the model buffers) against its own OpenBLAS replay on unaligned slices."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_bitexact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The shape every variable-rate test shares: boundaries at 1, 4, 39, 4132,
# 8228 and 9228; the first float4 holds two whole variables and part of a
# third; the 4096-float variable spans 17 chunks, a boundary in each end one;
# n = 21523 is odd, so the last variable ends in a 3-float tail.
V = (1, 3, 35, 4093, 4096, 1000, 12295)
M = (2.0, 1.0, 0.0, 0.5, 1.0, 10.0, 0.1)
LR = 0.05


def per_variable_step(lr, mults, momentum, wd, w, g, last, s, variables=V, only=None, blas=False):
    """The reference's per-variable call sequence (model.c:159-177): the
    oracle's replica step once per variable, on slices, with the rate
    -lr x multiplier in fp32.  ``only``: the variable indices to step."""
    lo = 0
    for v, count in enumerate(variables):
        hi = lo + count
        if count and (only is None or v in only):
            O.sma_optimise(np.float32(-lr) * np.float32(mults[v]), momentum, wd, w[lo:hi], g[lo:hi],
                           last[lo:hi] if last is not None else None, s[lo:hi], blas=blas)
        lo = hi


def test_chunk_table_builder_under_asan_and_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "optimise_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "crossbow_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "optimise_plan_test.cpp")],
                       check=True, capture_output=True, timeout=240)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.startswith("ok "), p.stdout


def test_new_calls_on_a_null_context_or_plan_are_errors_not_crashes():
    from crossbow_amd import _lib
    lib = _lib.load()
    assert lib.cbx_set_variable_learning_rates(None, 1) == _lib.CBX_ERR_INVALID
    assert lib.cbx_replica_optimise_variables(None, 0, 0, 0, None) == _lib.CBX_ERR_INVALID
    ve = (ctypes.c_longlong * 1)(4)
    assert lib.cbx_sma_plan_set_variables(None, ve, None, 1) == _lib.CBX_ERR_INVALID
    assert lib.cbx_sma_plan_optimise_variables(None, 0, None, None, None, None, None, 0.1, 0.0, 0.0, 0,
                                               1) == _lib.CBX_ERR_INVALID
    assert b"null" in lib.cbx_last_error()


def test_new_symbols_are_declared_in_the_header_and_the_binding():
    from crossbow_amd import _abi
    with open(os.path.join(ROOT, "include", "crossbow_sma.h")) as f:
        header = f.read()
    for name in ("cbx_set_variable_learning_rates", "cbx_replica_optimise_variables", "cbx_sma_plan_set_variables",
                 "cbx_sma_plan_optimise_variables"):
        assert f"int {name} (" in header, name
        assert name in _abi.SIGNATURES, name


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_per_slice_oracle_equals_its_openblas_replay(momentum, wd):
    # The slices start at odd offsets (1, 4, 39, 4132, ...): OpenBLAS takes
    # its unaligned paths there, and must still give the fma sequence's bits.
    n = sum(V)
    bufs = []
    for blas in (False, True):
        w = O.fill_normal(n, 500, 0.05)
        g = O.fill_normal(n, 501, 0.01)
        last = O.fill_normal(n, 502, 0.001) if momentum > 0 else None
        s = np.zeros(n, np.float32)
        per_variable_step(LR, M, momentum, wd, w, g, last, s, blas=blas)
        bufs.append((w, g, last, s))
    for a, b, what in zip(bufs[0], bufs[1], ("w", "g", "last", "s")):
        if a is not None:
            assert_bitexact(a, b, what)
    # and the multipliers matter: variable 0 (x 2) and variable 5 (x 10) moved
    # differently from a step with the one rate
    w1 = O.fill_normal(n, 500, 0.05)
    g1 = O.fill_normal(n, 501, 0.01)
    l1 = O.fill_normal(n, 502, 0.001) if momentum > 0 else None
    O.sma_optimise(np.float32(-LR), momentum, wd, w1, g1, l1, np.zeros(n, np.float32))
    assert not np.array_equal(bufs[0][0][:1], w1[:1])
    assert not np.array_equal(bufs[0][0][8228:9228], w1[8228:9228])
    assert_bitexact(bufs[0][0][1:4], w1[1:4], "multiplier 1 is the plain step")
