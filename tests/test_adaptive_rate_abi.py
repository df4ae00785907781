"""The entry points of the adaptive-rate step without a GPU: a NULL context or plan is an error, not a crash."""
from __future__ import annotations

import ctypes


def test_a_null_context_or_plan_is_an_error_not_a_crash():
    from crossbow_amd import _lib
    lib = _lib.load()
    out = _lib.AdaptiveStats()
    assert ctypes.sizeof(out) == 32
    for rc in (lib.cbx_set_adaptive_rate(None, 0.01, 1e-9, 0),
               lib.cbx_set_model_variable_adaptive_rate(None, 0, 1, 0),
               lib.cbx_replica_adaptive_stats(None, 0, ctypes.byref(out), 1),
               lib.cbx_sma_plan_set_adaptive(None, None, 1),
               lib.cbx_sma_plan_optimise_adaptive(None, 0, 0, None, None, None, None, None, 0.1, 0.9, 0.0, 0.01, 0.0, 0),
               lib.cbx_set_adaptive_kernel_policy(None, 0),
               lib.cbx_sma_plan_optimise_adaptive_timed(None, 0, 0, None, None, None, None, None, 0.1, 0.9, 0.0, 0.01, 0.0,
                                                        0, -1, None, None, None),
               lib.cbx_sma_plan_adaptive_stats(None, 0, 0, None, ctypes.byref(out), 1)):
        assert rc == _lib.CBX_ERR_INVALID and b"null" in lib.cbx_last_error()
