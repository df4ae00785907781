"""GPU parity of gradient clipping by global norm and the non-finite skip in
the context's replica step (``cbx_set_gradient_clip``).  The oracle is
tests/gradient_clip_common.py: S by exact fp64 on the host, the decision and
the scale as the header defines them, ``g <- float32(scale) * g``, then the
oracle's replica step unchanged.

Shapes: n = 1 (under one float4), 4,097 (one tile plus one float) and 262,149
(65 tiles: the reduce's second round, and the pad, are live).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact

pytestmark = pytest.mark.gpu

SHAPES = [1, 4097, 262149]
KINDS = ("w", "g", "last", "s")
AUX_CONFIGS = [(64, 2, 2), (256, 1, 0), (512, 1, 8)]
ZERO = {"sum_sq": 0.0, "nonfinite": 0, "scale": 0.0, "flags": 0, "steps": 0, "clipped_steps": 0, "skipped_steps": 0}

sweep = pytest.mark.parametrize("n,momentum,wd", [(n, m, wd) for n in SHAPES for m in (0.0, 0.9) for wd in (0.0, 5e-4)])


_gpu, _put, _get = C.context, C.put, C.get


def _check(gpu, i, bufs, what="", nans=False):
    got = _get(gpu, i, 1.0 if bufs[2] is not None else 0.0)
    for name, a, b in zip(KINDS, got, bufs):
        if b is not None:
            (C.assert_same_with_nans if nans else assert_bitexact)(a, b, f"{what}{name}[{i}]")


@sweep
def test_off_by_default_is_the_plain_step_and_the_record_stays_zero(n, momentum, wd):
    gpu = _gpu(n, momentum, wd)
    try:
        bufs = C.host(100, n, momentum)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        O.sma_optimise(np.float32(-C.LR), momentum, wd, *bufs)
        _check(gpu, 0, bufs)
        assert gpu.replica_clip_stats(0) == ZERO
        # on, then off again: the plain path once more, the record untouched
        gpu.set_gradient_clip(1.0, True)
        gpu.set_gradient_clip(0.0, False)
        gpu.replica_optimise(0, task=1)
        gpu.wait()
        O.sma_optimise(np.float32(-C.LR), momentum, wd, *bufs)
        _check(gpu, 0, bufs, "off again: ")
        assert gpu.replica_clip_stats(0) == ZERO
    finally:
        gpu.free()


@sweep
def test_a_norm_that_never_clips_is_bit_identical_to_the_plain_step(n, momentum, wd):
    gpu = _gpu(n, momentum, wd)
    try:
        gpu.set_gradient_clip(1e30, False)
        bufs = C.host(110, n, momentum)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        O.sma_optimise(np.float32(-C.LR), momentum, wd, *bufs)
        _check(gpu, 0, bufs)
        rec = gpu.replica_clip_stats(0)
        assert (rec["flags"], rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == (0, 1, 0, 0), rec
        assert rec["scale"] == 1.0 and rec["nonfinite"] == 0, rec
    finally:
        gpu.free()


@sweep
def test_exact_case_with_no_device_value_in_the_expectation(n, momentum, wd):
    gpu = _gpu(n, momentum, wd)
    try:
        bufs = C.host(120, n, momentum)
        bufs[1], S, c = C.exact_gradient(n)
        gpu.set_gradient_clip(c, False)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        scale, flags = C.decide(S, 0, c, False)
        assert (float(scale), flags) == (0.5, C.CLIPPED)
        C.step(bufs, scale, flags, momentum, wd)
        _check(gpu, 0, bufs)
        rec = gpu.replica_clip_stats(0)
        assert rec == {"sum_sq": S, "nonfinite": 0, "scale": 0.5, "flags": C.CLIPPED, "steps": 1, "clipped_steps": 1,
                       "skipped_steps": 0}, rec
    finally:
        gpu.free()


@sweep
def test_normal_data_clips_to_the_norm(n, momentum, wd):
    gpu = _gpu(n, momentum, wd)
    try:
        bufs = C.host(130, n, momentum)
        S_ref, K = C.exact_sum_sq(bufs[1])
        c = float(np.float32(0.25 * np.sqrt(S_ref)))  # clips to a quarter of the norm
        gpu.set_gradient_clip(c, False)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        # the reordering bound of a sum of n non-negative terms in fp64
        assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref, (rec["sum_sq"], S_ref)
        scale, flags = C.decide(rec["sum_sq"], K, c, False)
        assert flags == C.CLIPPED and rec["flags"] == C.CLIPPED and rec["nonfinite"] == 0
        assert np.float32(rec["scale"]).view(np.uint32) == scale.view(np.uint32), (rec["scale"], scale)
        g_clipped = (scale * bufs[1]).astype(np.float64)
        assert abs(np.sqrt(np.sum(g_clipped * g_clipped)) - c) <= 1e-6 * c
        C.step(bufs, scale, flags, momentum, wd)
        _check(gpu, 0, bufs)
    finally:
        gpu.free()


@pytest.mark.parametrize("n", SHAPES)
def test_sum_is_the_same_bits_whatever_the_launch_shape_or_stream(n):
    import torch
    momentum, wd = 0.9, 5e-4
    gpu = _gpu(n, momentum, wd)
    try:
        gpu.set_gradient_clip(1e30, False)  # scale 1: g keeps its bits from call to call
        bufs = C.host(140, n, momentum)
        _put(gpu, 0, bufs)
        sums = []
        stream = torch.cuda.Stream()
        for k, (aux, st) in enumerate([(None, None), (None, None)] + [(a, None) for a in AUX_CONFIGS] +
                                      [(None, stream)]):
            if aux:
                gpu.set_aux_kernel_config(*aux)
            else:
                gpu.set_aux_kernel_config()
            from crossbow_amd import BUF_GRADIENT
            gpu.replica_write(0, BUF_GRADIENT, bufs[1])
            gpu.replica_optimise(0, task=k, stream=st.cuda_stream if st else None)
            gpu.wait()
            sums.append(np.float64(gpu.replica_clip_stats(0)["sum_sq"]).view(np.uint64))
        assert len(set(int(s) for s in sums)) == 1, sums
        assert gpu.replica_clip_stats(0)["steps"] == len(sums)
    finally:
        gpu.free()


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("skip", [False, True])
def test_nonfinite_gradients(n, momentum, wd, skip):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT
    from tests.helpers import compare_states, download, upload
    R, alpha = 2, 0.1
    gpu = _gpu(n, momentum, wd, replicas=R, alpha=alpha)
    try:
        st = O.make_state(n, 1, R, alpha, momentum)
        upload(gpu, st)
        gpu.set_gradient_clip(0.5, skip)
        bufs = C.host(150, n, momentum)
        pos = C.nonfinite_positions(n)
        for p, v in zip(pos, (np.nan, np.inf, -np.inf)):
            bufs[1][p] = v
        S_ref, K = C.exact_sum_sq(bufs[1])
        assert K == len(pos)
        before = [None if b is None else b.copy() for b in bufs]
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        assert rec["nonfinite"] == K
        assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref
        scale, flags = C.decide(rec["sum_sq"], K, 0.5, skip)
        assert rec["flags"] == flags and bool(flags & C.SKIPPED) == skip
        assert np.float32(rec["scale"]).view(np.uint32) == scale.view(np.uint32)
        assert (rec["steps"], rec["skipped_steps"]) == (1, 1 if skip else 0)
        C.step(bufs, scale, flags, momentum, wd)
        if not skip:
            _check(gpu, 0, bufs, nans=True)
            return
        # skipped: s = the old w; w, g and last keep their bits (the NaN's too)
        got = _get(gpu, 0, momentum)
        assert_bitexact(got[3], before[0], "s = w")
        for k in (0, 2):
            if before[k] is not None:
                assert_bitexact(got[k], before[k], f"{KINDS[k]} unchanged")
        assert np.array_equal(got[1].view(np.uint32), before[1].view(np.uint32)), "g unchanged, bit for bit"
        # and the next barrier sees "no local movement" on replica 0
        st.w[0][:], st.s[0][:] = before[0], before[0]
        gpu.lockAny()
        gpu.synchronise(0, 1, 0, False)
        gpu.unlockAny()
        gpu.wait()
        O.sma_step(st)
        compare_states(download(gpu, st), st)
        assert_bitexact(gpu.replica_read(0, BUF_DATA), st.w[0], "w[0] after the barrier")
    finally:
        gpu.free()


def test_pad_of_the_gradient_is_never_read():
    import ctypes
    from crossbow_amd import BUF_GRADIENT
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    n = 262149  # padded to 263168 floats (1024 float4s): 1019 floats of pad
    padded = (((n + 3) // 4 + 1023) // 1024) * 1024 * 4
    gpu = _gpu(n, 0.9, 5e-4)
    try:
        bufs = C.host(160, n, 0.9)
        S_ref, _ = C.exact_sum_sq(bufs[1])
        c = float(np.float32(0.25 * np.sqrt(S_ref)))
        gpu.set_gradient_clip(c, True)
        _put(gpu, 0, bufs)
        gpu.wait()
        pad = np.full(padded - n, 1e30, np.float32)
        assert hip.hipMemcpy(gpu.replica_buffer(0, BUF_GRADIENT) + 4 * n, pad.ctypes.data, pad.nbytes, 1) == 0
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref, (rec["sum_sq"], S_ref)
        scale, flags = C.decide(rec["sum_sq"], 0, c, True)
        assert rec["flags"] == flags == C.CLIPPED
        C.step(bufs, scale, flags, 0.9, 5e-4)
        _check(gpu, 0, bufs)
    finally:
        gpu.free()  # the pad no longer holds zeros: the context ends here


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_per_variable_rates_with_clipping_and_the_refusals(momentum, wd):
    from crossbow_amd import CbxError, _lib
    from tests.test_optimise_plan import M, V
    n = sum(V)
    gpu = _gpu(n, momentum, wd, variables=list(V), mults=M)
    try:
        gpu.set_variable_learning_rates(True)
        bufs = C.host(170, n, momentum)
        S_ref, _ = C.exact_sum_sq(bufs[1])
        c = float(np.float32(0.5 * np.sqrt(S_ref)))
        gpu.set_gradient_clip(c, False)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        rec = gpu.replica_clip_stats(0)
        scale, flags = C.decide(rec["sum_sq"], 0, c, False)
        assert flags == C.CLIPPED == rec["flags"]
        C.step(bufs, scale, flags, momentum, wd, variables=V, mults=M)
        _check(gpu, 0, bufs)
        with pytest.raises(CbxError) as e:
            gpu.replica_optimise_variables(0, task=1, op=3)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED and "global norm" in str(e.value), e.value
        gpu.wait()
        _check(gpu, 0, bufs, "after the refusal: ")
        gpu.set_gradient_clip(0.0, False)  # off again: the per-operator step works as before
        gpu.replica_optimise_variables(0, task=1, op=3)
        gpu.wait()
        from tests.test_optimise_plan import per_variable_step
        per_variable_step(C.LR, M, momentum, wd, *bufs, only={3})
        _check(gpu, 0, bufs, "off again: ")
    finally:
        gpu.free()


@pytest.mark.parametrize("update_type", [0, 1])  # DEFAULT, WORKER
def test_worker_and_default_are_refused_while_the_feature_is_on(update_type):
    from crossbow_amd import CbxError, _lib
    gpu = _gpu(4097, 0.9, 5e-4, update_type=update_type)
    try:
        gpu.set_gradient_clip(1.0, False)
        with pytest.raises(CbxError) as e:
            gpu.replica_optimise(0, task=0)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, e.value
        assert ("WORKER" if update_type == 1 else "DEFAULT") in str(e.value)
        gpu.set_gradient_clip(0.0, False)
        gpu.replica_optimise(0, task=0)  # as before
        gpu.wait()
    finally:
        gpu.free()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_clock_loop_on_two_task_streams(momentum):
    import torch
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    from tests.helpers import compare_states, download, upload
    n, R, clocks, alpha, wd = 4097, 3, 3, 0.1, 1e-4
    sigma = 0.01
    c = float(np.float32(sigma * np.sqrt(n)))  # about the expected norm: some tasks clip, some do not
    gpu = _gpu(n, momentum, wd, replicas=R, alpha=alpha)
    try:
        gpu.set_gradient_clip(c, True)
        st = O.make_state(n, 1, R, alpha, momentum)
        upload(gpu, st)
        lasts = [np.zeros(n, np.float32) if momentum > 0 else None for _ in range(R)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        want = [dict(steps=0, clipped_steps=0, skipped_steps=0) for _ in range(R)]
        task = 0
        for clock in range(1, clocks + 1):
            pending = []
            for i in range(R):
                gr = O.fill_normal(n, 2000 + task, sigma * (0.8 + 0.2 * ((task * 7) % 3)))
                if task == 4:
                    gr[n // 2] = np.inf  # one task of the loop is skipped
                gpu.replica_write(i, BUF_GRADIENT, gr)
                gpu.replica_optimise(i, task, stream=streams[i % 2].cuda_stream)
                pending.append((i, gr))
                task += 1
            gpu.wait()
            for i, gr in pending:
                rec = gpu.replica_clip_stats(i)
                S_ref, K = C.exact_sum_sq(gr)
                assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref
                scale, flags = C.decide(rec["sum_sq"], K, c, True)
                assert rec["flags"] == flags and rec["nonfinite"] == K
                want[i]["steps"] += 1
                want[i]["clipped_steps"] += 1 if flags & C.CLIPPED else 0
                want[i]["skipped_steps"] += 1 if flags & C.SKIPPED else 0
                C.step([st.w[i], gr, lasts[i], st.s[i]], scale, flags, momentum, wd)
            gpu.lockAny()
            gpu.synchronise(0, clock, 0, False)
            gpu.unlockAny()
            O.sma_step(st)
        gpu.wait()
        compare_states(download(gpu, st), st)
        if momentum > 0:
            for i in range(R):
                assert_bitexact(gpu.replica_read(i, BUF_LAST), lasts[i], f"replica last[{i}]")
        got = [{k: gpu.replica_clip_stats(i)[k] for k in want[i]} for i in range(R)]
        assert got == want, (got, want)
        total = {k: sum(w[k] for w in want) for k in want[0]}
        assert total["steps"] == R * clocks and total["skipped_steps"] == 1
        assert 0 < total["clipped_steps"] < total["steps"], total  # it clips on some tasks and not on others
    finally:
        gpu.free()


def test_added_replica_clips_like_the_others():
    n, momentum, wd, R = 4097, 0.9, 5e-4, 2
    gpu = _gpu(n, momentum, wd, replicas=R)
    try:
        gpu.set_gradient_clip(0.25, False)
        bufs0 = C.host(180, n, momentum)
        _put(gpu, 0, bufs0)
        gpu.replica_optimise(0, task=0)  # replica 0's record counts a step ...
        gpu.addModel()  # ... and the new replica, its copy, starts a record of its own
        gpu.unlockAny()
        assert gpu.num_replicas() == R + 1
        assert gpu.replica_clip_stats(R) == ZERO
        bufs = C.host(190, n, momentum)
        _put(gpu, R, bufs)
        gpu.replica_optimise(R, task=1)
        gpu.wait()
        rec = gpu.replica_clip_stats(R)
        scale, flags = C.decide(rec["sum_sq"], 0, 0.25, False)
        assert flags == C.CLIPPED == rec["flags"] and rec["steps"] == 1
        C.step(bufs, scale, flags, momentum, wd)
        _check(gpu, R, bufs)
        assert gpu.replica_clip_stats(0)["steps"] == 1
    finally:
        gpu.free()


def test_invalid_arguments_are_refused():
    from crossbow_amd import CbxError, _lib
    gpu = _gpu(4097, 0.9, 5e-4)
    try:
        for args in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (1.0, 2), (1.0, -1)):
            with pytest.raises(CbxError) as e:
                _lib.check(gpu._L.cbx_set_gradient_clip(gpu._ctx, args[0], args[1]))
            assert e.value.code == _lib.CBX_ERR_INVALID, (args, e.value)
        with pytest.raises(CbxError) as e:
            gpu.replica_clip_stats(7)
        assert e.value.code == _lib.CBX_ERR_INVALID
        # nothing was switched on by the refused calls
        bufs = C.host(200, 4097, 0.9)
        _put(gpu, 0, bufs)
        gpu.replica_optimise(0, task=0)
        gpu.wait()
        assert gpu.replica_clip_stats(0) == ZERO
    finally:
        gpu.free()
