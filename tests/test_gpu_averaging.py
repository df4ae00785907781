"""The elastic-averaging and Polyak-Ruppert barriers on one GPU, through
``TheGPU`` and the C-ABI (run with -m gpu).

Bar: as for SMA at G = 1, the kernels use the reference's
fp32 operation order, one fma per cuBLAS saxpy element, so every array must be
BIT-EXACT with the CPU restatement (tests/native/averaging_ref.c, pinned by
tests/test_averaging_ref.py).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests.helpers import assert_bitexact, compare_states, download, upload

pytestmark = pytest.mark.gpu

EA, PR = "elastic", "polyak"


def _make(model, n, R, alpha, momentum, sync=0, wd=0.0):
    """A context whose update model runs `model`: EA, PR, or an update model id
    with the elastic switch left alone."""
    import crossbow_amd
    g = crossbow_amd.TheGPU()
    g.init([0])
    try:
        g.setModel(1, 4 * n)
        g.setModelVariable(0, 1, [n], 4 * n)
        if model == EA:
            g.setUpdateModelType(crossbow_amd.UPDATE_SYNCHRONOUSEAMSGD)
            g.setElasticAverage(True)
        elif model == PR:
            g.setUpdateModelType(crossbow_amd.UPDATE_POLYAK_RUPPERT)
        else:
            g.setUpdateModelType(model)
        g.setEamsgdAlpha(alpha)
        g.setMomentum(momentum, 0)
        g.setWeightDecay(wd)
        g.setLearningRateDecayPolicyFixed(0.05)
        g.setModelManager(R, sync)
    except Exception:
        g.free()
        raise
    return g


def _barrier(g, want, model, clock, first=0, held=(), staged=0):
    """One barrier on the GPU and the same step on `want`."""
    R = want.size
    for i in held:
        g.replica_lock(i)  # busy on the task side: lockAny (SSP) skips it
    g.lockAny()
    want.locked[:] = 1
    for i in held:
        want.locked[i] = 0
    want.first = first
    if staged:
        g.synchronise_staged(first, clock, 0, staged)
    else:
        g.synchronise(first, clock, 0, False)
    assert g.unlockAny() == R - len(held)
    for i in held:
        g.replica_unlock(i)
    AV.step(want, model == PR, clock)


def _run(model, n, R, alpha, momentum, first=0, held=(), config=None, split=False, bucket=0, clocks=(0,),
         copy_ids=()):
    st = O.make_state(n, 1, R, alpha, momentum)
    g = _make(model, n, R, alpha, momentum, sync=1 if held else 0)
    try:
        if config:
            g.set_kernel_config(policy=config["policy"])
            g.set_averaging_kernel_config(config["block"], config["unroll"], config["waves"])
        if split:
            g.set_force_split(True)
        if bucket:
            g.set_bucket_elements(bucket)
        upload(g, st)
        want = st.clone()
        for i in copy_ids:
            g.set_replica_copy(i, True)
            want.copy[i] = 1
        for clock in clocks:
            _barrier(g, want, model, clock, first=first, held=held)
        g.wait()
        got = download(g, st)
        compare_states(got, want)
        for i in range(R):
            assert g.replica_copy(i) == want.copy[i], f"copy flag of replica {i}"
        return got
    finally:
        g.free()


# n: below one float4, a ragged float4, under one workgroup's trip, several
# workgroups, several buckets' worth.  R: the unrolled kernels, the chunk
# boundary (kChunk = 8) and two and three chunk walks.
SHAPES = [
    dict(n=1, R=1, alpha=0.1, momentum=0.0),
    dict(n=3, R=2, alpha=0.5, momentum=0.9),
    dict(n=1031, R=8, alpha=0.1, momentum=0.9),
    dict(n=1031, R=9, alpha=0.0, momentum=0.0),
    dict(n=1031, R=17, alpha=0.1, momentum=0.9),
    dict(n=50_000, R=2, alpha=0.0, momentum=0.9),
    dict(n=50_000, R=8, alpha=0.5, momentum=0.0, held=(3,)),
    dict(n=50_000, R=9, alpha=0.1, momentum=0.9, first=2),
    dict(n=300_001, R=1, alpha=0.1, momentum=0.9),
    dict(n=300_001, R=8, alpha=0.1, momentum=0.0),
    dict(n=300_001, R=17, alpha=0.5, momentum=0.9, held=(0,)),
    # a small launch runs a grid-stride loop over 8 one-wave workgroups per CU
    # (small_launch_shape): 131072 float4s a trip, so this one takes a second, partial trip
    dict(n=600_001, R=2, alpha=0.1, momentum=0.9),
    # past 16 waves per CU the launch is one trip per lane under the occupancy cap
    dict(n=1_111_946, R=2, alpha=0.1, momentum=0.0),
    # plain loads / stores, four float4s per lane, 256-thread workgroups, no cap
    dict(n=50_000, R=2, alpha=0.1, momentum=0.9, config=dict(block=256, unroll=4, waves=0, policy=0)),
    # two float4s per lane, 128-thread workgroups, capped at 6 waves per CU
    dict(n=300_001, R=8, alpha=0.1, momentum=0.9, config=dict(block=128, unroll=2, waves=6, policy=1)),
]


@pytest.mark.parametrize("model", [EA, PR])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"n{c['n']}-R{c['R']}" + ("-config" if "config" in c else ""))
def test_step_bitexact(model, case):
    _run(model, clocks=(3,), **case)


@pytest.mark.parametrize("model", [EA, PR])
def test_disabled_theta_slot_is_counted_but_left_out(model):
    n, R = 1031, 4
    st = O.make_state(n, 1, R, 0.1, 0.9)
    g = _make(model, n, R, 0.1, 0.9)
    try:
        upload(g, st)
        g.set_replica_disabled(2, True)
        assert g.lockAny() == R
        g.synchronise(0, 5, 0, False)
        assert g.unlockAny() == R - 1
        want = st.clone()
        want.locked[2] = 0
        AV.step(want, model == PR, 5)
        g.wait()
        compare_states(download(g, st), want)
        assert g.replica_clock(2) == 0 and g.replica_clock(1) == 5
    finally:
        g.free()


@pytest.mark.parametrize("model", [EA, PR])
def test_three_steps_with_their_clocks(model):
    _run(model, 1031, 4, 0.1, 0.9, clocks=(0, 1, 2))


def test_polyak_depends_on_the_clock():
    a = _run(PR, 1031, 4, 0.1, 0.0, clocks=(0,))
    b = _run(PR, 1031, 4, 0.1, 0.0, clocks=(1,))
    assert not np.array_equal(a.z[0].view(np.uint32), b.z[0].view(np.uint32))
    for i in range(4):  # the replicas' move does not
        assert_bitexact(a.w[i], b.w[i], f"w[{i}]")


def test_polyak_copies_into_the_flagged_replica_only():
    got = _run(PR, 1031, 4, 0.1, 0.9, clocks=(2,), copy_ids=(1,))  # _run checks the flags too
    assert_bitexact(got.w[1], got.z[0], "the flagged replica")
    for i in (0, 2, 3):
        assert not np.array_equal(got.w[i].view(np.uint32), got.z[0].view(np.uint32))


def test_polyak_split_copies_into_the_flagged_replica_only():
    _run(PR, 1031, 4, 0.1, 0.9, clocks=(2,), copy_ids=(1,), split=True)


def test_elastic_leaves_a_raised_copy_flag_raised():
    got = _run(EA, 1031, 4, 0.1, 0.9, copy_ids=(1,))  # _run: the flag is still 1, as the restatement leaves it
    assert not np.array_equal(got.w[1].view(np.uint32), got.z[0].view(np.uint32))


# ---- routing -------------------------------------------------------------------
def _one_step(g, st, clock=1):
    upload(g, st)
    g.lockAny()
    g.synchronise(0, clock, 0, False)
    g.unlockAny()
    g.wait()
    return download(g, st)


def test_type_3_with_the_switch_off_is_sma():
    # The no-regression guard: nothing here touches the new interface.
    from crossbow_amd import UPDATE_SYNCHRONOUSEAMSGD
    st = O.make_state(4099, 1, 4, 0.1, 0.9)
    g = _make(UPDATE_SYNCHRONOUSEAMSGD, 4099, 4, 0.1, 0.9)
    try:
        got = _one_step(g, st)
    finally:
        g.free()
    want = st.clone()
    O.sma_step(want)
    compare_states(got, want)


def test_type_3_with_the_switch_on_is_elastic_averaging_and_off_again_is_sma():
    from crossbow_amd import UPDATE_SYNCHRONOUSEAMSGD
    st = O.make_state(4099, 1, 4, 0.1, 0.9)
    g = _make(UPDATE_SYNCHRONOUSEAMSGD, 4099, 4, 0.1, 0.9)
    try:
        g.setElasticAverage(True)
        got = _one_step(g, st)
        want = st.clone()
        AV.elastic_average(want)
        compare_states(got, want)
        g.setElasticAverage(False)
        got = _one_step(g, st)
        want = st.clone()
        O.sma_step(want)
        compare_states(got, want)
    finally:
        g.free()


def test_type_7_with_the_switch_on_is_still_sma():
    from crossbow_amd import UPDATE_SMA
    st = O.make_state(4099, 1, 4, 0.1, 0.9)
    g = _make(UPDATE_SMA, 4099, 4, 0.1, 0.9)
    try:
        g.setElasticAverage(True)
        got = _one_step(g, st)
    finally:
        g.free()
    want = st.clone()
    O.sma_step(want)
    compare_states(got, want)


def test_type_6_is_polyak_ruppert():
    st = O.make_state(4099, 1, 4, 0.1, 0.9)
    g = _make(PR, 4099, 4, 0.1, 0.9)
    try:
        got = _one_step(g, st, clock=4)
    finally:
        g.free()
    want = st.clone()
    AV.polyak_ruppert(want, 4)
    compare_states(got, want)


def test_refusals():
    from crossbow_amd import CbxError, _lib
    g = _make(PR, 1031, 2, 0.1, 0.0)
    try:
        L = _lib.load()
        assert L.cbx_set_elastic_average(g.ctx, 2) == _lib.CBX_ERR_INVALID
        assert L.cbx_set_elastic_average(g.ctx, -1) == _lib.CBX_ERR_INVALID
        assert L.cbx_set_averaging_kernel_config(g.ctx, 64, 3, -1) == _lib.CBX_ERR_INVALID
        before = download(g, O.make_state(1031, 1, 2, 0.1, 0.0))
        g.lockAny()
        with pytest.raises(CbxError) as e:
            g.synchronise(0, -1, 0, False)  # polyakruppert.c:16 would divide by zero
        assert e.value.code == _lib.CBX_ERR_INVALID
        g.unlockAny()
        with pytest.raises(CbxError) as e:
            g.replica_optimise(0, task=0)  # optimisers/polyakruppert.cu is a stub
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
        g.wait()
        compare_states(download(g, before), before)  # the refused calls changed nothing
    finally:
        g.free()


def test_optimiser_step_then_elastic_averaging():
    # optimisers/synchronouseamsgd.cu is optimisers/sma.cu's call sequence: the
    # task step under type 3 + elastic is the SMA one, then the barrier reads w.
    from crossbow_amd import BUF_GRADIENT, BUF_LAST
    n, R, mom, wd = 4099, 3, 0.9, 1e-4
    st = O.make_state(n, 1, R, 0.1, mom)
    g = _make(EA, n, R, 0.1, mom, wd=wd)
    try:
        upload(g, st)
        want = st.clone()
        for i in range(R):
            gr = O.fill_normal(n, 600 + i, 0.01)
            last = O.fill_normal(n, 620 + i, 0.001)
            g.replica_write(i, BUF_GRADIENT, gr)
            g.replica_write(i, BUF_LAST, last)
            g.replica_optimise(i, task=i)
            O.sma_optimise(np.float32(-0.05), mom, wd, want.w[i], gr, last, want.s[i])
        _barrier(g, want, EA, 1)
        g.wait()
        compare_states(download(g, st), want)
    finally:
        g.free()


# ---- forced split, staged, timing ------------------------------------------------
@pytest.mark.parametrize("model", [EA, PR])
@pytest.mark.parametrize("bucket", [0, 122_880], ids=["1-bucket", "3-ragged-buckets"])
def test_forced_split_same_bits_as_fused(model, bucket):
    # 300_001 floats pad to 74 x 1024 float4s: buckets of 30 + 30 + 14.  With
    # the split forced at one device elastic averaging still reads w.
    fused = _run(model, 300_001, 3, 0.1, 0.9, clocks=(0, 1))
    split = _run(model, 300_001, 3, 0.1, 0.9, clocks=(0, 1), split=True, bucket=bucket)
    compare_states(split, fused)


@pytest.mark.parametrize("model", [EA, PR])
def test_staged_step_in_the_pinned_mirrors(model):
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_LAST
    n, R = 65_537, 3
    st = O.make_state(n, 1, R, 0.1, 0.9)
    g = _make(model, n, R, 0.1, 0.9)
    try:
        g.base_host_view(0, BUF_DATA)[:] = st.z[0]
        g.base_host_view(0, BUF_LAST)[:] = st.last[0]
        for i in range(R):
            g.replica_host_view(i, BUF_DIFF)[:] = st.s[i]
            g.replica_host_view(i, BUF_DATA)[:] = st.w[i]
        want = st.clone()
        _barrier(g, want, model, 2, staged=2)
        g.wait()
        assert_bitexact(g.base_host_view(0, BUF_DATA), want.z[0], "z (host)")
        assert_bitexact(g.base_host_view(0, BUF_LAST), want.last[0], "last (host)")
        for i in range(R):
            assert_bitexact(g.replica_host_view(i, BUF_DATA), want.w[i], f"w[{i}] (host)")
        compare_states(download(g, st), want)
    finally:
        g.free()


@pytest.mark.parametrize("model", [EA, PR])
def test_kernel_time_is_reported(model):
    from crossbow_amd._lib import T_KERNEL, T_STEP
    st = O.make_state(50_000, 1, 4, 0.1, 0.9)
    g = _make(model, 50_000, 4, 0.1, 0.9)
    try:
        g.set_timing(True)
        _one_step(g, st)
        t = g.last_timing(0)
        assert t[T_KERNEL] > 0 and t[T_STEP] > 0
        assert g.timing_history(T_KERNEL)[-1] > 0
    finally:
        g.free()


def test_sma_after_a_foreign_step_rejoins_its_pipeline():
    # Cross-step pipelined SMA (mode 1, forced split, 4 buckets) keeps state
    # from step to step; an elastic-averaging step in between must invalidate
    # it, or the next SMA step would overlap buffers the foreign step wrote.
    from crossbow_amd import UPDATE_SYNCHRONOUSEAMSGD
    n, R = 50_000, 3
    st = O.make_state(n, 1, R, 0.1, 0.9)
    g = _make(UPDATE_SYNCHRONOUSEAMSGD, n, R, 0.1, 0.9)
    try:
        g.set_force_split(True)
        g.set_pipeline_mode(1)
        g.set_bucket_elements(16_384)
        upload(g, st)
        want = st.clone()
        for clock, elastic in enumerate([False, False, True, False, False]):
            g.setElasticAverage(elastic)
            g.lockAny()
            g.synchronise(0, clock, 0, False)
            g.unlockAny()
            if elastic:
                AV.elastic_average(want)
            else:
                O.sma_step(want)
        g.wait()
        compare_states(download(g, st), want)
    finally:
        g.free()
