"""The sma.c seam for the elastic-averaging and Polyak-Ruppert barriers:
cbx_ea_plan_step / cbx_pr_plan_step over buffers the CALLER owns
(include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip), on one GPU.

The caller's buffers hold exactly `elements` floats, so the averaging kernels
run their float4 bulk (whole 64-lane chunks, not whole kPadFloat4s) and a
scalar tail of up to 1,027 floats on extra workgroups of the same launch.
Every comparison is bit for bit against the CPU restatement
(tests/native/averaging_ref.c through tests/averaging_common.py, pinned by
tests/test_averaging_ref.py), over every element of z, last and every w; the
snapshots s must come back untouched.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests.helpers import assert_bitexact

pytestmark = pytest.mark.gpu

EA, PR = "elastic", "polyak"
ALPHA = 0.1


class _Buffers:
    """The caller's side: one unpadded device tensor per model buffer."""

    def __init__(self, st: O.SmaState):
        import torch
        dev = torch.device("cuda:0")
        self.z = torch.from_numpy(st.z[0].copy()).to(dev)
        self.last = torch.from_numpy(st.last[0].copy()).to(dev) if st.last is not None else None
        self.s = [torch.from_numpy(a.copy()).to(dev) for a in st.s]
        self.w = [torch.from_numpy(a.copy()).to(dev) for a in st.w]
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def check(self, want: O.SmaState, s0):
        self.stream.synchronize()
        assert_bitexact(self.z.cpu().numpy(), want.z[0], "z")
        if self.last is not None:
            assert_bitexact(self.last.cpu().numpy(), want.last[0], "last")
        for i in range(want.size):
            assert_bitexact(self.w[i].cpu().numpy(), want.w[i], f"w[{i}]")
            assert_bitexact(self.s[i].cpu().numpy(), s0[i], f"s[{i}] must be untouched")


def _seam_step(plan, buf: _Buffers, st: O.SmaState, model, clock, s_null=False):
    """One step through the seam with st's locked / copy / first, and the same
    step on st.  Returns (the seam's return value, the restatement's)."""
    R = st.size
    if model == PR:
        reps = [(0, buf.w[i].data_ptr(), int(st.locked[i]), int(st.copy[i])) for i in range(R)]
        got = plan.polyak_step([buf.stream.cuda_stream], [buf.z.data_ptr()],
                               [buf.last.data_ptr()] if buf.last is not None else None, reps, st.alpha, clock,
                               st.first)
        return got, AV.polyak_ruppert(st, clock)
    reps = [(0, buf.w[i].data_ptr(), None if s_null else buf.s[i].data_ptr(), int(st.locked[i])) for i in range(R)]
    got = plan.elastic_step([buf.stream.cuda_stream], [buf.z.data_ptr()], reps, st.alpha, st.first)
    AV.elastic_average(st)
    return got, None


def _run(model, n, R, alpha=ALPHA, mom=0.9, clocks=(3,), first=0, held=(), copy_at=None, s_null=False):
    """`clocks` steps on one plan; copy_at = {step index: replica ids whose copy
    flag is raised before it}.  Returns (buffers, expected state, counts)."""
    from crossbow_amd.seam import SmaPlan
    st = O.make_state(n, 1, R, alpha, mom)
    st.first = first
    s0 = [a.copy() for a in st.s]
    buf = _Buffers(st)
    counts = []
    with SmaPlan([0], n) as plan:
        for k, clock in enumerate(clocks):
            st.locked[:] = 1
            for i in held:
                st.locked[i] = 0
            for i in (copy_at or {}).get(k, ()):
                st.copy[i] = 1
            got, want = _seam_step(plan, buf, st, model, clock, s_null=s_null)
            if model == PR:
                assert got == want, (k, got, want)
            else:
                assert got is None
            counts.append(got)
        buf.check(st, s0)
    return buf, st, counts


# (name, n, R, extra): no bulk (n < 1,024: the launch is tail workgroups only),
# the largest such size, bulk only, one chunk plus a tail that is no multiple
# of 4, a kPadFloat4 plus a tail, a bulk of 1,280 float4s (whole chunks, not
# whole kPadFloat4s), the chunked replica walk (R > kChunk) tail included,
# `first` with an unlocked replica over a grid-stride bulk, nothing locked.
SHAPES = [
    ("one-element", 1, 1, {}),
    ("three-elements", 3, 2, {}),
    ("largest-tail-only", 1023, 3, {}),
    ("bulk-only", 1024, 2, {}),
    ("chunk-and-ragged-tail", 1027, 4, {}),
    ("ragged-4099", 4099, 4, {}),
    ("quarter-chunk-bulk", 4096 + 1024 + 7, 3, {}),
    ("chunked-9-replicas", 65_541, 9, {}),
    ("first-and-held", 300_007, 8, dict(first=2, held=(5,))),
    ("no-replica-locked", 4099, 2, dict(held=(0, 1))),
    ("three-steps", 4099, 4, dict(clocks=(0, 1, 2))),
]


@pytest.mark.parametrize("model", [EA, PR])
@pytest.mark.parametrize("name,n,R,extra", SHAPES, ids=[c[0] for c in SHAPES])
def test_seam_step_bitexact(model, name, n, R, extra):
    _run(model, n, R, **extra)


@pytest.mark.parametrize("n", [4099, 1027])
@pytest.mark.parametrize("mom", [0.0, 0.9], ids=["last-null", "last-given"])
def test_polyak_last_null_and_given(n, mom):
    # make_state has no `last` at momentum 0: the seam gets NULL (model.c:116-120)
    buf, st, _ = _run(PR, n, 3, mom=mom, clocks=(0, 1))
    assert (buf.last is None) == (mom == 0.0)
    if buf.last is not None:  # left holding L = D - z of the last step: what moved z
        assert np.any(buf.last.cpu().numpy() != O.make_state(n, 1, 3, ALPHA, mom).last[0])


@pytest.mark.parametrize("n", [4099, 1027])
def test_polyak_alpha_zero_leaves_the_replicas(n):
    buf, st, _ = _run(PR, n, 3, alpha=0.0, clocks=(2,))
    w0 = O.make_state(n, 1, 3, 0.0, 0.9).w
    for i in range(3):
        assert_bitexact(buf.w[i].cpu().numpy(), w0[i], f"w[{i}] with alpha 0")


@pytest.mark.parametrize("n", [4099, 1027])
def test_polyak_copy_into_a_locked_replica(n):
    buf, st, counts = _run(PR, n, 4, clocks=(1, 2), copy_at={1: (2,)})
    assert counts == [0, 1]
    z = buf.z.cpu().numpy()
    assert_bitexact(buf.w[2].cpu().numpy(), z, "the flagged replica, tail included")
    for i in (0, 1, 3):
        assert not np.array_equal(buf.w[i].cpu().numpy().view(np.uint32), z.view(np.uint32))


@pytest.mark.parametrize("n", [4099, 1027])
def test_polyak_copy_flags_of_replicas_outside_the_step(n):
    # replica 0 is below `first`, replica 2 is unlocked: untouched, not counted
    buf, st, counts = _run(PR, n, 4, clocks=(1,), first=1, held=(2,), copy_at={0: (0, 2)})
    assert counts == [0]
    w0 = O.make_state(n, 1, 4, ALPHA, 0.9).w
    for i in (0, 2):
        assert_bitexact(buf.w[i].cpu().numpy(), w0[i], f"w[{i}]")


@pytest.mark.parametrize("n", [4099, 1027, 3])
def test_elastic_one_rank_without_snapshots(n):
    _run(EA, n, 3, s_null=True, clocks=(0, 1))


@pytest.mark.parametrize("model", [EA, PR])
def test_seam_agrees_with_the_context(model):
    """The other door: the same inputs through cbx_synchronise (update model 3
    with cbx_set_elastic_average(1), and update model 6) end in the same bits."""
    from tests.helpers import download, upload
    from tests.test_gpu_averaging import _make
    n, R, clock = 4099, 3, 2
    buf, _, _ = _run(model, n, R, clocks=(clock,))
    st = O.make_state(n, 1, R, ALPHA, 0.9)
    g = _make(model, n, R, ALPHA, 0.9)
    try:
        upload(g, st)
        g.lockAny()
        g.synchronise(0, clock, 0, False)
        g.unlockAny()
        g.wait()
        ctx = download(g, st)
    finally:
        g.free()
    assert_bitexact(buf.z.cpu().numpy(), ctx.z[0], "z")
    if model == PR:
        assert_bitexact(buf.last.cpu().numpy(), ctx.last[0], "last")
    for i in range(R):
        assert_bitexact(buf.w[i].cpu().numpy(), ctx.w[i], f"w[{i}]")


def test_sma_elastic_sma_on_one_plan():
    """The steps share the plan's scratch and the caller's stream order."""
    from crossbow_amd.seam import SmaPlan
    n, R, mom = 4099, 3, 0.9
    st = O.make_state(n, 1, R, ALPHA, mom)
    s0 = [a.copy() for a in st.s]
    buf = _Buffers(st)
    with SmaPlan([0], n) as plan:
        for kind in ("sma", EA, "sma", PR, "sma"):
            if kind == "sma":
                reps = [(0, buf.w[i].data_ptr(), buf.s[i].data_ptr(), 1, 0) for i in range(R)]
                plan.step([buf.stream.cuda_stream], [buf.z.data_ptr()], [buf.last.data_ptr()], reps, ALPHA, mom)
                O.sma_step(st)
            else:
                _seam_step(plan, buf, st, kind, 1)
            buf.check(st, s0)  # each step bit-exact, not only the last


def test_plan_timing_history_of_the_fused_launches():
    """cbx_sma_plan_set_timing: each step's launch stamps itself; same bits."""
    from crossbow_amd.seam import SmaPlan
    n, R = 4099, 3
    st = O.make_state(n, 1, R, ALPHA, 0.9)
    s0 = [a.copy() for a in st.s]
    buf = _Buffers(st)
    with SmaPlan([0], n) as plan:
        assert plan.timing_history(4) == []
        plan.set_timing(True)
        for clock, model in enumerate((EA, PR, EA)):
            _seam_step(plan, buf, st, model, clock)
        t = plan.timing_history(8)
        assert len(t) == 3 and all(0.0 < x < 100.0 for x in t), t
        assert len(plan.timing_history(2)) == 2
        plan.set_timing(False)
        _seam_step(plan, buf, st, EA, 3)
        assert plan.timing_history(8) == []
        buf.check(st, s0)


@pytest.mark.parametrize("model", [EA, PR])
def test_seam_refusals_write_nothing(model):
    import torch

    from crossbow_amd import CbxError
    from crossbow_amd._lib import CBX_ERR_INVALID, CBX_ERR_UNSUPPORTED
    from crossbow_amd.seam import SmaPlan
    n, R = 4099, 2
    st = O.make_state(n, 1, R, ALPHA, 0.9)
    s0 = [a.copy() for a in st.s]
    buf = _Buffers(st)
    streams, z, last = [buf.stream.cuda_stream], [buf.z.data_ptr()], [buf.last.data_ptr()]

    def step(plan, z=z, dev=0, count=R, clock=1):
        if model == PR:
            reps = [(dev, buf.w[i % R].data_ptr(), 1, 0) for i in range(count)]
            return plan.polyak_step(streams, z, last, reps, ALPHA, clock)
        reps = [(dev, buf.w[i % R].data_ptr(), buf.s[i % R].data_ptr(), 1) for i in range(count)]
        return plan.elastic_step(streams, z, reps, ALPHA)

    with SmaPlan([0], n) as plan:
        if model == PR:
            with pytest.raises(CbxError) as e:  # polyakruppert.c:16 would divide by zero
                step(plan, clock=-1)
            assert e.value.code == CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:
            step(plan, z=[0])
        assert e.value.code == CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:  # a device the plan does not have
            step(plan, dev=1)
        assert e.value.code == CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:
            step(plan, dev=-1)
        assert e.value.code == CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:  # kMaxReplicas = 64 locked replicas per device
            step(plan, count=65)
        assert e.value.code == CBX_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        buf.check(st, s0)  # the refused calls changed nothing
        step(plan)  # and the plan still works
        AV.step(st, model == PR, 1)
        buf.check(st, s0)
