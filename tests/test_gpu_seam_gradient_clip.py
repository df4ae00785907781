"""The sma.c seam of gradient clipping by global norm:
``cbx_sma_plan_optimise_clipped`` and ``cbx_sma_plan_clip_stats`` over buffers
the CALLER owns, of exactly ``elements`` floats, each followed here by a guard
of sentinel floats that must survive.  The oracle is
tests/gradient_clip_common.py.

Shapes: n = 1 (under one float4), 1,027 (four float4 chunks and a 3-float
tail) and 4,099 (one tile plus three floats: a second tile that is all tail).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact

pytestmark = pytest.mark.gpu

SHAPES = [1, 1027, 4099]
GUARD = 1024
sweep = pytest.mark.parametrize("n,momentum,wd", [(n, m, wd) for n in SHAPES for m in (0.0, 0.9) for wd in (0.0, 5e-4)])


class _Buffers:
    """w, g, last, s on the host and on the device; the device copies carry
    GUARD sentinel floats past the n the plan knows of."""

    def __init__(self, seed, n, momentum, g=None):
        import torch
        self.n = n
        self.host = C.host(seed, n, momentum)
        if g is not None:
            self.host[1] = g
        self.guard = O.fill_normal(GUARD, seed + 4, 3.0)
        self.dev = [torch.from_numpy(np.concatenate([a, self.guard])).to("cuda:0") if a is not None else None
                    for a in self.host]
        for t in self.dev:
            assert t is None or t.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() if t is not None else None for t in self.dev]

    def check(self, what="", nans=False):
        for name, t, a in zip(("w", "g", "last", "s"), self.dev, self.host):
            if a is None:
                continue
            got = t.cpu().numpy()
            (C.assert_same_with_nans if nans else assert_bitexact)(got[:self.n], a, what + name)
            assert_bitexact(got[self.n:], self.guard, what + name + " guard")


@sweep
def test_a_norm_that_never_clips_and_no_norm_at_all_are_the_plain_step(n, momentum, wd):
    import torch

    from crossbow_amd.seam import SmaPlan
    stream = torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        assert plan.clip_stats(0, 3, stream.cuda_stream)["steps"] == 0  # all zeros before the first step
        for slot, c in ((3, 1e30), (4, 0.0)):
            b = _Buffers(700 + slot, n, momentum)
            plan.optimise_clipped(0, slot, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, c)
            rec = plan.clip_stats(0, slot, stream.cuda_stream)
            O.sma_optimise(np.float32(-C.LR), momentum, wd, *b.host)
            b.check(f"max_norm {c}: ")
            assert (rec["flags"], rec["steps"], rec["clipped_steps"], rec["skipped_steps"], rec["scale"]) == \
                (0, 1, 0, 0, 1.0), rec
        assert plan.clip_stats(0, 5, stream.cuda_stream) == {k: 0 for k in rec}  # a slot never stepped


@sweep
def test_exact_case_with_no_device_value_in_the_expectation(n, momentum, wd):
    import torch

    from crossbow_amd.seam import SmaPlan
    g, S, c = C.exact_gradient(n)
    b = _Buffers(720, n, momentum, g=g)
    stream = torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        plan.optimise_clipped(0, 0, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, c)
        rec = plan.clip_stats(0, 0, stream.cuda_stream)
    scale, flags = C.decide(S, 0, c, False)
    assert (float(scale), flags) == (0.5, C.CLIPPED)
    C.step(b.host, scale, flags, momentum, wd)
    b.check()
    assert rec == {"sum_sq": S, "nonfinite": 0, "scale": 0.5, "flags": C.CLIPPED, "steps": 1, "clipped_steps": 1,
                   "skipped_steps": 0}, rec


@sweep
def test_normal_data_clips_to_the_norm(n, momentum, wd):
    import torch

    from crossbow_amd.seam import SmaPlan
    b = _Buffers(740, n, momentum)
    S_ref, K = C.exact_sum_sq(b.host[1])
    c = float(np.float32(0.25 * np.sqrt(S_ref)))
    stream = torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        plan.optimise_clipped(0, 63, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, c)
        rec = plan.clip_stats(0, 63, stream.cuda_stream)
    assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref, (rec["sum_sq"], S_ref)
    scale, flags = C.decide(rec["sum_sq"], K, c, False)
    assert flags == C.CLIPPED == rec["flags"] and rec["nonfinite"] == 0
    assert np.float32(rec["scale"]).view(np.uint32) == scale.view(np.uint32), (rec["scale"], scale)
    g_clipped = (scale * b.host[1]).astype(np.float64)
    assert abs(np.sqrt(np.sum(g_clipped * g_clipped)) - c) <= 1e-6 * c
    C.step(b.host, scale, flags, momentum, wd)
    b.check()


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("skip", [False, True])
def test_nonfinite_gradients(n, momentum, wd, skip):
    import torch

    from crossbow_amd.seam import SmaPlan
    b = _Buffers(760, n, momentum)
    pos = C.nonfinite_positions(n)
    for p, v in zip(pos, (np.nan, np.inf, -np.inf)):
        b.host[1][p] = v
    b.dev[1][:n] = torch.from_numpy(b.host[1]).to("cuda:0")
    torch.cuda.synchronize()
    S_ref, K = C.exact_sum_sq(b.host[1])
    stream = torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        plan.optimise_clipped(0, 1, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, 0.5, skip_nonfinite=skip)
        rec = plan.clip_stats(0, 1, stream.cuda_stream)
    assert rec["nonfinite"] == K == len(pos)
    assert abs(rec["sum_sq"] - S_ref) <= 2 * n * 2.0 ** -53 * S_ref
    scale, flags = C.decide(rec["sum_sq"], K, 0.5, skip)
    assert rec["flags"] == flags and bool(flags & C.SKIPPED) == skip
    assert (rec["steps"], rec["skipped_steps"]) == (1, 1 if skip else 0)
    C.step(b.host, scale, flags, momentum, wd)  # skipped: s = w and nothing else
    b.check(nans=True)
    if skip:  # g kept its bits, the NaN's payload too
        assert np.array_equal(b.dev[1].cpu().numpy()[:n].view(np.uint32), b.host[1].view(np.uint32))


@pytest.mark.parametrize("n,variables,mults", [(1027, (1, 3, 35, 988), (2.0, 1.0, 0.0, 0.5)),
                                               (4099, (1, 3, 35, 4060), (2.0, 1.0, 0.0, 0.5))])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("skip", [False, True])
def test_per_variable_step_with_clipping(n, variables, mults, momentum, wd, skip):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    b = _Buffers(780, n, momentum)
    if skip:
        b.host[1][n - 1] = np.inf
        b.dev[1][:n] = torch.from_numpy(b.host[1]).to("cuda:0")
        torch.cuda.synchronize()
    S_ref, K = C.exact_sum_sq(b.host[1])
    c = float(np.float32(0.5 * np.sqrt(S_ref)))
    stream = torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        with pytest.raises(CbxError) as e:  # no tables yet
            plan.optimise_clipped(0, 0, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, c, use_variables=True)
        assert e.value.code == _lib.CBX_ERR_STATE
        plan.set_variables(variables, mults)
        plan.optimise_clipped(0, 0, stream.cuda_stream, *b.ptrs(), C.LR, momentum, wd, c, skip_nonfinite=skip,
                              use_variables=True)
        rec = plan.clip_stats(0, 0, stream.cuda_stream)
    scale, flags = C.decide(rec["sum_sq"], K, c, skip)
    assert rec["flags"] == flags == (C.CLIPPED | (C.SKIPPED if skip else 0))
    C.step(b.host, scale, flags, momentum, wd, variables=variables, mults=mults)
    b.check(nans=True)


@pytest.mark.parametrize("n", [4097, 262149])
def test_seam_and_context_return_the_same_sum_bits(n):
    import torch

    from crossbow_amd import BUF_GRADIENT
    from crossbow_amd.seam import SmaPlan
    from tests.test_gpu_gradient_clip import _gpu
    b = _Buffers(800, n, 0.9)
    stream = torch.cuda.Stream()
    sums = []
    with SmaPlan([0], n) as plan:
        for slot in (0, 0, 7):  # a repeated call, and another slot
            b.dev[1][:n] = torch.from_numpy(b.host[1]).to("cuda:0")
            torch.cuda.synchronize()
            plan.optimise_clipped(0, slot, stream.cuda_stream, *b.ptrs(), C.LR, 0.9, 5e-4, 1e30)
            sums.append(plan.clip_stats(0, slot, stream.cuda_stream)["sum_sq"])
    gpu = _gpu(n, 0.9, 5e-4)
    try:
        gpu.set_gradient_clip(1e30, False)
        gpu.replica_write(0, BUF_GRADIENT, b.host[1])
        gpu.replica_optimise(0, task=0)
        sums.append(gpu.replica_clip_stats(0)["sum_sq"])
    finally:
        gpu.free()
    assert len({np.float64(s).view(np.uint64).item() for s in sums}) == 1, sums


def test_slots_are_independent_and_refusals():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n = 1027
    a, b = _Buffers(820, n, 0.9), _Buffers(830, n, 0.9)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with SmaPlan([0], n) as plan:
        w, g, last, s = a.ptrs()
        for args, code in (((0, 64, None, w, g, last, s, C.LR, 0.9, 0.0, 1.0), _lib.CBX_ERR_INVALID),
                           ((0, -1, None, w, g, last, s, C.LR, 0.9, 0.0, 1.0), _lib.CBX_ERR_INVALID),
                           ((1, 0, None, w, g, last, s, C.LR, 0.9, 0.0, 1.0), _lib.CBX_ERR_INVALID),
                           ((0, 0, None, w, g, last, s, C.LR, 0.9, 0.0, -1.0), _lib.CBX_ERR_INVALID),
                           ((0, 0, None, w, g, last, s, C.LR, 0.9, 0.0, float("nan")), _lib.CBX_ERR_INVALID),
                           ((0, 0, None, w, g, last, s, C.LR, 0.9, 0.0, float("inf")), _lib.CBX_ERR_INVALID),
                           ((0, 0, None, w, g, None, s, C.LR, 0.9, 0.0, 1.0), _lib.CBX_ERR_INVALID),
                           ((0, 0, None, w + 4, g, last, s, C.LR, 0.9, 0.0, 1.0), _lib.CBX_ERR_INVALID)):
            with pytest.raises(CbxError) as e:
                plan.optimise_clipped(*args)
            assert e.value.code == code, args
        rc = plan.lib.cbx_sma_plan_optimise_clipped(plan._p, 0, 0, None, w, g, last, s, C.LR, 0.9, 0.0, 1.0, 2, 0)
        assert rc == _lib.CBX_ERR_INVALID
        with pytest.raises(CbxError) as e:
            plan.clip_stats(0, 64, None)
        assert e.value.code == _lib.CBX_ERR_INVALID
        a.check("after the refusals: ")
        # two replicas in flight on two streams, a slot each
        plan.optimise_clipped(0, 10, s1.cuda_stream, *a.ptrs(), C.LR, 0.9, 5e-4, 0.01)
        plan.optimise_clipped(0, 11, s2.cuda_stream, *b.ptrs(), C.LR, 0.9, 5e-4, 1e30)
        ra, rb = plan.clip_stats(0, 10, s1.cuda_stream), plan.clip_stats(0, 11, s2.cuda_stream)
    for bufs, rec, c in ((a, ra, 0.01), (b, rb, 1e30)):
        scale, flags = C.decide(rec["sum_sq"], 0, c, False)
        assert rec["flags"] == flags and rec["steps"] == 1
        C.step(bufs.host, scale, flags, 0.9, 5e-4)
        bufs.check()
    assert ra["flags"] == C.CLIPPED and rb["flags"] == 0
