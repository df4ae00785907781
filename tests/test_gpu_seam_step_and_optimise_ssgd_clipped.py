"""The seam's cbx_ssgd_plan_accumulate_clipped and cbx_ssgd_plan_step_and_optimise_clipped over buffers
the CALLER owns (the TAIL instantiations of task_ssgd_clipped_kernels.hip).  Both roads, the fused call
and the clipped task step per stepping id followed by cbx_ssgd_plan_step, run against one host
expectation (``exact_sum_sq``, ``decide``, then nothing or ``g = float32(scale) * g`` and
``O.ssgd_worker``; then ``O.ssgd_sync``), bit for bit over every buffer and record; the guard floats
behind each buffer come back untouched, and the accumulator is not zero on entry."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.test_gpu_seam_step_and_optimise import DISCARD, _rates
from tests.test_gpu_seam_step_and_optimise_ssgd import CONFIGS, SsgdBuffers, SsgdData
from tests.test_gpu_step_and_synchronise_clipped import gradient

pytestmark = pytest.mark.gpu


def _mixes(R):
    """All stepping, the last skipped (at R = 9 the second chunk's); and replica 0 only joining (unrolled 8)."""
    every = [("clipped", "unclipped", "skipped")[i % 3] for i in range(R - 1)] + ["skipped"]
    return [every, ["join"] + every[1:]]


def _expect(d, kinds, rates, wd, c, keep):
    """The host's sequence in place on d; returns each stepping replica's (S, K, scale, flags)."""
    kept = {i: d.g[i].copy() for i, k in enumerate(kinds) if k != "join" and not keep}
    decision = {}
    for i, k in enumerate(kinds):  # ascending id: the accumulator depends on the order
        if k == "join":
            continue
        S, K = C.exact_sum_sq(d.g[i])
        scale, flags = C.decide(S, K, c, True)
        decision[i] = (S, K, float(scale), flags)
        if not flags & C.SKIPPED:
            d.g[i] = np.float32(scale) * d.g[i]
            O.ssgd_worker(np.float32(-rates[i]), wd, d.st.w[i], d.g[i], d.acc)
    O.ssgd_sync(d.st, [d.acc], d.wpc)
    for i, g in kept.items():
        d.g[i] = g
    return decision


def _setup(n, R, config, kinds):
    bmom, wd = CONFIGS[config]
    d = SsgdData(n, R, bmom, acc_seed=7777)
    d.g = [gradient(n, k if k != "join" else "unclipped", i) for i, k in enumerate(kinds)]
    return d, SsgdBuffers(d), wd, C.exact_gradient(n)[2]


# elements: the tail alone; one float past a float4 bulk; a ragged bulk of several waves.
@pytest.mark.parametrize("how", ["fused", "fused-discard", "sequence"])
@pytest.mark.parametrize("config", ["mom-wd", "plain"])
@pytest.mark.parametrize("R", [2, 9])
@pytest.mark.parametrize("n", [1, 4_097, 70_001])
def test_both_roads_bitexact(n, R, config, how):
    from crossbow_amd.seam import SmaPlan
    rates = _rates(R)
    slots = [40 - 3 * i for i in range(R)]
    for kinds in _mixes(R):
        d, buf, wd, c = _setup(n, R, config, kinds)
        steps = [k != "join" for k in kinds]
        stream = buf.stream.cuda_stream
        with SmaPlan([0], n) as plan:
            if how == "sequence":
                for i in range(R):
                    if steps[i]:
                        plan.ssgd_accumulate_clipped(0, slots[i], stream, buf.w[i].ptr, buf.g[i].ptr, buf.acc.ptr,
                                                     rates[i], wd, c, True)
                plan.ssgd_step([stream], [buf.z.ptr], [buf.blast.ptr] if buf.blast is not None else None,
                               [buf.acc.ptr], [(0, buf.w[i].ptr, 1) for i in range(R)], d.st.momentum, d.wpc)
            else:
                plan.ssgd_step_and_optimise_clipped(
                    [stream], [buf.z.ptr], [buf.blast.ptr] if buf.blast is not None else None, [buf.acc.ptr],
                    buf.replicas(steps, rates, g_null=[i for i in range(R) if not steps[i]]), d.st.momentum, wd,
                    d.wpc, 0, DISCARD if how == "fused-discard" else 0,
                    [s if st else -1 for s, st in zip(slots, steps)], c, True)
            decision = _expect(d, kinds, rates, wd, c, keep=how != "fused-discard")
            buf.check(f"{how} {kinds}:")
            assert not np.isnan(d.st.z[0]).any() and C.SKIPPED & decision[R - 1][3]
            for i, want in decision.items():
                rec = plan.clip_stats(0, slots[i], stream)
                got = (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"])
                assert got == want and rec["steps"] == 1, (kinds, i, rec)
                assert rec["skipped_steps"] == (kinds[i] == "skipped") == bool(want[3] & C.SKIPPED), (kinds, i, rec)


def test_two_stepping_replicas_sharing_a_slot_is_refused_before_any_launch():
    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n, R = 4_097, 3
    kinds = ["clipped", "join", "skipped"]
    d, buf, wd, c = _setup(n, R, "mom-wd", kinds)
    steps = [k != "join" for k in kinds]
    with SmaPlan([0], n) as plan:
        with pytest.raises(CbxError) as e:
            plan.ssgd_step_and_optimise_clipped([buf.stream.cuda_stream], [buf.z.ptr], [buf.blast.ptr], [buf.acc.ptr],
                                                buf.replicas(steps, _rates(R)), d.st.momentum, wd, d.wpc, 0, 0,
                                                [5, 5, 5], c, True)
        assert e.value.code == _lib.CBX_ERR_INVALID and "slot 5" in str(e.value)
        assert plan.clip_stats(0, 5, buf.stream.cuda_stream)["steps"] == 0
    buf.stream.synchronize()
    buf.acc.check(d.acc, "acc")
