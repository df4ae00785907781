"""GPU parity of ``cbx_replica_accumulate_clipped`` and ``cbx_step_and_synchronise_ssgd_clipped``
(task_ssgd_clipped_kernels.hip).  No device result enters an expectation: per stepping replica in
ascending id ``exact_sum_sq`` and ``decide``; a skipped replica does nothing, otherwise
``g = float32(scale) * g`` and ``O.ssgd_worker``; then ``O.ssgd_sync``.  The gradients have an exact S
in any order, so every buffer and record field compares bit for bit.  n = 9,095: three norm tiles, a
ragged tail, padded to 12,288."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact
from tests.test_gpu_step_and_synchronise import DISCARD, _exp, _gpu, _snapshot
from tests.test_gpu_step_and_synchronise_clipped import MAX_NORM, ZERO, _mixes, gradient
from tests.test_gpu_step_and_synchronise_ssgd import SsgdCase, _rates, _sgpu
from tests.test_gpu_step_and_synchronise_variables import SHAPES

pytestmark = pytest.mark.gpu

N = 9_095
BOTH = pytest.mark.parametrize("flags", [0, DISCARD])


class ClipSsgdCase(SsgdCase):
    def set_gradients(self, kinds):
        self.g = [gradient(self.n, k if k != "join" else "unclipped", i) for i, k in enumerate(kinds)]
        self.decision = {}

    def worker_clipped(self, i, rate, wd, c):
        """One clipped task step of replica i (cbx_replica_accumulate_clipped)."""
        S, K = C.exact_sum_sq(self.g[i])
        scale, flags = C.decide(S, K, c, True)
        self.decision[i] = (S, K, float(scale), flags)
        if not flags & C.SKIPPED:  # skipped: nothing, not g, not the accumulator
            self.g[i] = np.float32(scale) * self.g[i]
            self.worker(i, rate, wd)

    def step(self, tasks, rates, wd, c, keep=True):
        kept = {i: self.g[i].copy() for i in range(self.R) if tasks[i] >= 0 and not keep}
        self.decision = {}
        for i in range(self.R):  # ascending id: the accumulator depends on the order
            if tasks[i] >= 0:
                self.worker_clipped(i, rates[i], wd, c)
        O.ssgd_sync(self.st, [self.acc], self.wpc)
        for i, g in kept.items():  # the device left them alone: so does the mirror, for the clocks to come
            self.g[i] = g
        self.dev_s, self.dev_g = self.st.s, self.g

    def check_all(self, gpu, counts, what=""):
        """Every buffer, then every record; counts[i] = [steps, clipped_steps, skipped_steps] before this step."""
        self.check(gpu, what)
        for i, (_, _, _, flags) in self.decision.items():
            counts[i] = [counts[i][0] + 1, counts[i][1] + bool(flags & C.CLIPPED), counts[i][2] + bool(flags & C.SKIPPED)]
        for i in range(self.R):
            rec = gpu.replica_clip_stats(i)
            assert [rec["steps"], rec["clipped_steps"], rec["skipped_steps"]] == counts[i], (what, i, rec)
            if i in self.decision:
                assert (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"]) == self.decision[i], (what, i, rec)


def _call(gpu, clock, tasks, flags=0, streams=None, fused=True):
    if not fused:  # the two-call sequence
        for i, t in enumerate(tasks):
            if t >= 0:
                gpu.replica_accumulate_clipped(i, t, streams[i] if streams else None)
    gpu.lockAny()
    if fused:
        gpu.step_and_synchronise_ssgd_clipped(0, clock, 0, tasks, streams, flags)
    else:
        gpu.synchronise(0, clock, 0, False)
    gpu.unlockAny()
    gpu.wait()


def _tasks(all_tasks, kinds):
    return [t if k != "join" else -1 for t, k in zip(all_tasks, kinds)]


def _mix_run(n, R, momentum, wd, mixes, shapes):
    """One context; the launch shapes, the flags and the outcome mixes run on it one after the other, each from
    fresh buffers."""
    all_tasks, c = [3 + 2 * i for i in range(R)], C.exact_gradient(n)[2]
    rates = _rates(_exp, R, all_tasks, momentum)
    gpu = _sgpu(n, R, momentum, wd)
    try:
        gpu.set_gradient_clip(c, True)
        clock, counts = 0, [[0, 0, 0] for _ in range(R)]
        for shape, flags, kinds in [(s, f, k) for s in shapes for f in (0, DISCARD) for k in mixes]:
            gpu.set_task_barrier_kernel_config(*shape)
            tasks = _tasks(all_tasks, kinds)
            case = ClipSsgdCase(n, R, momentum)
            case.set_gradients(kinds)
            case.upload(gpu)
            clock += 1
            _call(gpu, clock, tasks, flags)
            case.step(tasks, rates, wd, c, keep=flags == 0)
            # the host's decisions are the outcomes the mix names
            assert [bool(case.decision[i][3] & C.SKIPPED) for i, k in enumerate(kinds) if k != "join"] == \
                [k == "skipped" for k in kinds if k != "join"]
            case.check_all(gpu, counts, f"shape {shape} flags {flags} {kinds}:")
            assert [gpu.replica_clock(i) for i in range(R)] == [clock] * R
        if all(k == "join" for kinds in mixes for k in kinds):
            assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R  # no norm was launched
    finally:
        gpu.free()


# R: unrolled forms, the largest of them, and the first chunked one, whose second chunk holds a skipped replica.
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("R", [1, 3, 8, 9])
def test_outcome_mix(R, momentum, wd):
    assert C.exact_gradient(N)[2] == MAX_NORM
    _mix_run(N, R, momentum, wd, _mixes(R), SHAPES)


# One norm tile, one pad quantum; all skipped (z moves by the base momentum alone) and all joining.
@pytest.mark.parametrize("kinds", [["unclipped", "clipped", "skipped"], ["join", "skipped", "clipped"],
                                   ["skipped"] * 3, ["join"] * 3])
@pytest.mark.parametrize("n", [8, 1])
def test_one_tile(n, kinds):
    _mix_run(n, 3, 0.9, 1e-4, [kinds], SHAPES[:1])


# The case that catches an fma(rate, 0, acc) or a load that was not skipped.
@BOTH
@pytest.mark.parametrize("R,skipped", [(3, 1), (9, 8)])
def test_base_gradient_that_is_not_zero_on_entry_and_a_skipped_nonfinite_gradient(R, skipped, flags):
    from crossbow_amd import BUF_DATA, BUF_GRADIENT
    momentum, wd = 0.9, 1e-4
    kinds = ["skipped" if i == skipped else ("clipped", "unclipped")[i % 2] for i in range(R)]
    tasks = [3 + 2 * i for i in range(R)]
    rates = _rates(_exp, R, tasks, momentum)
    case = ClipSsgdCase(N, R, momentum)
    case.set_gradients(kinds)
    gpu = _sgpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        case.upload(gpu)
        # an earlier task of the same clock through the clipped task step, then a fresh exact gradient
        gpu.replica_accumulate_clipped(0, 1)
        case.worker_clipped(0, _rates(_exp, R, [1] + [-1] * (R - 1), momentum)[0], wd, MAX_NORM)
        gpu.wait()
        assert case.acc.any()
        assert_bitexact(gpu.base_read(0, BUF_GRADIENT), case.acc, "base gradient before the fused call")
        case.g[0] = gradient(N, kinds[0], 0)
        gpu.replica_write(0, BUF_GRADIENT, case.g[0])
        before = _snapshot(gpu, R, momentum)[0]
        _call(gpu, 1, tasks, flags)
        case.step(tasks, rates, wd, MAX_NORM, keep=flags == 0)
        assert case.decision[skipped][1::2] == (3, C.CLIPPED | C.SKIPPED)  # K and the flags
        case.check_all(gpu, [[i == 0, i == 0, 0] for i in range(R)])
        reads = [gpu.base_read(0, BUF_DATA), gpu.base_read(0, BUF_GRADIENT)] + [gpu.replica_read(i, BUF_DATA) for i in range(R)]
        assert not any(np.isnan(a).any() for a in reads)
        after = _snapshot(gpu, R, momentum)[0]
        for name in (f"g[{skipped}]", f"last[{skipped}]"):  # every bit, the NaN's and the infinities' included
            assert_bitexact(after[name], before[name], name)
    finally:
        gpu.free()


# 5 clocks, gradients rewritten each clock: odd clocks fused, even ones the two-call sequence; the norm
# passes on the sync stream, or each on a task stream of its replica's.
@BOTH
@pytest.mark.parametrize("own_streams", [False, True])
def test_clock_loop_alternates_with_the_two_call_sequence(own_streams, flags):
    import torch

    from crossbow_amd import BUF_GRADIENT
    R, clocks, momentum, wd = 4, 5, 0.9, 1e-4
    twin = _gpu(4, R, momentum, 0.0, _exp)
    case = ClipSsgdCase(N, R, momentum)
    gpu = _sgpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        case.upload(gpu)
        counts = [[0, 0, 0] for _ in range(R)]
        held = [torch.cuda.Stream() for _ in range(R)] if own_streams else None
        streams = [s.cuda_stream for s in held] if own_streams else None
        for clock in range(1, clocks + 1):
            kinds = [("clipped", "skipped", "unclipped", "join", "clipped")[(i + clock) % 5] for i in range(R)]
            case.set_gradients(kinds)
            for i in range(R):
                gpu.replica_write(i, BUF_GRADIENT, case.g[i])
            tasks = _tasks([R * clock + i for i in range(R)], kinds)
            rates = [twin.replica_learning_rate(i, t) if t >= 0 else 0.0 for i, t in enumerate(tasks)]
            fused = clock % 2 == 1
            _call(gpu, clock, tasks, flags, streams, fused)
            case.step(tasks, rates, wd, MAX_NORM, keep=not fused or flags == 0)
            case.check_all(gpu, counts, f"clock {clock} ({'fused' if fused else 'two calls'}) {kinds}:")
        assert [gpu.replica_clock(i) for i in range(R)] == [clocks] * R
        assert sum(c[2] for c in counts) >= 3
    finally:
        torch.cuda.synchronize()
        gpu.free()
        twin.free()


@BOTH
@pytest.mark.parametrize("fused", [True, False])
def test_with_clipping_off_both_calls_are_the_plain_ones(fused, flags):
    R, momentum, wd = 3, 0.9, 1e-4
    tasks = [3, -1, 7]
    rates = _rates(_exp, R, tasks, momentum)
    case = SsgdCase(N, R, momentum)  # normal data, the plain oracle
    gpu = _sgpu(N, R, momentum, wd)
    try:
        gpu.set_gradient_clip(1.0, True)
        gpu.set_gradient_clip(0.0, False)  # on, then off again
        case.upload(gpu)
        _call(gpu, 1, tasks, flags, None, fused)
        case.step(tasks, rates, wd, keep=not fused or flags == 0)
        case.check(gpu)
        assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
    finally:
        gpu.free()


# (error code, keyword arguments of the context, flags of the fused call, which of the two calls)
@pytest.mark.parametrize("code,kw,flags,call", [
    ("CBX_ERR_UNSUPPORTED", {"update_type": 7}, 0, "fused"), ("CBX_ERR_UNSUPPORTED", {"update_type": 7}, 0, "step"),
    ("CBX_ERR_UNSUPPORTED", {"method": 1}, 0, "fused"), ("CBX_ERR_UNSUPPORTED", {"method": 1}, 0, "step"),
    ("CBX_ERR_INVALID", {}, 2, "fused"), ("CBX_ERR_STATE", {"wpc": 0}, 0, "fused")])
def test_refusals_change_nothing(code, kw, flags, call):
    from crossbow_amd import BUF_GRADIENT, CbxError, _lib
    n, R, momentum, wd = 4_099, 3, 0.9, 1e-4
    wpc = kw.get("wpc", R)
    gpu = _gpu(n, R, momentum, wd, update_type=kw.get("update_type", 1), method=kw.get("method", 0),
               before_manager=(lambda g: g.setModelWorkPerClock(wpc)) if wpc else None)
    try:
        gpu.set_gradient_clip(MAX_NORM, True)
        case = ClipSsgdCase(n, R, momentum)
        case.set_gradients(["clipped", "skipped", "unclipped"])
        case.upload(gpu)
        acc = O.fill_normal(n, 5555, 0.01)
        gpu.base_write(0, BUF_GRADIENT, acc)
        gpu.set_replica_copy(0, True)
        before = _snapshot(gpu, R, momentum)
        gpu.lockAny()
        with pytest.raises(CbxError) as e:
            if call == "fused":
                gpu.step_and_synchronise_ssgd_clipped(0, 1, 0, [3, 4, 5], None, flags)
            else:
                gpu.replica_accumulate_clipped(1, 4)
        gpu.unlockAny()
        assert e.value.code == getattr(_lib, code), str(e.value)
        gpu.wait()
        after = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after[0][key], before[0][key], f"{key} after the refused call")
        assert after[1:] == before[1:], "copy flags and clocks after the refused call"
        assert_bitexact(gpu.base_read(0, BUF_GRADIENT), acc, "base gradient after the refused call")
        assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
    finally:
        gpu.free()
