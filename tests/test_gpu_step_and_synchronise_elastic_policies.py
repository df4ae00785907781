"""GPU parity of ``cbx_step_and_synchronise_elastic_clipped_variables``: the
replicas' pending task steps, clipped by global L2 norm (or skipped over a
non-finite gradient), with a learning rate per variable, or both, fused into the
one-GPU elastic-averaging barrier (the three task_elastic_*_kernels.hip), under
update model 3 with ``setElasticAverage``.

Expectations come from the host, never from a device result: per stepping
replica ``tests.gradient_clip_common.decide`` and ``step(..., variables=,
mults=)`` (clipping on) or ``tests.test_optimise_plan.per_variable_step``
(rates only), both of which rest on ``O.sma_optimise``; then
``tests.averaging_common.elastic_average``.  The clipped gradients have an exact
S in any summation order (``C.exact_gradient``: scale exactly 0.5), so S, K, the
scale and the flags are known without the device and the records compare bit
for bit.  Every comparison is bit for bit over every buffer, a NaN only having
to be a NaN where the oracle has one in z and w; s, g and ``last`` compare as
bits, NaN payloads included.

The three policies are what is on: "variables" (rates only), "clipped"
(clipping only: the multipliers are there, the switch is off) and
"clipped_variables".
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import averaging_common as AV
from tests import gradient_clip_common as C
from tests.helpers import assert_bitexact, bits
from tests.test_gpu_step_and_synchronise import ALPHA, DISCARD, _busy, _exp, _hip, _inv, _snapshot
from tests.test_gpu_step_and_synchronise_clipped import ZERO, gradient
from tests.test_optimise_plan import per_variable_step

pytestmark = pytest.mark.gpu

EAMSGD = 3  # CBX_UPDATE_SYNCHRONOUSEAMSGD
POLICIES = ("variables", "clipped", "clipped_variables")
RAGGED = (1, 3, 35, 4093, 4096, 1000)  # boundaries inside a float4 and inside a 256-float chunk
RAGGED_M = (3.0, 0.75, 1.0, 1.7, 0.3, 2.5)  # no power of two but the 1
SNAN = 0x7FA00001  # a signalling NaN with a payload


def clips(policy):
    return policy in ("clipped", "clipped_variables")


def per_variable(policy):
    return policy in ("variables", "clipped_variables")


def layout(n):
    """Three variables whose boundaries lie inside float4s (and inside chunks), multipliers no power of two."""
    if n < 3:
        return (n,), (3.0,)
    a = n // 3
    return (a, a + 1, n - 2 * a - 1), (3.0, 0.75, 1.7)


def two_variables(n):
    """tests/test_gpu_step_and_synchronise.py's ``_two_variables`` as a layout: one operator, two variables."""
    return (n // 2, n - n // 2), (1.0, 2.0)


def _gpu(policy, R, momentum, wd, variables, mults, rate_policy=_exp, sync=0, c=None, skip=True, one_operator=False,
         update_type=EAMSGD, elastic=True, method=0):
    """A context of one device; one operator per variable unless ``one_operator``.  ``policy`` None: both off."""
    from crossbow_amd import TheGPU
    n = sum(variables)
    g = TheGPU()
    g.init([0])
    try:
        if one_operator:
            g.setModel(1, 4 * n)
            for v, count in enumerate(variables):
                g.setModelVariable(0, v + 1, [count], 4 * count)
                g.setModelVariableLearningRateMultiplier(0, v + 1, mults[v])
        else:
            g.setModel(len(variables), 4 * n)
            for v, count in enumerate(variables):
                g.setModelVariable(v, 1, [count], 4 * count)
                g.setModelVariableLearningRateMultiplier(v, 1, mults[v])
        g.setModelWorkPerClock(3)
        g.setUpdateModelType(update_type)
        if elastic:
            g.setElasticAverage(True)
        g.setEamsgdAlpha(ALPHA)
        g.setMomentum(momentum, method)
        g.setWeightDecay(wd)
        rate_policy(g)
        g.setModelManager(R, sync)
        g.set_variable_learning_rates(policy is not None and per_variable(policy))
        if policy is not None and clips(policy):
            g.set_gradient_clip(c if c is not None else C.exact_gradient(n)[2], skip)
    except Exception:
        g.free()
        raise
    return g


def _rates(rate_policy, R, tasks, momentum):
    """Each stepping replica's rate, read from a twin context's own configuration."""
    twin = _gpu(None, R, momentum, 0.0, (4,), (1.0,), rate_policy, update_type=7, elastic=False)
    try:
        return [twin.replica_learning_rate(i, tasks[i]) if tasks[i] >= 0 else 0.0 for i in range(R)]
    finally:
        twin.free()


class PolicyCase:
    """The device's buffers mirrored on the host: the oracle's state plus the replicas' gradients and momenta."""

    def __init__(self, policy, R, momentum, variables, mults, seed=0):
        self.policy, self.R, self.momentum, self.variables, self.mults = policy, R, momentum, variables, mults
        self.n = n = sum(variables)
        self.st = O.make_state(n, 1, R, ALPHA, momentum)
        self.g = [O.fill_normal(n, 5000 + seed + i, 0.01) for i in range(R)]
        self.last = [O.fill_normal(n, 5100 + seed + i, 0.001) if momentum > 0 else None for i in range(R)]
        self.decision = {}

    def set_gradients(self, kinds):
        """Exact gradients by outcome ("join" takes an unclipped one that nobody reads)."""
        self.g = [gradient(self.n, k if k != "join" else "unclipped", i) for i, k in enumerate(kinds)]

    def upload(self, gpu):
        from crossbow_amd import BUF_GRADIENT, BUF_LAST
        from tests.helpers import upload
        upload(gpu, self.st)
        for i in range(self.R):
            gpu.replica_write(i, BUF_GRADIENT, self.g[i])
            if self.last[i] is not None:
                gpu.replica_write(i, BUF_LAST, self.last[i])

    def step(self, tasks, rates, wd, c=None, skip=True, keep=True, sums=None):
        """The two-call sequence.  sums[i] = (S, K) where the host's exact pair is not to be used."""
        st, pv = self.st, self.policy is not None and per_variable(self.policy)
        c = c if c is not None else C.exact_gradient(self.n)[2]
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if tasks[i] >= 0 and not keep}
        self.decision = {}
        with np.errstate(all="ignore"):
            for i in range(self.R):
                if tasks[i] < 0:
                    continue
                bufs = [st.w[i], self.g[i], self.last[i], st.s[i]]
                if self.policy is not None and clips(self.policy):
                    S, K = sums[i] if sums else C.exact_sum_sq(self.g[i])
                    scale, flags = C.decide(S, K, c, skip)
                    self.decision[i] = (S, K, float(scale), flags)
                    C.step(bufs, scale, flags, self.momentum, wd, lr=rates[i], variables=self.variables if pv else None,
                           mults=self.mults if pv else None)
                elif pv:
                    per_variable_step(rates[i], self.mults, self.momentum, wd, *bufs, variables=self.variables)
                else:
                    O.sma_optimise(np.float32(-rates[i]), self.momentum, wd, *bufs)
            AV.elastic_average(st)  # z and w of the locked replicas from st.first on; last and copy untouched
        self.dev_s = [kept[i][0] if i in kept else st.s[i] for i in range(self.R)]
        self.dev_g = [kept[i][1] if i in kept else self.g[i] for i in range(self.R)]

    def check(self, gpu, what=""):
        from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
        st, same = self.st, C.assert_same_with_nans
        same(gpu.base_read(0, BUF_DATA), st.z[0], f"{what} z")
        if st.last is not None:
            assert_bitexact(gpu.base_read(0, BUF_LAST), st.last[0], f"{what} base last")  # left alone
        for i in range(self.R):
            same(gpu.replica_read(i, BUF_DATA), st.w[i], f"{what} w[{i}]")
            for kind, want, name in ((BUF_DIFF, self.dev_s[i], "s"), (BUF_GRADIENT, self.dev_g[i], "g"),
                                     (BUF_LAST, self.last[i], "last")):
                if want is None:
                    continue
                got = gpu.replica_read(i, kind)
                skipped = i in self.decision and self.decision[i][3] & C.SKIPPED
                if skipped or not np.isnan(want).any():  # a skipped replica's buffers keep every bit, NaN payloads too
                    assert np.array_equal(bits(got), bits(want)), f"{what} {name}[{i}] differs in its bits"
                else:
                    same(got, want, f"{what} {name}[{i}]")
        for a in (st.z[0], *st.w):
            assert np.count_nonzero(np.isnan(a)) * 4 <= a.size  # at most a quarter of a compared array is NaN

    def check_records(self, gpu, counts, what=""):
        """counts[i] = (steps, clipped_steps, skipped_steps) expected so far."""
        for i in range(self.R):
            rec = gpu.replica_clip_stats(i)
            assert (rec["steps"], rec["clipped_steps"], rec["skipped_steps"]) == tuple(counts[i]), (what, i, rec)
            if i in self.decision:
                S, K, scale, flags = self.decision[i]
                assert (rec["sum_sq"], rec["nonfinite"], rec["scale"], rec["flags"]) == (S, K, scale, flags), (what, i, rec)


def _count(counts, case):
    for i, (_, _, _, flags) in case.decision.items():
        counts[i][0] += 1
        counts[i][1] += 1 if flags & C.CLIPPED else 0
        counts[i][2] += 1 if flags & C.SKIPPED else 0


def _fused(gpu, first, clock, tasks, streams=None, flags=0):
    gpu.lockAny()
    gpu.step_and_synchronise_elastic_clipped_variables(first, clock, 0, tasks, streams, flags)
    gpu.unlockAny()


def _sequence(gpu, first, clock, tasks):
    for i, t in enumerate(tasks):
        if t >= 0:
            gpu.replica_optimise(i, t)
    gpu.lockAny()
    gpu.synchronise(first, clock, 0, False)
    gpu.unlockAny()


def _kinds(policy, R):
    """All stepping: unclipped, clipped and skipped in turn under a clipped policy."""
    return [("unclipped", "clipped", "skipped")[i % 3] for i in range(R)] if clips(policy) else ["dense"] * R


def _run(policy, variables, mults, R, momentum, wd, flags, rate_policy=_exp, config=None, load_policy=None,
         one_operator=False, gpu=None, clock=1, counts=None):
    tasks = [3 + 2 * i for i in range(R)]  # a task number, hence a rate, per replica
    rates = _rates(rate_policy, R, tasks, momentum)
    assert R == 1 or len(set(rates)) == R, rates
    case = PolicyCase(policy, R, momentum, variables, mults)
    if clips(policy):
        case.set_gradients(_kinds(policy, R))
    own = gpu is None
    gpu = gpu or _gpu(policy, R, momentum, wd, variables, mults, rate_policy, one_operator=one_operator)
    try:
        if load_policy is not None:
            gpu.set_kernel_config(64, 0, load_policy, 2)  # the load/store policy is shared by every kernel
        if config:
            gpu.set_task_barrier_kernel_config(*config)
        case.upload(gpu)
        _fused(gpu, 0, clock, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        what = f"{policy} {config} policy {load_policy} flags {flags}:"
        case.check(gpu, what)
        if clips(policy):
            counts = counts if counts is not None else [[0, 0, 0] for _ in range(R)]
            _count(counts, case)
            case.check_records(gpu, counts, what)
        assert [gpu.replica_clock(i) for i in range(R)] == [clock] * R
    finally:
        if own:
            gpu.free()


# ---- the policies at the shapes --------------------------------------------------------------
# n: one element; one float past a pad quantum; 2 * 4,096 + 903 (a partial norm tile); a ragged size of
# several waves.  R: the largest unrolled count (8) and the first that needs a second chunk (9).  With and
# without momentum and weight decay; at mu = 0, wd = 0 only the clipped policies write g.
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("n,R,momentum,wd,rate_policy", [
    (1, 1, 0.0, 0.0, _exp),
    (4_097, 2, 0.9, 5e-4, _inv),
    (9_095, 3, 0.0, 1e-4, _exp),
    (70_001, 8, 0.9, 0.0, _exp),
    (70_001, 9, 0.0, 0.0, _inv),
    (4_097, 9, 0.9, 5e-4, _exp),
])
@pytest.mark.parametrize("policy", POLICIES)
def test_every_buffer_bitexact(policy, n, R, momentum, wd, rate_policy, flags):
    _run(policy, *layout(n), R, momentum, wd, flags, rate_policy)


def test_the_device_steps_each_variable_at_its_own_rate():
    # the device's w, held to the expectation with every multiplier forced to 1, differs in exactly the
    # variables whose multiplier is not 1: the matrix above is no test of the plain step alone
    from crossbow_amd import BUF_DATA
    R, momentum, wd, tasks = 2, 0.0, 0.0, [3, 5]
    rates = _rates(_exp, R, tasks, momentum)
    case = PolicyCase("variables", R, momentum, RAGGED, RAGGED_M)
    ones = PolicyCase("variables", R, momentum, RAGGED, (1.0,) * len(RAGGED))
    gpu = _gpu("variables", R, momentum, wd, RAGGED, RAGGED_M)
    try:
        case.upload(gpu)
        _fused(gpu, 0, 1, tasks)
        gpu.wait()
        case.step(tasks, rates, wd)
        case.check(gpu)
        ones.step(tasks, rates, wd)
        for i in range(R):
            got, lo = gpu.replica_read(i, BUF_DATA), 0
            for v, count in enumerate(RAGGED):
                same = np.array_equal(bits(got[lo:lo + count]), bits(ones.st.w[i][lo:lo + count]))
                assert same == (RAGGED_M[v] == 1.0), (i, v)
                lo += count
    finally:
        gpu.free()


# ---- variable lists: boundaries inside a 256-float chunk and inside a float4 ------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("which", ["two_variables_of_one_operator", "ragged"])
@pytest.mark.parametrize("policy", ["variables", "clipped_variables"])
def test_variable_lists(policy, which, flags):
    if which == "ragged":
        assert sum(RAGGED[:3]) % 4 != 0 and sum(RAGGED[:4]) % 256 != 0
        for momentum, wd in ((0.0, 0.0), (0.9, 1e-4)):
            _run(policy, RAGGED, RAGGED_M, 3, momentum, wd, flags)
    else:
        variables, mults = two_variables(4_099)
        assert variables[0] % 4 != 0
        _run(policy, variables, mults, 3, 0.9, 5e-4, flags, one_operator=True)


# ---- one call of every outcome ---------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("bad", ["nan", "inf", "minus_inf"])
@pytest.mark.parametrize("policy", ["clipped", "clipped_variables"])
def test_unclipped_clipped_skipped_and_joining_in_one_call(policy, bad, flags):
    # Replica 2 is skipped over one non-finite float.  Its g and last also hold signalling NaNs with
    # payloads, and so does its w: s = w must be a bit copy, g and last must keep every bit, and w' = w_i
    # goes into the barrier as it is (one NaN in z, far below a quarter).
    from crossbow_amd import BUF_DATA
    R, momentum, wd = 4, 0.9, 1e-4
    variables, mults = layout(9_095)
    n = sum(variables)
    kinds, tasks = ["unclipped", "clipped", "clipped", "join"], [3, 5, 7, -1]
    rates = _rates(_exp, R, tasks, momentum)
    case = PolicyCase(policy, R, momentum, variables, mults)
    case.set_gradients(kinds)
    snan = np.array([SNAN], np.uint32).view(np.float32)[0]
    case.g[2][17] = {"nan": np.nan, "inf": np.inf, "minus_inf": -np.inf}[bad]
    bits(case.g[2])[5_000] = SNAN
    bits(case.last[2])[123] = SNAN + 1
    bits(case.st.w[2])[4_100] = SNAN + 2
    assert np.isnan(snan) and bits(case.g[2])[5_000] == SNAN
    gpu = _gpu(policy, R, momentum, wd, variables, mults)
    try:
        case.upload(gpu)
        w2 = case.st.w[2].copy()
        g2, last2 = case.g[2].copy(), case.last[2].copy()
        _fused(gpu, 0, 1, tasks, None, flags)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        assert [case.decision[i][2:] for i in (0, 1)] == [(1.0, 0), (0.5, C.CLIPPED)]
        assert case.decision[2][3] == C.CLIPPED | C.SKIPPED and 3 not in case.decision
        case.check(gpu)
        case.check_records(gpu, [[1, 0, 0], [1, 1, 0], [1, 1, 1], [0, 0, 0]])
        assert gpu.replica_clip_stats(3) == ZERO  # the joining replica's record was not touched
        snap = _snapshot(gpu, R, momentum)[0]
        assert np.array_equal(bits(snap["g[2]"]), bits(g2)), "g of the skipped replica"
        assert np.array_equal(bits(snap["last[2]"]), bits(last2)), "last of the skipped replica"
        if flags == 0:
            assert np.array_equal(bits(snap["s[2]"]), bits(w2)), "s = w of the skipped replica is a bit copy"
        assert np.count_nonzero(np.isnan(gpu.base_read(0, BUF_DATA))) == 1
    finally:
        gpu.free()


# ---- participation ------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("first,tasks,hold", [
    (0, [5, -1, 7], None), (1, [-1, 5, 7], None), (1, [-1, -1, 4], None),
    (0, [5, -1, 7], 1),  # SSP: a task thread holds replica 1, the barrier goes on without it
])
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_participation(policy, first, tasks, hold, flags):
    R, momentum, wd = 3, 0.9, 5e-4
    variables, mults = layout(9_095)
    rates = _rates(_inv, R, tasks, momentum)
    case = PolicyCase(policy, R, momentum, variables, mults)
    if clips(policy):
        case.set_gradients(["clipped", "skipped", "unclipped"])
    case.st.first = first
    gpu = _gpu(policy, R, momentum, wd, variables, mults, _inv, sync=0 if hold is None else 1)
    try:
        case.upload(gpu)
        if hold is not None:
            gpu.replica_lock(hold)
            case.st.locked[hold] = 0
        _fused(gpu, first, 2, tasks, None, flags)
        if hold is not None:
            gpu.replica_unlock(hold)
        gpu.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        if clips(policy):
            counts = [[0, 0, 0] for _ in range(R)]
            _count(counts, case)
            case.check_records(gpu, counts)
            for i in range(R):
                if tasks[i] < 0:
                    assert gpu.replica_clip_stats(i) == ZERO, i
    finally:
        gpu.free()


# ---- launch shapes ------------------------------------------------------------------------------
# one and two float4s per lane, 64 and 256 threads, with and without a cap, both load policies: one context
# per (policy, load policy), the shapes and the flags on it one after the other from freshly uploaded buffers
@pytest.mark.parametrize("load_policy", [0, 1])
@pytest.mark.parametrize("policy", POLICIES)
def test_forced_launch_shapes_bitexact(policy, load_policy):
    R, momentum, wd = 3, 0.9, 5e-4
    variables, mults = layout(70_001)
    gpu = _gpu(policy, R, momentum, wd, variables, mults)
    try:
        clock, counts = 0, [[0, 0, 0] for _ in range(R)]
        for config in [(64, 1, 0), (64, 2, 2), (256, 1, 4), (256, 2, 0)]:
            for flags in (0, DISCARD):
                clock += 1
                _run(policy, variables, mults, R, momentum, wd, flags, config=config, load_policy=load_policy, gpu=gpu,
                     clock=clock, counts=counts)
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("policy", POLICIES)
def test_grid_stride_shape_bitexact(policy, flags):
    # The default configuration on a launch too small to fill the chip 16 waves per CU over
    # (small_launch_shape): 800,001 floats are 3,136 waves on at most 2,048 blocks, so some blocks take a
    # second trip, and the chunk-table lookup with them.
    _run(policy, *layout(800_001), 2, 0.9, 5e-4, flags)


# ---- caller streams --------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("policy", POLICIES)
def test_gradients_and_norms_on_caller_streams(policy, flags):
    # Each replica's gradient arrives on a task stream, behind ~2 ms of other work; the norm passes go on
    # those streams and the launch behind them.  Until then g holds another gradient.
    import torch
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    variables, mults = layout(70_001)
    n = sum(variables)
    tasks = [2, 4, 6]
    rates = _rates(_exp, R, tasks, momentum)
    gpu = _gpu(policy, R, momentum, wd, variables, mults)
    hip = _hip()
    try:
        case = PolicyCase(policy, R, momentum, variables, mults)
        if clips(policy):
            case.set_gradients(["clipped", "skipped", "unclipped"])
        fresh = [torch.from_numpy(g).cuda() for g in case.g]
        case.upload(gpu)
        stale = np.full(n, 3.0, np.float32)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, stale)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for st in streams:
            _busy(torch, st)
        for i in range(R):
            assert hip.hipMemcpyAsync(gpu.replica_buffer(i, BUF_GRADIENT), fresh[i].data_ptr(), 4 * n, 3,
                                      streams[i % 2].cuda_stream) == 0  # device to device
        _fused(gpu, 0, 1, tasks, [streams[i % 2].cuda_stream for i in range(R)], flags)
        gpu.wait()
        torch.cuda.synchronize()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        if clips(policy):
            case.check_records(gpu, [[1, 1, 0], [1, 1, 1], [1, 0, 0]])
    finally:
        torch.cuda.synchronize()
        gpu.free()


# ---- a clock loop, and the records against the sequence's --------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("policy", POLICIES)
def test_clock_loop_alternates_with_the_two_call_sequence(policy, flags):
    # 5 clocks on one context, gradients rewritten each clock: the odd clocks through the fused call, the
    # even ones through cbx_replica_optimise and cbx_synchronise.  A twin context runs the sequence on every
    # clock: buffers, records (all 48 bytes), copy flags and clocks are the same after each.
    from crossbow_amd import BUF_GRADIENT
    R, clocks, momentum, wd = 3, 5, 0.9, 1e-4
    variables, mults = layout(9_095)
    rate_twin = _gpu(None, R, momentum, 0.0, (4,), (1.0,), update_type=7, elastic=False)
    case = PolicyCase(policy, R, momentum, variables, mults)
    gpu, twin = (_gpu(policy, R, momentum, wd, variables, mults) for _ in range(2))
    try:
        case.upload(gpu)
        case.upload(twin)
        task, counts = 0, [[0, 0, 0] for _ in range(R)]
        for clock in range(1, clocks + 1):
            kinds = [("clipped", "unclipped", "skipped")[(i + clock) % 3] for i in range(R)]
            if clips(policy):
                case.set_gradients(kinds)
            else:
                case.g = [O.fill_normal(case.n, 6000 + task + i, 0.01) for i in range(R)]
            tasks = list(range(task, task + R))
            task += R
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            rates = [rate_twin.replica_learning_rate(i, tasks[i]) for i in range(R)]
            fused = clock % 2 == 1
            if fused:
                _fused(gpu, 0, clock, tasks, None, flags)
            else:
                _sequence(gpu, 0, clock, tasks)
            _sequence(twin, 0, clock, tasks)
            case.step(tasks, rates, wd, keep=not fused or flags == 0)
            gpu.wait()
            twin.wait()
            what = f"clock {clock} ({'fused' if fused else 'two calls'}):"
            case.check(gpu, what)
            if clips(policy):
                _count(counts, case)
                case.check_records(gpu, counts, what)
                assert [gpu.replica_clip_stats(i) for i in range(R)] == [twin.replica_clip_stats(i) for i in range(R)], what
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                if flags == 0 or not (fused and key[0] in "sg"):  # under the discard flag s and g stay as they were
                    assert np.array_equal(bits(a[0][key]), bits(b[0][key])), f"{what} {key} against the sequence"
            assert a[1:] == b[1:], what
            if flags != 0 and fused:  # the twin's kept outputs are what the next clocks start from on both
                from crossbow_amd import BUF_DIFF
                for i in range(R):
                    twin.replica_write(i, BUF_DIFF, a[0][f"s[{i}]"])
        assert [gpu.replica_clock(i) for i in range(R)] == [clocks] * R
    finally:
        gpu.free()
        twin.free()
        rate_twin.free()


# ---- MULTISTEP: the copy flag stays raised ------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("policy", POLICIES)
def test_a_raised_copy_flag_stays_raised(policy, flags):
    # Replica 1 crosses the boundary at the task that is passed, (task + 1) >= 3, and the query raises its
    # copy flag.  This barrier has no Phase D: the flag stays raised, as after the two calls on the twin.
    from crossbow_amd import BUF_DATA

    def multistep(g):
        g.setLearningRateDecayPolicyMultiStep(0.1, 0.5, 0, [3])
    R, momentum, wd = 3, 0.9, 5e-4
    variables, mults = layout(9_095)
    tasks = [0, 2, 1]
    case = PolicyCase(policy, R, momentum, variables, mults)
    if clips(policy):
        case.set_gradients(["clipped", "unclipped", "skipped"])
    gpu, twin = (_gpu(policy, R, momentum, wd, variables, mults, multistep) for _ in range(2))
    try:
        case.upload(gpu)
        case.upload(twin)
        rates = _rates(multistep, R, tasks, momentum)
        assert rates == pytest.approx([0.1, 0.05, 0.1])
        _sequence(twin, 0, 7, tasks)
        assert [gpu.replica_copy(i) for i in range(R)] == [0, 0, 0]
        _fused(gpu, 0, 7, tasks, None, flags)
        gpu.wait()
        twin.wait()
        case.step(tasks, rates, wd, keep=flags == 0)
        case.check(gpu)
        z = gpu.base_read(0, BUF_DATA)
        for i in range(R):
            assert not np.array_equal(bits(gpu.replica_read(i, BUF_DATA)), bits(z)), f"w[{i}] is z"
        assert [gpu.replica_copy(i) for i in range(R)] == [twin.replica_copy(i) for i in range(R)] == [0, 1, 0]
        assert [gpu.replica_clock(i) for i in range(R)] == [twin.replica_clock(i) for i in range(R)] == [7] * R
        if clips(policy):
            assert [gpu.replica_clip_stats(i) for i in range(R)] == [twin.replica_clip_stats(i) for i in range(R)]
    finally:
        gpu.free()
        twin.free()


# ---- the feature combinations -------------------------------------------------------------------------
def _on_then_off(gpu):
    gpu.set_gradient_clip(1.0, True)  # the scratch exists, its records all zeros
    gpu.set_gradient_clip(0.0, False)
    return gpu


@pytest.mark.parametrize("flags", [0, DISCARD])
def test_with_both_off_it_is_the_plain_elastic_call(flags):
    # the same kernel, the same bits: a twin through cbx_step_and_synchronise_elastic, and the oracle
    R, momentum, wd = 3, 0.9, 5e-4
    variables, mults = layout(9_095)
    tasks = [3, 5, 7]
    rates = _rates(_exp, R, tasks, momentum)
    for make in (lambda: _gpu(None, R, momentum, wd, variables, mults),
                 lambda: _on_then_off(_gpu(None, R, momentum, wd, variables, mults)),
                 lambda: _gpu("variables", R, momentum, wd, variables, (1.0,) * 3)):  # the switch on, no irregular one
        gpu, twin = make(), make()
        try:
            for g in (gpu, twin):
                g.set_timing(True)
            case = PolicyCase(None, R, momentum, variables, mults)
            case.upload(gpu)
            case.upload(twin)
            _fused(gpu, 0, 1, tasks, None, flags)
            twin.lockAny()
            twin.step_and_synchronise_elastic(0, 1, 0, tasks, None, flags)
            twin.unlockAny()
            gpu.wait()
            twin.wait()
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                assert np.array_equal(bits(a[0][key]), bits(b[0][key])), f"{key} against cbx_step_and_synchronise_elastic"
            assert a[1:] == b[1:]
            assert len(gpu.timing_history()) == len(twin.timing_history()) == 1
            case.step(tasks, rates, wd, keep=flags == 0)
            case.check(gpu)
        finally:
            gpu.free()
            twin.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("policy", ["clipped", "clipped_variables"])
def test_clipping_on_and_nobody_stepping_touches_no_record(policy, flags):
    # nothing to clip: no norm pass, the per-variable or the plain kernel; the barrier alone, as cbx_synchronise
    R, momentum, wd = 3, 0.9, 1e-4
    variables, mults = layout(9_095)
    case = PolicyCase(policy, R, momentum, variables, mults)
    gpu = _gpu(policy, R, momentum, wd, variables, mults)
    try:
        gpu.set_timing(True)
        case.upload(gpu)
        _fused(gpu, 0, 1, [-1] * R, None, flags)
        gpu.wait()
        case.step([-1] * R, [0.0] * R, wd)
        case.check(gpu)
        assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
        assert len(gpu.timing_history()) == 1
    finally:
        gpu.free()


@pytest.mark.parametrize("flags", [0, DISCARD])
@pytest.mark.parametrize("row", ["multipliers_all_1", "switch_off", "clipping_off"])
def test_with_one_feature_off_it_is_the_policy_of_the_other(row, flags):
    # Each degenerate setting against a twin that is set up plainly for the policy it should fall to, over two
    # clocks: the same bits in every buffer, the same records, one timing entry per call; and the oracle's.
    from crossbow_amd import BUF_GRADIENT
    R, momentum, wd = 3, 0.9, 1e-4
    variables, mults = layout(9_095)
    ones = (1.0,) * len(variables)
    if row == "multipliers_all_1":  # clipping on, the switch on, no irregular multiplier: the clipped kernel
        policy = "clipped"
        make = lambda: _gpu("clipped_variables", R, momentum, wd, variables, ones)  # noqa: E731
    elif row == "switch_off":  # clipping on, irregular multipliers, the switch off: the clipped kernel
        policy = "clipped"
        make = lambda: _gpu("clipped", R, momentum, wd, variables, mults)  # noqa: E731
    else:  # clipping switched on and off again (the scratch exists), the rates on: the per-variable kernel
        policy = "variables"
        make = lambda: _on_then_off(_gpu("variables", R, momentum, wd, variables, mults))  # noqa: E731
    twin_mults = mults if policy == "variables" else ones
    gpu, twin = make(), _gpu(policy, R, momentum, wd, variables, twin_mults)
    try:
        for g in (gpu, twin):
            g.set_timing(True)
        case = PolicyCase(policy, R, momentum, variables, twin_mults)
        case.upload(gpu)
        case.upload(twin)
        counts = [[0, 0, 0] for _ in range(R)]
        for k in range(2):
            if clips(policy):
                case.set_gradients(["unclipped", "clipped", "skipped"])
            else:
                case.g = [O.fill_normal(case.n, 6100 + 3 * k + i, 0.01) for i in range(R)]
            for g in (gpu, twin):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, case.g[i])
            tasks = [3 * k, 3 * k + 1, 3 * k + 2]
            rates = _rates(_exp, R, tasks, momentum)
            _fused(gpu, 0, k + 1, tasks, None, flags)
            _fused(twin, 0, k + 1, tasks, None, flags)
            gpu.wait()
            twin.wait()
            a, b = _snapshot(gpu, R, momentum), _snapshot(twin, R, momentum)
            for key in a[0]:
                assert np.array_equal(bits(a[0][key]), bits(b[0][key])), f"{row} clock {k + 1}: {key} against the twin"
            assert a[1:] == b[1:]
            assert len(gpu.timing_history()) == len(twin.timing_history()) == k + 1
            if flags == 0:  # under the discard flag s and g keep what the clock found: the mirror follows the kept form
                case.step(tasks, rates, wd)
                case.check(gpu, f"{row} clock {k + 1}:")
            if clips(policy):
                assert [gpu.replica_clip_stats(i) for i in range(R)] == [twin.replica_clip_stats(i) for i in range(R)]
                if flags == 0:
                    _count(counts, case)
                    case.check_records(gpu, counts)
            else:
                assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R  # no norm ran, no record touched
    finally:
        gpu.free()
        twin.free()


def test_dense_sums_hold_the_reordering_bound_before_the_scale_is_used():
    # Normal-data gradients under both clipped policies: the device's S must lie within the reordering bound
    # of the exact one before its scale is used; then every buffer is the oracle's from that S.
    R, momentum, wd = 3, 0.9, 1e-4
    variables, mults = layout(9_095)
    n = sum(variables)
    tasks = [3, 5, 7]
    rates = _rates(_exp, R, tasks, momentum)
    for policy in ("clipped", "clipped_variables"):
        case = PolicyCase(policy, R, momentum, variables, mults)
        exact = [C.exact_sum_sq(g) for g in case.g]
        c = float(np.float32(0.5 * np.sqrt(exact[1][0])))  # some replicas clip, by no power of two
        gpu = _gpu(policy, R, momentum, wd, variables, mults, c=c)
        try:
            case.upload(gpu)
            _fused(gpu, 0, 1, tasks)
            gpu.wait()
            sums = []
            for i in range(R):
                rec = gpu.replica_clip_stats(i)
                S, K = exact[i]
                # n terms summed in some order in fp64: |S_dev - S| <= (n - 1) * 2^-53 * S to first order
                print(f"{policy} replica {i}: S {rec['sum_sq']!r} exact {S!r} bound {n * 2.0 ** -53 * S!r}")
                assert abs(rec["sum_sq"] - S) <= n * 2.0 ** -53 * S and rec["nonfinite"] == K == 0
                sums.append((rec["sum_sq"], K))
            case.step(tasks, rates, wd, c=c, sums=sums)
            assert any(case.decision[i][3] & C.CLIPPED for i in range(R))
            case.check(gpu)
        finally:
            gpu.free()


# ---- refusals ---------------------------------------------------------------------------------------------
REFUSALS = {
    # name: (error code name, keyword arguments of the context, set-up after the manager, call arguments)
    "force_split": ("CBX_ERR_UNSUPPORTED", {}, lambda g: g.set_force_split(True), {}),
    "nesterov": ("CBX_ERR_UNSUPPORTED", {"method": 1}, None, {}),
    "worker": ("CBX_ERR_UNSUPPORTED", {"update_type": 1, "elastic": False}, None, {}),
    "polyak_ruppert": ("CBX_ERR_UNSUPPORTED", {"update_type": 6, "elastic": False}, None, {}),
    "sma": ("CBX_ERR_UNSUPPORTED", {"update_type": 7, "elastic": False}, None, {}),
    "eamsgd_without_elastic_average": ("CBX_ERR_UNSUPPORTED", {"update_type": 3, "elastic": False}, None, {}),
    "below_first": ("CBX_ERR_INVALID", {}, None, {"first": 1, "tasks": [3, 4, 5]}),
    "unlocked": ("CBX_ERR_INVALID", {"sync": 1, "hold": 2}, None, {}),
    "task_minus_2": ("CBX_ERR_INVALID", {}, None, {"tasks": [3, -2, 5]}),
    "null_tasks": ("CBX_ERR_INVALID", {}, None, {"tasks": None}),
    "flag_bit_2": ("CBX_ERR_INVALID", {}, None, {"flags": 2}),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_change_nothing(name):
    # cbx_step_and_synchronise_elastic's table without the two rows this call honours, with both features on:
    # no buffer, flag or clock changes, no norm pass runs and no record's counter is bumped
    from crossbow_amd import CbxError, _lib
    code, kw, after, call = REFUSALS[name]
    R, momentum, wd = 3, 0.9, 5e-4
    variables, mults = two_variables(4_099)
    update_type, elastic = kw.get("update_type", EAMSGD), kw.get("elastic", True)
    gpu = _gpu("clipped_variables", R, momentum, wd, variables, mults, sync=kw.get("sync", 0), c=1.0, update_type=update_type, elastic=elastic, method=kw.get("method", 0))
    try:
        if after:
            after(gpu)
        case = PolicyCase("clipped_variables", R, momentum, variables, mults)
        case.upload(gpu)
        if update_type == EAMSGD and not kw.get("method"):
            gpu.replica_optimise(1, 0)  # a record that is not all zeros: one clipped step behind replica 1
            gpu.wait()
            assert gpu.replica_clip_stats(1)["steps"] == 1
        gpu.set_replica_copy(0, True)  # a flag the refused call must leave raised
        before = _snapshot(gpu, R, momentum)
        records = [gpu.replica_clip_stats(i) for i in range(R)]
        hold = kw.get("hold")
        if hold is not None:
            gpu.replica_lock(hold)
        gpu.lockAny()
        first, tasks, flags = call.get("first", 0), call.get("tasks", [3, 4, 5]), call.get("flags", 0)
        if tasks is None:
            rc = gpu._L.cbx_step_and_synchronise_elastic_clipped_variables(gpu._ctx, first, 1, 0, None, None, flags)
            assert rc == getattr(_lib, code), _lib.last_error()
        else:
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_elastic_clipped_variables(first, 1, 0, tasks, None, flags)
            assert e.value.code == getattr(_lib, code), str(e.value)
        assert "cbx_step_and_synchronise_elastic_clipped_variables" in _lib.last_error(), _lib.last_error()
        gpu.wait()
        after_call = _snapshot(gpu, R, momentum)
        for key in before[0]:
            assert_bitexact(after_call[0][key], before[0][key], f"{key} after the refused call")
        assert after_call[1:] == before[1:], "copy flags and clocks after the refused call"
        assert [gpu.replica_clip_stats(i) for i in range(R)] == records, "no counter was bumped"
        gpu.unlockAny()
        if hold is not None:
            gpu.replica_unlock(hold)
    finally:
        gpu.free()


def test_variables_that_do_not_tile_the_model_are_refused():
    # a variable whose capacity is more than its shape's bytes: the variables do not tile the model's
    # elements, so with the switch on and an irregular multiplier nothing says where a rate applies
    from crossbow_amd import CbxError, TheGPU, _lib
    n, R = 4_099, 3
    gpu = TheGPU()
    gpu.init([0])
    try:
        gpu.setModel(1, 4 * n)
        gpu.setModelVariable(0, 1, [n - 16], 4 * n)
        gpu.setModelVariableLearningRateMultiplier(0, 1, 2.0)
        gpu.setUpdateModelType(EAMSGD)
        gpu.setElasticAverage(True)
        gpu.setEamsgdAlpha(ALPHA)
        gpu.setMomentum(0.9, 0)
        _exp(gpu)
        try:
            gpu.setModelManager(R, 0)
            gpu.set_variable_learning_rates(True)
            gpu.set_gradient_clip(1.0, True)
        except CbxError:
            pytest.fail("the set-up itself was refused: " + _lib.last_error())
        before = _snapshot(gpu, R, 0.9)
        gpu.lockAny()
        with pytest.raises(CbxError) as e:
            gpu.step_and_synchronise_elastic_clipped_variables(0, 1, 0, [3, 4, 5], None, 0)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        assert "cbx_step_and_synchronise_elastic_clipped_variables with variable learning rates" in _lib.last_error()
        gpu.unlockAny()
        gpu.wait()
        after = _snapshot(gpu, R, 0.9)
        for key in before[0]:
            assert_bitexact(after[0][key], before[0][key], f"{key} after the refused call")
        assert after[1:] == before[1:]
        assert [gpu.replica_clip_stats(i) for i in range(R)] == [ZERO] * R
    finally:
        gpu.free()


def test_the_plain_elastic_call_still_refuses_both_features():
    from crossbow_amd import CbxError, _lib
    variables, mults = layout(9_095)
    gpu = _gpu("clipped_variables", 3, 0.9, 1e-4, variables, mults)  # both on
    try:
        for setup in (lambda: None, lambda: gpu.set_gradient_clip(0.0, False),  # both; then variable rates alone
                      lambda: (gpu.set_gradient_clip(1.0, False), gpu.set_variable_learning_rates(False))):  # clipping alone
            setup()
            gpu.lockAny()
            with pytest.raises(CbxError) as e:
                gpu.step_and_synchronise_elastic(0, 1, 0, [3, 4, 5], None, 0)
            assert e.value.code == _lib.CBX_ERR_UNSUPPORTED
            assert "cbx_step_and_synchronise_elastic_clipped_variables" in _lib.last_error()  # the call to take
            gpu.unlockAny()
        assert [gpu.replica_clip_stats(i) for i in range(3)] == [ZERO] * 3
    finally:
        gpu.free()
