"""The sma.c seam for the fused task steps: cbx_sma_plan_step_and_optimise over
buffers the CALLER owns (include/crossbow_sma.h, crossbow_amd/csrc/sma_seam.hip,
the TAIL instantiations of task_barrier_kernels.hip), on one GPU.

Expected values come from the oracle only: ``O.sma_optimise`` for every
stepping replica in id order, then ``O.sma_step``.  Every comparison is bit
for bit over z, the base ``last``, and ``w``, ``last``, ``s`` and ``g`` of
every replica.  Each device buffer is the first n floats of a larger
allocation whose other GUARD floats hold a sentinel pattern that must come
back untouched: a bulk or tail store past ``elements`` would break it.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import multidev_common as C
from tests.helpers import GUARD, Guarded, assert_bitexact  # noqa: F401 (Guarded: other test files take it from here)

pytestmark = pytest.mark.gpu

ALPHA = 0.1
DISCARD = 1  # CBX_STEP_DISCARD_TASK_OUTPUTS
# (replica momentum, weight decay, base momentum); the last has base and replica momentum that differ
CONFIGS = {"mom-wd": (0.9, 5e-4, 0.9), "plain": (0.0, 0.0, 0.0), "base-mom-only": (0.0, 5e-4, 0.9)}


def _rates(R):
    """A distinct learning rate per replica, exact in fp32."""
    return [float(np.float32(0.05 / (1.0 + 0.37 * i))) for i in range(R)]


class Data:
    """The caller's buffers mirrored on the host: the oracle's state plus the
    replicas' gradients and momenta (the fills of test_gpu_step_and_synchronise)."""

    def __init__(self, n, R, rmom, bmom, seed=0):
        self.n, self.R, self.rmom = n, R, rmom
        self.st = O.make_state(n, 1, R, ALPHA, bmom)
        self.g = [O.fill_normal(n, 5000 + seed + i, 0.01) for i in range(R)]
        self.last = [O.fill_normal(n, 5100 + seed + i, 0.001) if rmom > 0 else None for i in range(R)]

    def step(self, steps, rates, wd, keep=True):
        """The oracle's two-call sequence with st's locked / copy / first.  Without
        `keep` the device leaves s and g of the stepping replicas alone."""
        st = self.st
        kept = {i: (st.s[i].copy(), self.g[i].copy()) for i in range(self.R) if steps[i] and not keep}
        for i in range(self.R):
            if steps[i]:
                O.sma_optimise(np.float32(-rates[i]), self.rmom, wd, st.w[i], self.g[i], self.last[i], st.s[i])
        copies = O.sma_step(st)
        for i, (s, g) in kept.items():
            st.s[i], self.g[i] = s, g
        return 1 if copies > 0 else 0


class Buffers:
    def __init__(self, d: Data):
        import torch
        st = d.st
        self.d = d
        self.z = Guarded(st.z[0], 1)
        self.blast = Guarded(st.last[0], 2) if st.last is not None else None
        self.w = [Guarded(a, 10 + i) for i, a in enumerate(st.w)]
        self.s = [Guarded(a, 110 + i) for i, a in enumerate(st.s)]
        self.g = [Guarded(a, 210 + i) for i, a in enumerate(d.g)]
        self.last = [Guarded(a, 310 + i) if a is not None else None for i, a in enumerate(d.last)]
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def replicas(self, steps, rates, s_null=(), g_null=(), rlast_null=()):
        st = self.d.st
        return [(0, self.w[i].ptr, None if i in s_null else self.s[i].ptr, None if i in g_null else self.g[i].ptr,
                 None if self.last[i] is None or i in rlast_null else self.last[i].ptr, int(st.locked[i]),
                 int(st.copy[i]), int(bool(steps[i])), rates[i]) for i in range(self.d.R)]

    def call(self, plan, steps, rates, wd, flags=0, **nulls):
        st = self.d.st
        return plan.step_and_optimise([self.stream.cuda_stream], [self.z.ptr],
                                      [self.blast.ptr] if self.blast is not None else None,
                                      self.replicas(steps, rates, **nulls), ALPHA, st.momentum, self.d.rmom, wd,
                                      st.first, flags)

    def check(self, what=""):
        self.stream.synchronize()
        d, st = self.d, self.d.st
        self.z.check(st.z[0], f"{what} z")
        if self.blast is not None:
            self.blast.check(st.last[0], f"{what} base last")
        for i in range(d.R):
            self.w[i].check(st.w[i], f"{what} w[{i}]")
            self.s[i].check(st.s[i], f"{what} s[{i}]")
            self.g[i].check(d.g[i], f"{what} g[{i}]")
            if self.last[i] is not None:
                self.last[i].check(d.last[i], f"{what} last[{i}]")


def _run(n, R, config, flags, steps=None, first=0, held=(), copies=(), s_null=()):
    from crossbow_amd.seam import SmaPlan
    rmom, wd, bmom = CONFIGS[config]
    d = Data(n, R, rmom, bmom)
    d.st.first = first
    for i in held:
        d.st.locked[i] = 0
    for i in copies:
        d.st.copy[i] = 1
    steps = [i >= first and i not in held for i in range(R)] if steps is None else steps
    rates = _rates(R)
    buf = Buffers(d)
    with SmaPlan([0], n) as plan:
        got = buf.call(plan, steps, rates, wd, flags, s_null=s_null)
        want = d.step(steps, rates, wd, keep=flags == 0)
        buf.check()
    assert got == want, (got, want)
    return buf, got


# (id, n, R, configurations, extra): the SHAPES of test_gpu_seam_averaging.  Every
# shape meets two configurations, 1,027 and 65,541 all three.
SHAPES = [
    ("one-element", 1, 1, ("mom-wd", "plain"), {}),
    ("three-elements", 3, 2, ("plain", "base-mom-only"), {}),
    ("largest-tail-only", 1023, 3, ("base-mom-only", "mom-wd"), {}),
    ("bulk-only", 1024, 2, ("mom-wd", "plain"), {}),
    ("chunk-and-ragged-tail", 1027, 4, ("mom-wd", "plain", "base-mom-only"), {}),
    ("ragged-4099", 4099, 4, ("plain", "base-mom-only"), {}),
    ("quarter-chunk-bulk", 4096 + 1024 + 7, 3, ("base-mom-only", "mom-wd"), {}),
    ("chunked-9-replicas", 65_541, 9, ("mom-wd", "plain", "base-mom-only"), {}),
    ("first-and-held", 300_007, 8, ("mom-wd", "plain"), dict(first=2, held=(5,))),
]
CASES = [(f"{name}-{config}", n, R, config, extra) for name, n, R, configs, extra in SHAPES for config in configs]


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("name,n,R,config,extra", CASES, ids=[c[0] for c in CASES])
def test_every_buffer_bitexact(name, n, R, config, extra, flags):
    _run(n, R, config, flags, **extra)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("n", [1027, 65_541])
def test_mixed_mask(n, config, flags):
    _run(n, 9, config, flags, steps=[i in (0, 3, 8) for i in range(9)])


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [1027, 65_541])
def test_nobody_steps_is_the_plain_step(n, flags):
    """With an empty mask the call is cbx_sma_plan_step: the same bits as that
    call on a second set of buffers, and g and the replicas' last untouched."""
    from crossbow_amd.seam import SmaPlan
    R = 9
    buf, _ = _run(n, R, "mom-wd", flags, steps=[False] * R)
    d = Data(n, R, 0.9, 0.9)
    plain = Buffers(d)
    with SmaPlan([0], n) as plan:
        reps = [(0, plain.w[i].ptr, plain.s[i].ptr, 1, 0) for i in range(R)]
        plan.step([plain.stream.cuda_stream], [plain.z.ptr], [plain.blast.ptr], reps, ALPHA, 0.9)
        plain.stream.synchronize()
    for a, b, name in [(buf.z, plain.z, "z"), (buf.blast, plain.blast, "base last")] + \
            [(buf.w[i], plain.w[i], f"w[{i}]") for i in range(R)]:
        assert_bitexact(a.t.cpu().numpy(), b.t.cpu().numpy(), name)


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
@pytest.mark.parametrize("n", [1027, 4099])
def test_phase_d(n, flags):
    # a copy flag on a stepping replica (1) and on one that only joins (2)
    R, steps = 4, [True, True, False, True]
    buf, got = _run(n, R, "mom-wd", flags, steps=steps, copies=(1, 2))
    assert got == 1
    z = buf.z.t.cpu().numpy()[:n]
    for i in range(R):
        assert_bitexact(buf.w[i].t.cpu().numpy()[:n], z, f"w[{i}] == the new z, tail included")
    # last_i (and s_i, g_i when kept) are still the step's values: _run compared them with the oracle's,
    # which differ from what the buffers held before
    fresh = Data(n, R, 0.9, 0.9)
    for i in (0, 1, 3):
        assert np.any(buf.last[i].t.cpu().numpy()[:n] != fresh.last[i])
        assert np.any(buf.s[i].t.cpu().numpy()[:n] != fresh.st.s[i]) == (flags == 0)
    _, got = _run(n, R, "mom-wd", flags, steps=steps)
    assert got == 0


@pytest.mark.parametrize("n", [1027, 4099 + 1024])
def test_discard_keeps_s_and_g_and_accepts_a_null_s(n):
    R, steps = 4, [True, False, True, True]
    buf, _ = _run(n, R, "mom-wd", DISCARD, steps=steps, s_null=(0, 3))
    fresh = Data(n, R, 0.9, 0.9)
    for i in range(R):  # stepping or joining: every bit of s and g as it was, the last n mod 1,024 floats too
        assert_bitexact(buf.s[i].t.cpu().numpy()[:n], fresh.st.s[i], f"s[{i}]")
        assert_bitexact(buf.g[i].t.cpu().numpy()[:n], fresh.g[i], f"g[{i}]")
    buf, _ = _run(n, R, "mom-wd", 0, steps=steps)
    for i in range(R):  # kept: the stepping replicas' are rewritten, the joining one's are not
        assert np.any(buf.s[i].t.cpu().numpy()[:n] != fresh.st.s[i]) == steps[i]
        assert np.any(buf.g[i].t.cpu().numpy()[:n] != fresh.g[i]) == steps[i]


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_two_clocks_then_sma_and_elastic_on_one_plan(flags):
    """The calls share the plan's scratch and the caller's stream order."""
    from crossbow_amd.seam import SmaPlan
    from tests import averaging_common as AV
    n, R, wd = 4099, 3, 5e-4
    d = Data(n, R, 0.9, 0.9)
    buf = Buffers(d)
    rates = _rates(R)
    st = d.st
    with SmaPlan([0], n) as plan:
        for clock in range(2):
            steps = [True] * R  # every replica steps in both clocks: the discard flag's promise holds
            buf.call(plan, steps, rates, wd, flags)
            d.step(steps, rates, wd, keep=flags == 0)
            buf.check(f"clock {clock}:")
        # the plain pair next, as the promise wants before anyone reads s: a step, then a barrier
        from crossbow_amd.seam import optimise_buffers
        for i in range(R):
            optimise_buffers(buf.stream.cuda_stream, buf.w[i].ptr, buf.g[i].ptr, buf.last[i].ptr, buf.s[i].ptr, n,
                             rates[i], 0.9, wd)
            O.sma_optimise(np.float32(-rates[i]), 0.9, wd, st.w[i], d.g[i], d.last[i], st.s[i])
        reps = [(0, buf.w[i].ptr, buf.s[i].ptr, 1, 0) for i in range(R)]
        plan.step([buf.stream.cuda_stream], [buf.z.ptr], [buf.blast.ptr], reps, ALPHA, 0.9)
        O.sma_step(st)
        buf.check("after cbx_sma_plan_step:")
        plan.elastic_step([buf.stream.cuda_stream], [buf.z.ptr], [(0, buf.w[i].ptr, None, 1) for i in range(R)],
                          ALPHA)
        AV.elastic_average(st)
        buf.check("after cbx_ea_plan_step:")
        buf.call(plan, [True] * R, rates, wd, flags)
        d.step([True] * R, rates, wd, keep=flags == 0)
        buf.check("the fused call again:")


def _context(n, R, momentum, wd):
    """A context of R replicas on device 0 with an exponential rate policy."""
    from crossbow_amd import TheGPU
    g = TheGPU()
    g.init([0])
    g.setModel(1, 4 * n)
    g.setModelVariable(0, 1, [n], 4 * n)
    g.setUpdateModelType(7)  # SMA
    g.setEamsgdAlpha(ALPHA)
    g.setMomentum(momentum, 0)
    g.setWeightDecay(wd)
    g.setLearningRateDecayPolicyExp(0.05, 0.97)
    g.setModelManager(R, 0)
    return g


@pytest.mark.parametrize("flags", [0, DISCARD], ids=["keep", "discard"])
def test_seam_agrees_with_the_context(flags):
    """The other door: the same Data through cbx_step_and_synchronise on a
    context, with the rates the context itself reports for its tasks."""
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST
    from crossbow_amd.seam import SmaPlan
    from tests.helpers import upload
    n, R, momentum, wd = 4099, 4, 0.9, 5e-4
    tasks = [3 + 2 * i for i in range(R)]
    twin = _context(4, R, momentum, 0.0)  # asked for the rates only: the query may change host state
    try:
        rates = [twin.replica_learning_rate(i, tasks[i]) for i in range(R)]
    finally:
        twin.free()
    assert len(set(rates)) == R
    d = Data(n, R, momentum, momentum)
    gpu = _context(n, R, momentum, wd)
    try:
        upload(gpu, d.st)
        for i in range(R):
            gpu.replica_write(i, BUF_GRADIENT, d.g[i])
            gpu.replica_write(i, BUF_LAST, d.last[i])
        buf = Buffers(d)
        with SmaPlan([0], n) as plan:
            buf.call(plan, [True] * R, rates, wd, flags)
            buf.stream.synchronize()
        gpu.lockAny()
        gpu.step_and_synchronise(0, 1, 0, tasks, None, flags)
        gpu.unlockAny()
        gpu.wait()
        assert_bitexact(buf.z.t.cpu().numpy()[:n], gpu.base_read(0, BUF_DATA), "z")
        assert_bitexact(buf.blast.t.cpu().numpy()[:n], gpu.base_read(0, BUF_LAST), "base last")
        for i in range(R):
            for mine, kind, name in [(buf.w[i], BUF_DATA, "w"), (buf.s[i], BUF_DIFF, "s"),
                                     (buf.g[i], BUF_GRADIENT, "g"), (buf.last[i], BUF_LAST, "last")]:
                assert_bitexact(mine.t.cpu().numpy()[:n], gpu.replica_read(i, kind), f"{name}[{i}]")
    finally:
        gpu.free()


def test_each_call_adds_one_timing_entry():
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 4099, 3, 5e-4
    d = Data(n, R, 0.9, 0.9)
    buf = Buffers(d)
    rates = _rates(R)
    with SmaPlan([0], n) as plan:
        plan.set_timing(True)
        assert plan.timing_history(4) == []
        for flags in (0, DISCARD):
            buf.call(plan, [True] * R, rates, wd, flags)
            d.step([True] * R, rates, wd, keep=flags == 0)
        t = plan.timing_history(8)
        assert len(t) == 2 and all(0.0 < x < 100.0 for x in t), t
        buf.check()


# name: (what is wrong, keyword arguments of the call)
INVALID = {
    "flag_bit_2": dict(flags=2),
    "stepping_unlocked": dict(held=(1,), steps=[True, True, True]),
    "stepping_below_first": dict(first=1, steps=[True, True, True]),
    "null_g_of_a_stepping_replica": dict(g_null=(2,)),
    "null_rlast_with_replica_momentum": dict(rlast_null=(0,)),
    "null_s_of_a_joining_replica": dict(steps=[True, False, True], s_null=(1,), flags=DISCARD),
    "null_s_of_a_stepping_replica_kept": dict(s_null=(1,)),
    "null_g_array": dict(null_array=8),
    "null_step_array": dict(null_array=12),
    "null_rate_array": dict(null_array=13),
}


@pytest.mark.parametrize("name", list(INVALID))
def test_invalid_calls_write_nothing(name):
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan, _ints, _ptrs
    kw = dict(INVALID[name])
    n, R, wd = 4099, 3, 5e-4
    d = Data(n, R, 0.9, 0.9)
    d.st.first = kw.pop("first", 0)
    for i in kw.pop("held", ()):
        d.st.locked[i] = 0
    steps, flags, null_array = kw.pop("steps", [True] * R), kw.pop("flags", 0), kw.pop("null_array", None)
    buf = Buffers(d)
    rates = _rates(R)
    with SmaPlan([0], n) as plan:
        if null_array is None:
            with pytest.raises(CbxError) as e:
                buf.call(plan, steps, rates, wd, flags, **kw)
            assert e.value.code == _lib.CBX_ERR_INVALID, str(e.value)
        else:
            reps = buf.replicas(steps, rates)
            args = [plan._p, _ptrs([buf.stream.cuda_stream]), _ptrs([buf.z.ptr]), _ptrs([buf.blast.ptr]), R,
                    _ints([r[0] for r in reps]), _ptrs([r[1] for r in reps]), _ptrs([r[2] for r in reps]),
                    _ptrs([r[3] for r in reps]), _ptrs([r[4] for r in reps]), _ints([r[5] for r in reps]),
                    _ints([r[6] for r in reps]), _ints([r[7] for r in reps]), (ctypes.c_float * R)(*rates),
                    ALPHA, 0.9, 0.9, wd, 0, 0]
            args[null_array] = None
            assert plan.lib.cbx_sma_plan_step_and_optimise(*args) == _lib.CBX_ERR_INVALID
        assert "cbx_sma_plan_step_and_optimise" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        buf.check("after the refused call:")  # the host mirror never stepped
        d.st.first = 0
        d.st.locked[:] = 1
        buf.call(plan, [True] * R, rates, wd)  # and the plan still works
        d.step([True] * R, rates, wd)
        buf.check("after a good call:")


def test_more_than_64_participating_replicas_is_unsupported():
    import torch

    from crossbow_amd import CbxError, _lib
    from crossbow_amd.seam import SmaPlan
    n, R, wd = 1027, 2, 0.0
    d = Data(n, R, 0.0, 0.0)
    buf = Buffers(d)
    reps = buf.replicas([True] * R, _rates(R))
    with SmaPlan([0], n) as plan:
        with pytest.raises(CbxError) as e:
            plan.step_and_optimise([buf.stream.cuda_stream], [buf.z.ptr], None, [reps[i % R] for i in range(65)], ALPHA,
                                   0.0, 0.0, wd)
        assert e.value.code == _lib.CBX_ERR_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        buf.check()


def _refused_on(SmaPlan, L, devices, comms):
    """step_and_optimise on a plan the call does not cover, over raw guarded
    buffers (torch-free).  Returns (what the call raised, buffers that changed)."""
    from tests.test_gpu_seam import _Dev
    n, R = 4099, 2
    d = Data(n, R, 0.9, 0.9)
    mem = _Dev()
    data = {"z": d.st.z[0], "last": d.st.last[0]}
    for i in range(R):
        data.update({f"w{i}": d.st.w[i], f"s{i}": d.st.s[i], f"g{i}": d.g[i], f"l{i}": d.last[i]})
    sentinel = (np.arange(GUARD, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(0x7FC00000)).view(np.float32)
    host = {k: np.concatenate([v, sentinel]) for k, v in data.items()}
    dev = {k: mem.upload(v) for k, v in host.items()}
    stream = mem.stream()
    G = len(devices)
    plan = SmaPlan(devices, n, comms=comms, lib=L)
    try:
        reps = [(0, dev[f"w{i}"], dev[f"s{i}"], dev[f"g{i}"], dev[f"l{i}"], 1, 0, 1, 0.05) for i in range(R)]
        try:
            plan.step_and_optimise([stream] * G, [dev["z"]] * G, [dev["last"]] * G, reps, ALPHA, 0.9, 0.9, 5e-4)
            out = "the call was accepted"
        except Exception as e:  # the standalone seam raises RuntimeError("<code> <message>")
            out = str(e)
        mem.sync()
        changed = [k for k, v in host.items()
                   if not np.array_equal(mem.download(dev[k], v.size).view(np.uint32), v.view(np.uint32))]
        return out, changed
    finally:
        plan.free()
        mem.free()


def _two_device_worker(q):
    """A plan over two devices of the loopback clique (both HIP device 0)."""
    try:
        from tests.test_gpu_seam import _seam_standalone
        L, A = C.load_variant()
        out, changed = _refused_on(_seam_standalone().SmaPlan, L, [0, 0], None)
        q.put(((out, changed, A.CBX_ERR_UNSUPPORTED), None))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((None, traceback.format_exc()))


def test_a_plan_of_two_devices_is_unsupported():
    from tests.test_gpu_seam import _spawn
    assert os.path.exists(C.VARIANT), "the build makes it: scripts/build_fake_rccl.sh"
    res, err = _spawn(_two_device_worker, ())
    assert err is None, err
    out, changed, code = res
    assert out.startswith(f"{code} ") and "kernel A" in out, out
    assert not changed, changed


def _rank_worker(world, rank, d, q):
    """One rank of a real RCCL communicator of `world` ranks on the one GPU
    (one process per rank, as tests/test_gpu_seam.py::_rank_worker): a plan of
    one device whose communicator has more than one rank."""
    try:
        from tests.test_gpu_realrccl import load_real, rank_env
        from tests.test_gpu_seam import _seam_standalone, _Uid
        rank_env(rank)
        L, A = load_real()
        R = ctypes.CDLL("librccl.so.1")
        path = os.path.join(d, "uid")
        if rank == 0:
            uid = _Uid()
            assert R.ncclGetUniqueId(ctypes.byref(uid)) == 0
            with open(path + ".tmp", "wb") as f:
                f.write(bytes(uid))
            os.replace(path + ".tmp", path)
        C.wait_files([path])
        uid = _Uid.from_buffer_copy(open(path, "rb").read())
        comm = ctypes.c_void_p()
        R.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _Uid, ctypes.c_int]
        assert R.ncclCommInitRank(ctypes.byref(comm), world, uid, rank) == 0
        try:
            out, changed = _refused_on(_seam_standalone().SmaPlan, L, [0], [comm.value])
        finally:
            R.ncclCommDestroy(comm)
        q.put(((out, changed, A.CBX_ERR_UNSUPPORTED), None))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((None, traceback.format_exc()))


def test_a_one_device_plan_in_a_two_rank_communicator_is_unsupported():
    import multiprocessing as mp
    import tempfile
    world = 2
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        qs, ps = [], []
        for rank in range(world):
            q = ctx.Queue()
            p = ctx.Process(target=_rank_worker, args=(world, rank, d, q))
            p.start()
            qs.append(q)
            ps.append(p)
        try:
            res = [q.get(timeout=110) for q in qs]
        finally:
            for p in ps:
                p.join(timeout=30)
                if p.is_alive():
                    p.kill()
    errs = [e for _, e in res if e]
    assert not errs, errs[0]
    for rank, ((out, changed, code), _) in enumerate(res):
        assert out.startswith(f"{code} ") and "2 ranks" in out and "kernel A" in out, (rank, out)
        assert not changed, (rank, changed)
