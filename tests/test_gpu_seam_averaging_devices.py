"""cbx_ea_plan_step / cbx_pr_plan_step at G > 1 on ONE GPU: the seam over G
devices of one process through the loopback clique (tests/native/fake_rccl.cpp;
tests/multidev_common.py and the helpers of tests/test_gpu_seam.py, unchanged).

Each device accumulates its own replicas (kernel A), the sums are all-reduced
into the plan's D and every device applies it (kernel B), in buckets whose
last one carries the scalar tail.  Rank-order loopback: bit for bit against
the CPU restatement (tests/native/averaging_ref.c).  Ring-order loopback
(G = 4): the stated G > 1 tolerance in every element.  Always: z, and last for
Polyak-Ruppert, bitwise identical on every device.  With several ranks elastic
averaging takes its difference from the snapshots s.

Workers are spawned, torch-free processes, so no real RCCL sits beside the
loopback one.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from tests import multidev_common as C

pytestmark = pytest.mark.gpu

N, R, STEPS = 40_009, 2, 2

# (name, buckets, loopback order, caller's communicators, snapshots far from w)
# buckets: 0 = the default eight, 1 = in order on the caller's stream, 5 = a
# ragged last bucket (4 x 2,048 + 1,792 float4s of the 9,984 in the bulk) that
# carries the 73-float tail.  Bucket starts stay on kPadFloat4, so at this size
# the default of eight comes to the same five.
JOBS = [
    ("default-buckets", 0, "rank", False, False),
    ("in-order", 1, "rank", False, False),
    ("ragged-last-bucket", 5, "rank", False, False),
    ("snapshots-far-from-w", 0, "rank", False, True),
    ("caller-comms", 0, "rank", True, False),
    ("ring-order", 0, "ring", False, False),
]


def _run(L, world, polyak, buckets, exact, comms, far_s):
    from tests import averaging_common as AV
    from tests.test_gpu_seam import _Dev, _seam_standalone
    O = C.oracle()
    SmaPlan = _seam_standalone().SmaPlan
    st = O.make_state(N, world, R, 0.1, 0.9)
    size = world * R
    if far_s:  # a step that read w instead of s (one rank's rule) would show everywhere
        for i in range(size):
            st.s[i] = O.fill_normal(N, 800 + i, 0.05)
    s0 = [a.copy() for a in st.s]
    mem = _Dev()
    devs = list(range(world))
    z = [mem.upload(st.z[d]) for d in devs]
    last = [mem.upload(st.last[d]) for d in devs]
    w = [mem.upload(a) for a in st.w]
    s = [mem.upload(a) for a in st.s]
    streams = [mem.stream() for _ in devs]
    plan = SmaPlan([0] * world, N, comms=comms, lib=L, buckets=buckets)
    bad = []
    try:
        for clock in range(STEPS):
            st.locked[:] = 1
            if polyak and clock == 1:
                st.copy[size - 1] = 1
            if polyak:
                reps = [(i % world, w[i], int(st.locked[i]), int(st.copy[i])) for i in range(size)]
                got = plan.polyak_step(streams, z, last, reps, 0.1, clock)
                want = AV.polyak_ruppert(st, clock)
                if got != want:
                    bad.append(f"clock {clock}: returned {got}, the restatement copied {want}")
            else:
                reps = [(i % world, w[i], s[i], int(st.locked[i])) for i in range(size)]
                plan.elastic_step(streams, z, reps, 0.1)
                AV.elastic_average(st)
        mem.sync()
        check = C.Checker(exact=exact)
        dig = {}
        for d in devs:
            zd, ld = mem.download(z[d], N), mem.download(last[d], N)
            dig[d] = C.digest(zd, ld)
            check(f"z[{d}]", zd, st.z[d])
            check(f"last[{d}]", ld, st.last[d])  # elastic averaging: untouched
        for i in range(size):
            check(f"w[{i}]", mem.download(w[i], N), st.w[i])
            if not np.array_equal(mem.download(s[i], N).view(np.uint32), s0[i].view(np.uint32)):
                bad.append(f"s[{i}] was written")
        if polyak and not np.array_equal(mem.download(w[size - 1], N).view(np.uint32),
                                         mem.download(z[(size - 1) % world], N).view(np.uint32)):
            bad.append("the flagged replica is not its device's z")
        return {"bad": bad + check.bad, "digest": dig, "differs": check.differs}
    finally:
        plan.free()
        mem.free()


def _worker(G, polyak, q):
    try:
        L, A = C.load_variant()
        F = ctypes.CDLL(os.path.join(C.ROOT, "tests", "native", "libfakerccl.so"))
        out = []
        for name, buckets, order, caller, far_s in JOBS:
            if order == "ring" and G < 4:
                continue
            os.environ["FAKE_RCCL_ORDER"] = order
            comms = None
            if caller:  # the caller's communicators, as executioncontext.c:185-201 creates them
                arr = (ctypes.c_void_p * G)()
                devs = (ctypes.c_int * G)(*([0] * G))
                assert F.ncclCommInitAll(arr, G, devs) == 0
                comms = [arr[k] for k in range(G)]
            try:
                r = _run(L, G, polyak, buckets, order == "rank", comms, far_s)
            finally:
                for c in comms or ():
                    F.ncclCommDestroy(ctypes.c_void_p(c))
            out.append((name, r))
        q.put((out, None))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((None, traceback.format_exc()))


@pytest.mark.skipif(not os.path.exists(C.VARIANT), reason="run scripts/build_fake_rccl.sh first")
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("polyak", [False, True], ids=["elastic", "polyak"])
def test_seam_averaging_devices_one_process(G, polyak):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(G, polyak, q))
    p.start()
    try:
        res, err = q.get(timeout=60)
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert p.exitcode == 0
    assert len(res) == (len(JOBS) if G == 4 else len(JOBS) - 1)
    for name, r in res:
        assert not r["bad"], (name, r["bad"])
        assert len(set(r["digest"].values())) == 1, f"{name}: z / last differ across devices"
