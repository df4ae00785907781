"""The elastic-averaging and Polyak-Ruppert barriers at G > 1 on ONE GPU,
through the loopback collective (tests/native/fake_rccl.cpp; the machinery of
tests/multidev_common.py, unchanged).

Each device accumulates its own replicas, the sums are all-reduced and every
device applies the same D.  Rank-order loopback: bit for bit against the CPU
restatement (tests/native/averaging_ref.c sums the per-device partials in
rank order from rank 0's).  Ring-order loopback (G = 4): the stated G > 1
tolerance over every element.  Always: z, and last for Polyak-Ruppert,
bitwise identical on every device.

Workers are spawned, torch-free processes, so no real RCCL sits beside the
loopback one.
"""
from __future__ import annotations

import ctypes
import os
import tempfile

import pytest

from tests import multidev_common as C

pytestmark = pytest.mark.gpu

N = 50_000
ONE_BUCKET = 1 << 40


def _run(g, world, local, polyak, R, bucket, order):
    """Two steps (clocks 0 and 1) on the devices `local` of a G = `world` job;
    Polyak-Ruppert's second step has one copy flag raised."""
    from tests import averaging_common as AV
    O = C.oracle()
    A = g.A
    mom = 0.9
    C.setup_model(g, A, N, R, mom, A.UPDATE_POLYAK_RUPPERT if polyak else A.UPDATE_SYNCHRONOUSEAMSGD, A.SYNC_BSP,
                  2 * world * R)
    if not polyak:
        g("cbx_set_elastic_average", 1)
    if bucket:
        g("cbx_set_bucket_elements", ctypes.c_longlong(bucket))
    size = world * R
    mine = [i for i in range(size) if i % world in local]
    st = O.make_state(N, world, R, 0.1, mom)
    for d in local:
        g.write("cbx_base_write", d, A.BUF_DATA, st.z[d])
        g.write("cbx_base_write", d, A.BUF_LAST, st.last[d])
    for i in mine:
        g.write("cbx_replica_write", i, A.BUF_DIFF, st.s[i])
        g.write("cbx_replica_write", i, A.BUF_DATA, st.w[i])
    flagged = size - 1
    for clock in (0, 1):
        if clock == 1:
            st.copy[flagged] = 1
            if flagged in mine:
                g("cbx_replica_set_copy", flagged, 1)
        g("cbx_lock_any")
        g("cbx_synchronise", 0, clock, 0, 0)
        g("cbx_unlock_any")
        AV.step(st, polyak, clock)
    g("cbx_wait")
    check = C.Checker(exact=order == "rank" or world < 3)
    dig = {}
    for d in local:
        z = g.read("cbx_base_read", d, A.BUF_DATA, N)
        last = g.read("cbx_base_read", d, A.BUF_LAST, N)
        dig[d] = C.digest(z, last)
        check(f"z[{d}]", z, st.z[d])
        check(f"last[{d}]", last, st.last[d])  # elastic averaging: untouched
    for i in mine:
        check(f"w[{i}]", g.read("cbx_replica_read", i, A.BUF_DATA, N), st.w[i])
        if g("cbx_replica_get_copy", i) != int(st.copy[i]):
            check.bad.append(f"copy flag of replica {i} is not {int(st.copy[i])}")
    return {"bad": check.bad, "digest": dig}


def _jobs(G):
    jobs = [(R, bucket, "rank") for R in (1, 3) for bucket in (0, ONE_BUCKET)]
    if G == 4:
        jobs += [(R, 0, "ring") for R in (1, 3)]
    return jobs


def _worker(G, polyak, jobs, q):
    try:
        L, A = C.load_variant()
        out = []
        for R, bucket, order in jobs:
            os.environ["FAKE_RCCL_ORDER"] = order
            g = C.init_local(L, A, G)
            try:
                out.append(_run(g, G, list(range(G)), polyak, R, bucket, order))
            finally:
                g.free()
        q.put((out, None))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((None, traceback.format_exc()))


@pytest.mark.skipif(not os.path.exists(C.VARIANT), reason="run scripts/build_fake_rccl.sh first")
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("polyak", [False, True], ids=["elastic", "polyak"])
def test_one_process_many_devices_vs_restatement(G, polyak):
    import multiprocessing as mp
    jobs = _jobs(G)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(G, polyak, jobs, q))
    p.start()
    try:
        res, err = q.get(timeout=60)
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert p.exitcode == 0
    for job, r in zip(jobs, res):
        assert not r["bad"], (job, r["bad"])
        assert len(set(r["digest"].values())) == 1, f"{job}: z / last differ across devices"


def _rank_main(rank, world, uids, fake_dir, q):
    os.environ["FAKE_RCCL_DIR"] = fake_dir
    os.environ["FAKE_RCCL_ORDER"] = "rank"
    try:
        L, A = C.load_variant()
        out = []
        for polyak, uid in zip((False, True), uids):
            g = C.init_rank(L, A, rank, world, uid)
            try:
                out.append(_run(g, world, [rank], polyak, 3, 0, "rank"))
            finally:
                g.free()
        q.put((rank, out, None))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.skipif(not os.path.exists(C.VARIANT), reason="run scripts/build_fake_rccl.sh first")
def test_one_process_per_rank_vs_restatement():
    # cbx_init_rank, G = 2: both steps, 3 replicas per rank, the default buckets.
    import multiprocessing as mp
    world = 2
    uids = [os.urandom(16) + bytes(112) for _ in range(2)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    got = {}
    with tempfile.TemporaryDirectory(dir=C.loopback_dir()) as fake_dir:
        procs = [ctx.Process(target=_rank_main, args=(r, world, uids, fake_dir, q)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            for _ in range(world):
                rank, res, err = q.get(timeout=60)  # each child under its own limit
                # a rank that failed leaves the other waiting in a collective: stop here
                assert err is None, f"rank {rank}:\n{err}"
                got[rank] = res
        finally:
            for p in procs:
                p.join(timeout=30 if len(got) == world else 1)
                if p.is_alive():
                    p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    for j in range(2):
        for rank in range(world):
            assert not got[rank][j]["bad"], (rank, j, got[rank][j]["bad"])
        assert got[0][j]["digest"][0] == got[1][j]["digest"][1], "z / last differ across ranks"
