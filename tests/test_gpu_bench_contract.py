"""bench.py's output contract, on the GPU: exactly ONE JSON line on stdout
(native libraries' banners go to stderr), with the fields the driver reads,
at N = 1 and through the driver's own N > 1 launcher (torch.distributed.run,
two ranks on the one GPU over RCCL's socket transport: --rehearse-one-gpu).
Short runs: the numbers are not checked here, only the shape of the line."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-staged", "--no-copy-ceiling", "--no-optimiser", "--no-seam"]


def _one_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must carry exactly one line, got {len(lines)}: {lines[:3]}"
    return json.loads(lines[0])


def _check(d: dict, n: int):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == n and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert 0 < r["frac"] < 1 and r["achieved"] > 0
    assert "workload" in d["config"]


@pytest.mark.timeout(240)
def test_bench_one_gpu_prints_one_json_line():
    p = subprocess.run([sys.executable, "bench.py"] + QUICK, cwd=ROOT, capture_output=True, text=True, timeout=220)
    assert p.returncode == 0, p.stderr[-2000:]
    _check(_one_line(p.stdout), 1)


@pytest.mark.timeout(300)
def test_bench_two_ranks_through_the_launcher_prints_one_json_line():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29671", "bench.py", "--gpus", "2",
           "--rehearse-one-gpu", "--bucket-mb", "16", "--full"] + QUICK
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    assert d["config"]["parallelism"] == "sma-dp2" and "allreduce" in d and "rehearsal" in d
    assert d["config"]["process_form"] == "per-rank"
    # an explicit configuration: the per-rank peer-read form's block is not run
    assert d["config"]["peer_ipc"] == "not attempted: explicit configuration"
    # N > 1: the roofline of the kernels as they ran in the timed region
    # (summed busy spans beside the collectives), the calibration's apart
    r = d["roofline"]
    assert r["timed_in"].startswith("timed region") and r["launches"] >= 3
    assert 0 < r["apply_kernel"]["frac"] < 1 and 0 < r["a_plus_b"]["frac"] < 1
    assert r["collective_busy_ms_mean"] > 0
    assert d["roofline_unpipelined"]["timed_in"].startswith("calibration")
    # the link rate of the collectives as they ran in the timed region, the
    # calibration's (the collective alone) apart
    ar = d["allreduce"]
    assert ar["timed"]["busbw_GBs"] > 0, ar
    assert ar["timed"]["xgmi_frac"] is None and "no xGMI link" in ar["timed"]["note"]  # one GPU: no link fraction
    assert ar["timed"]["timed_in"].startswith("timed region")
    assert ar["unpipelined"]["busbw_GBs"] > 0 and ar["unpipelined"]["timed_in"].startswith("calibration")
    # RCCL's own tuning choices, parsed from its TUNING log of a separate short
    # run (the measured run keeps RCCL's per-collective log off)
    t = ar["rccl_tuning"]
    assert isinstance(t, list) and t, ar
    assert all(e["collective"] and e["algo"] and e["proto"] and e["bytes"] > 0 and e["calls"] > 0 for e in t)
    assert "separate" in ar["rccl_tuning_source"]
    assert d["host"]["enqueue_ms_per_step_timed"] > 0 and d["host"]["devices_per_process"] == 1
    assert d["config"]["hw_queues"]["GPU_MAX_HW_QUEUES"] >= 1
    # every rank ends the timed region with the same z and last, bit for bit
    idn = d["identity"]
    assert idn["z_last_identical_on_every_gpu"] is True and idn["finite"] is True and idn["gpus_checked"] == 2
    # the measured (bucketed) configuration against one in-order all-reduce of
    # the same step, from a fresh state (values of order 1: not vacuous)
    agree = idn["vs_all_reduce"]
    assert agree["within_tolerance"] is True and agree["vacuous"] is False and agree["max_abs_value"] < 1, agree
    assert idn["trusted"] is True and idn["max_abs_value"] > 0


TUNED = ["--tune-steps", "2", "--tune-passes", "1", "--calib-steps", "2"]


@pytest.mark.timeout(300)
def test_bench_two_ranks_peer_block_after_the_rccl_forms():
    """One process per GPU, tuner on: the RCCL forms are tuned and timed
    first; then the peer-read form's IPC mapping, its tuner candidates and
    (when its best candidate beats RCCL's) its own timed block.  The faster
    timed block sets `value`, the other is kept in `other_form`."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29675", "bench.py", "--gpus", "2",
           "--rehearse-one-gpu", "--no-rccl-tuning-run"] + QUICK + TUNED
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    c = d["config"]
    assert c["peer_ipc"] == "mapped", c["peer_ipc"]
    assert "incomplete_phase" not in d
    table = c["bucket_tuning_ms_per_step"]
    other = d["other_form"]
    if c["allreduce_algorithm"] == "peer-read two-shot":  # the peer block won and set `value`
        assert all(k.endswith("/peer") for k in table) and other["value"] > 0 and other["value"] <= d["value"]
        assert other["config"]["allreduce_algorithm"] != "peer-read two-shot"
    else:  # RCCL's block set `value`; the peer form was tuned (and maybe timed) after it
        assert not any(k.endswith("/peer") for k in table), table
        assert all(k.endswith("/peer") for k in other["config"]["bucket_tuning_ms_per_step"]), other
    assert d["identity"]["trusted"] is True, d["identity"]


@pytest.mark.timeout(300)
def test_bench_two_ranks_survives_a_stalled_ipc_mapping():
    """VERDICT r04 Next #1: rank 0 stuck where the IPC handles are opened
    ($CBX_FAULT_IPC_STALL: as a thread inside hipIpcOpenMemHandle would be,
    out of reach of the library's timers) must not cost the line: the RCCL
    forms' block is measured first, the mapping misses its deadline, and the
    watchdog prints that block's line naming the failure; exit 0."""
    env = dict(os.environ, CBX_FAULT_IPC_STALL="600")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29677", "bench.py", "--gpus", "2",
           "--rehearse-one-gpu", "--no-rccl-tuning-run", "--peer-ipc-deadline", "30"] + QUICK + TUNED
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    assert d["incomplete_phase"]["phase"] == "peer-read IPC mapping", d["incomplete_phase"]
    assert d["config"]["peer_ipc"].startswith("failed: 'peer-read IPC mapping' missed its 30 s deadline")
    assert d["config"]["allreduce_algorithm"] in ("all-reduce", "reduce-scatter+all-gather")
    assert d["allreduce"]["timed"]["busbw_GBs"] > 0 and d["identity"]["trusted"] is True
    assert "WATCHDOG" in p.stderr and " wchan=" in p.stderr


@pytest.mark.timeout(300)
def test_bench_two_ranks_keeps_the_line_when_another_rank_crashes():
    """A rank that dies after the line exists (here rank 1, SIGKILLed as it
    enters the IPC mapping, $CBX_BENCH_FAULT_KILL) makes torch.distributed.run
    SIGTERM every other rank: rank 0 prints the RCCL block's line naming the
    phase it was ended in -- by that SIGTERM, or by its gloo collective
    failing first (connection reset), whichever comes first.  The launcher
    itself still reports rank 1's exit."""
    env = dict(os.environ, CBX_BENCH_FAULT_KILL="1:peer-read IPC mapping")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29679", "bench.py", "--gpus", "2",
           "--rehearse-one-gpu", "--no-rccl-tuning-run"] + QUICK + TUNED
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode != 0, p.stderr[-3000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    inc = d["incomplete_phase"]
    assert inc["phase"] == "peer-read IPC mapping" and inc["error"], inc
    assert inc["error"] == "SIGTERM" or "Connection reset" in inc["error"], inc
    assert d["allreduce"]["timed"]["busbw_GBs"] > 0 and d["identity"]["trusted"] is True


@pytest.mark.timeout(300)
def test_bench_single_process_two_devices_one_gpu():
    """The reference's own multi-GPU topology: one process over N devices
    (cbx_init -> ncclCommInitAll), here two devices that are both device 0,
    so the all-reduce is the peer-read form (RCCL refuses a repeated device)."""
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--single-process", "--rehearse-one-gpu", "--full"] + QUICK
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    c = d["config"]
    assert c["process_form"] == "single" and c["allreduce_algorithm"] == "peer-read two-shot"
    assert d["host"]["devices_per_process"] == 2 and d["host"]["enqueue_ms_per_step_idle_gpu"] > 0
    assert d["roofline"]["timed_in"].startswith("timed region") and "roofline_unpipelined" in d
    assert "rehearsal" in d
    # the tuner timed the peer-read form at 1 / 4 / 8 buckets and, for the
    # winner, one enqueue thread per device against the reference's one
    table = c["bucket_tuning_ms_per_step"]
    assert {"1/0/peer", "4/0/peer", "4/1/peer", "8/1/peer"} <= set(table), table
    assert any(k.endswith("/t1") for k in table), table
    assert c["enqueue_threads"] in (0, 1) and c["buckets"] in (1, 4, 8)
    assert not c["tuning_errors"], c["tuning_errors"]
    assert d["allreduce"]["rccl_tuning"] is None and d["allreduce"]["timed"]["busbw_GBs"] > 0
    assert d["identity"]["z_last_identical_on_every_gpu"] is True and d["identity"]["gpus_checked"] == 2


@pytest.mark.timeout(300)
def test_bench_tuner_drops_a_failing_candidate():
    """A tuner candidate whose steps fail ($CBX_FAULT_FAIL_STEP_BUCKETS: every
    split step over exactly 4 buckets returns an error before it enqueues
    anything) is dropped and recorded; the run goes on and picks another."""
    env = dict(os.environ, CBX_FAULT_FAIL_STEP_BUCKETS="4")
    cmd = [sys.executable, "bench.py", "--force-split"] + QUICK
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_line(p.stdout)
    _check(d, 1)
    c = d["config"]
    assert sorted(c["tuning_errors"]) == ["4/0", "4/1", "4/1/s2"], c["tuning_errors"]
    assert all("fault injection" in v for v in c["tuning_errors"].values())
    assert not any(k.startswith("4/") for k in c["bucket_tuning_ms_per_step"])
    assert c["buckets"] != 4 and "1/0" in c["bucket_tuning_ms_per_step"]


@pytest.mark.timeout(300)
def test_bench_two_ranks_host_staged_field():
    # the N > 1 host-staged leg (zero-copy staging over two rehearsal ranks)
    quick = [a for a in QUICK if a != "--no-staged"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29673", "bench.py", "--gpus", "2",
           "--rehearse-one-gpu", "--bucket-mb", "16", "--full"] + quick
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_line(p.stdout)
    _check(d, 2)
    z = d["host_staged"]["zerocopy"]
    assert z["step_ms"] > 0 and z["end_to_end_GBs"] > 0 and z["per_gpu_GBs"] > 0


@pytest.mark.timeout(300)
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run times the steps and prints the line: none of the legs that
    take runs of their own (--full) are in it.  --dump-outputs writes what the
    last timed step left for the caller -- z, last and every replica's w --
    bit for bit what the oracle computes in warm-up + timed steps from the
    synthetic state this process fills with the same seed (so the inputs, and
    with them the files, are the same from run to run).  LeNet: whole arrays."""
    import numpy as np

    from oracle import oracle as O
    n, R, W, K = 1_111_946, 8, 1, 3
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--model", "lenet",
           "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=140)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_line(p.stdout)
    _check(d, 1)
    for key in ("replica_optimiser", "seam", "copy_ceiling_GBs", "host_staged", "cpu_baseline",
                "cpu_baseline_multithread", "cpu_c1_lenet"):
        assert key not in d, key
    names = ["z", "last"] + [f"w{i}" for i in range(R)]
    assert d["outputs"]["arrays"] == names and d["outputs"]["elements_per_array"] == n
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{k}.npy" for k in names)
    got = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in names}
    assert sum(os.path.getsize(tmp_path / "out" / f"{k}.npy") for k in names) <= 64_000_000
    # the inputs: the library's own synthetic state, as bench.py sets it up
    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd.variables import MODELS, register
    g = TheGPU()
    g.init([0])
    try:
        assert register(g, MODELS["lenet"]()) == n
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setModelManager(R, SYNC_BSP)
        g.fill_synthetic(O.SEED)
        st = O.SmaState(1, R, n, 0.1, 0.9, [g.base_read(0, BUF_DATA)], [g.base_read(0, BUF_LAST)],
                        [g.replica_read(i, BUF_DIFF) for i in range(R)],
                        [g.replica_read(i, BUF_DATA) for i in range(R)])
    finally:
        g.free()
    for _ in range(W + K):
        O.sma_step(st)
    want = dict([("z", st.z[0]), ("last", st.last[0])] + [(f"w{i}", st.w[i]) for i in range(R)])
    for k, a in got.items():
        assert a.dtype == np.float32 and a.shape == (n,)
        assert np.array_equal(a.view(np.uint32), want[k].view(np.uint32)), f"{k} differs from the oracle"
