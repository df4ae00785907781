#!/usr/bin/env python3
"""Time the three fused model-averaging barriers in one session on one GPU:
SMA (update model 7), elastic averaging (3 with cbx_set_elastic_average) and
Polyak-Ruppert (6), on ResNet-50's parameters with R = 8 replicas.

Times are the library's own dispatch timestamps (cbx_timing_history,
CBX_T_KERNEL): each fused step is one kernel whose dispatch stamps its own
start and stop, so nothing of the host or the queue is in them.  Per model:
`--warmup` untimed steps, then `--repeats` runs of `--steps` back-to-back
steps; the figure is the median step of each run, and the spread over the runs
is reported beside their median.  The float4 copy ceiling (launch_copy) is
measured in the same process before and after, and every model is reported as
a fraction of it; SMA's fraction in the same run is the yardstick for the two
new kernels, not a fixed number.

Algorithmic bytes per step (every input read once, every output written once):
  SMA               (3R + 2 + 2m) * 4n   reads z, last, s_i, w_i; writes w_i, z, last
  elastic averaging (2R + 2) * 4n        reads z, w_i; writes w_i, z
  Polyak-Ruppert    (2R + 2 + m) * 4n    the same, and writes last (m = 1 if momentum > 0)

One JSON line per model on stdout.  With --sweep, one line per model and
launch geometry instead (float4s per lane x waves per CU, -1 = the library's
automatic cap), for retuning the kernels' launch configuration.
Usage: python3 scripts/bench_averaging.py [--steps 200] [--warmup 50] [--repeats 3] [--replicas 8] [--momentum 0.9]
                                          [--sweep]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, datasheet


def make(model, R, momentum):
    from crossbow_amd import SYNC_BSP, UPDATE_POLYAK_RUPPERT, UPDATE_SMA, UPDATE_SYNCHRONOUSEAMSGD, TheGPU
    from crossbow_amd.variables import MODELS, register
    g = TheGPU()
    g.init([0])
    n = register(g, MODELS["resnet50"]())
    g.setUpdateModelType({"sma": UPDATE_SMA, "elastic": UPDATE_SYNCHRONOUSEAMSGD, "polyak": UPDATE_POLYAK_RUPPERT}[model])
    if model == "elastic":
        g.setElasticAverage(True)
    g.setEamsgdAlpha(0.1)
    g.setMomentum(momentum, 0)
    g.setModelManager(R, SYNC_BSP)
    g.fill_synthetic(1)
    return g, n


def run_steps(g, count, clock):
    for _ in range(count):
        g.lockAny()
        g.synchronise(0, clock, 0, False)
        g.unlockAny()
        clock += 1
    g.wait()
    return clock


def copy_ceiling(g, n):
    # two buffers of the model's size times four: far beyond the 256 MiB last-level cache
    return g.bench_copy(16 * n, 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    from crossbow_amd._lib import T_KERNEL
    R, m = args.replicas, 1 if args.momentum > 0 else 0
    floats = {"sma": 3 * R + 2 + 2 * m, "elastic": 2 * R + 2, "polyak": 2 * R + 2 + m}
    rows = []
    copies = []
    shapes = [(u, w) for u in (1, 2, 4) for w in (-1, 2, 3, 4, 5, 6, 8, 12)] if args.sweep else [(None, None)]
    for model in ("sma", "elastic", "polyak"):
        g, n = make(model, R, args.momentum)
        try:
            copies.append(copy_ceiling(g, n))
            g.set_timing(True)
            clock = 0
            for unroll, waves in shapes:
                if unroll is not None and model == "sma":
                    g.set_kernel_config(block=64, blocks_per_cu=0, policy=1, unroll=unroll)
                    g.set_kernel_occupancy(waves)
                elif unroll is not None:
                    g.set_averaging_kernel_config(64, unroll, waves)
                clock = run_steps(g, args.warmup, clock)
                medians = []
                for _ in range(args.repeats):
                    clock = run_steps(g, args.steps, clock)
                    t = g.timing_history(T_KERNEL, 0, args.steps)
                    assert t.size == args.steps and np.all(t > 0), "a step kept no kernel time"
                    medians.append(float(np.median(t)) * 1e3)
                rows.append({"model": model, "n": n, "replicas": R, "momentum": args.momentum,
                             "bytes_per_step": floats[model] * 4 * n, "kernel_us_runs": [round(x, 2) for x in medians]})
                if unroll is not None:
                    rows[-1].update({"unroll": unroll, "waves_per_cu": waves})
            copies.append(copy_ceiling(g, n))
        finally:
            g.free()
    copy = float(np.median(copies))
    for row in rows:
        us = float(np.median(row["kernel_us_runs"]))
        gbps = row["bytes_per_step"] / (us * 1e-6) / 1e9
        row.update({"kernel_us": round(us, 2),
                    "spread_pct": round(100.0 * (max(row["kernel_us_runs"]) - min(row["kernel_us_runs"])) / us, 2),
                    "gbps": round(gbps, 1), "of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
                    "copy_gbps": round(copy, 1), "copy_gbps_runs": [round(c, 1) for c in copies],
                    "of_copy": round(gbps / copy, 4), "steps": args.steps, "warmup": args.warmup})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
