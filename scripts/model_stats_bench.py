#!/usr/bin/env python3
"""Time cbx_model_stats at the C3 shape: ResNet-50's variables as bench.py
registers them (n = 25,557,032, 161 variables), 8 replicas, one GPU.

In one process: the float4 copy ceiling (cbx_bench_copy), 5 warm-up and 20
timed calls of the reduction with per-variable results, and one timed
synchronise step for scale.  Prints one JSON line:

  ms_per_call            host wall time of a blocking call (median of 20)
  pass_ms / device_ms    the pass over memory alone / with its two reductions,
                         from the dispatches' own timestamps (medians)
  read_GBs               (R + 1) * 4n bytes over pass_ms
  fraction_of_read_ceiling   read_GBs over the copy ceiling.  cbx_bench_copy
                         already counts the read and the write of every byte
                         it copies (the doubling), so a reader that keeps the
                         bus as busy as the copy does scores 1.0
  sma_step_ms            one fused synchronise step (device time)

Usage: python scripts/model_stats_bench.py [--replicas 8] [--calls 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    args = ap.parse_args()

    from crossbow_amd import SYNC_BSP, UPDATE_SMA, TheGPU, _lib
    from crossbow_amd.build import code_object_digest
    from crossbow_amd.variables import MODELS, register

    g = TheGPU()
    g.init([0])
    try:
        shapes = MODELS[args.model]()
        n = register(g, shapes)
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setModelManager(args.replicas, SYNC_BSP)
        g.fill_synthetic(20260101)
        g.set_timing(True)
        g.wait()
        copy = g.bench_copy(1 << 30, 20)

        wall, pass_ms, dev_ms = [], [], []
        out = None
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            out = g.modelStats(_lib.BUF_DATA, per_variable=True)
            t1 = time.perf_counter()
            p, t = g.model_stats_last_ms()
            if k >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                pass_ms.append(p)
                dev_ms.append(t)
        base, reps, _, _ = out

        g.lockAny()
        try:
            g.synchronise(0, 1, 0, False)
        finally:
            g.unlockAny()
        g.wait()
        step_ms = float(g.last_timing()[_lib.T_STEP])

        R = args.replicas
        nbytes = (R + 1) * 4 * n
        p_med = statistics.median(pass_ms)
        read = nbytes / (p_med * 1e-3) / 1e9
        line = {
            "metric": "cbx_model_stats, per-variable, one pass over z and every w",
            "model": args.model, "elements": n, "variables": len(shapes), "replicas": R,
            "bytes_read": nbytes,
            "ms_per_call": round(statistics.median(wall), 4),
            "ms_per_call_min": round(min(wall), 4),
            "pass_ms": round(p_med, 4), "pass_ms_min": round(min(pass_ms), 4),
            "device_ms": round(statistics.median(dev_ms), 4),
            "read_GBs": round(read, 1),
            "copy_ceiling_GBs": round(copy, 1),
            # the copy ceiling counts a read and a write per byte copied: a
            # reader at the same bus rate reads copy_ceiling bytes per second
            "fraction_of_read_ceiling": round(read / copy, 4),
            "sma_step_ms": round(step_ms, 4),
            "calls": args.calls, "warmup": args.warmup,
            "check": {"z_sum_sq": float(base[0]["sum_sq"]), "w0_dist_sq": float(reps[0]["dist_sq"]),
                      "nonfinite": int(base[0]["nonfinite"] + reps["nonfinite"].sum())},
            "code_object_digest": code_object_digest(),
        }
        print(json.dumps(line))
    finally:
        g.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
