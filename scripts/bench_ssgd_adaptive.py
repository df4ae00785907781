#!/usr/bin/env python3
"""Time one synchronous-SGD clock (update model WORKER) with and without layer-wise adaptive rates
(cbx_set_adaptive_rate) at ResNet-50's shape: its 161 variables as bench.py registers them (n = 25,557,032), one
GPU, 8 replicas all stepping, base momentum 0.9, the batch-norm variables excluded from the scaling.

  plain      cbx_step_and_synchronise_ssgd, the rates off             (8R + 24) n bytes, 1 launch
  fused      cbx_step_and_synchronise_ssgd_adaptive, flags 0          (8R + 36) n bytes, 3 launches
  discard    the same with CBX_STEP_DISCARD_TASK_OUTPUTS              (8R + 36) n bytes

(with --weight-decay > 0: (16R + 24) n, (16R + 36) n and (12R + 36) n.)  Every clock runs on the sync stream.  The
script starts one fresh process per measurement (`--processes`, default 2).  Per process: `--warmup` clocks of each
kind, then `--runs` (3) runs of `--steps` (1000: windows of 0.35 to 0.5 s) back-to-back clocks of each kind, the
kinds alternating, each run between two events that wait for the step event.  The plain call's kernel lives in an
object that this change does not touch, so it is the yardstick, timed in the same process.  Without weight decay
the byte model predicts
(8R + 36) / (8R + 24) = 100/88 = 1.136 x the plain call's time for both adaptive kinds, which are then one kernel.

Prints one JSON line per process and, with --record, writes every run of every kind to FILE (default
profiles/ssgd_adaptive/bench.jsonl), replacing it.

Usage: python scripts/bench_ssgd_adaptive.py [--processes 2] [--weight-decay 0] [--record [FILE]]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
KINDS = ("plain", "fused", "discard")


def worker(args) -> int:
    import torch

    from crossbow_amd import BUF_GRADIENT, SYNC_BSP, TheGPU, build
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int
    g = TheGPU()
    g.init([0])
    try:
        shapes = MODELS["resnet50"]()
        n = register(g, shapes)
        bn = [k for k, s in enumerate(shapes) if len(s) == 1 and k != len(shapes) - 1]
        for k in bn:
            g.set_model_variable_adaptive_rate(k, 1, False)
        R = args.replicas
        g.setUpdateModelType(1)  # CBX_UPDATE_WORKER
        g.setModelWorkPerClock(R)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(args.weight_decay)
        g.setLearningRateDecayPolicyFixed(0.05)
        g.setModelManager(R, SYNC_BSP)
        g.fill_synthetic(20260101)
        grad = O.fill_normal(n, 77, 0.01)
        for i in range(R):
            g.replica_write(i, BUF_GRADIENT, grad)
        g.wait()
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0}

        def clock(kind):
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"] += 1
            g.lockAny()
            if kind == "plain":
                g.step_and_synchronise_ssgd(0, state["clock"], 0, tasks)
            else:
                g.step_and_synchronise_ssgd_adaptive(0, state["clock"], 0, tasks, None,
                                                     STEP_DISCARD_TASK_OUTPUTS if kind == "discard" else 0)
            g.unlockAny()

        def mark():
            """An event on the side stream behind the end of the last step."""
            if hip.hipStreamWaitEvent(side.cuda_stream, g.step_event(0), 0) != 0:
                raise RuntimeError("hipStreamWaitEvent failed")
            e = torch.cuda.Event(enable_timing=True)
            e.record(side)
            return e

        def timed(kind, count):
            # the switch is host state only: no launch, no synchronise
            g.set_adaptive_rate(0.0 if kind == "plain" else 0.001, 0.0 if kind == "plain" else 1e-9, 0)
            a = mark()
            for _ in range(count):
                clock(kind)
            b = mark()
            b.synchronize()
            return a.elapsed_time(b) / count

        for kind in KINDS:
            timed(kind, args.warmup)
        g.wait()
        ms = {kind: [] for kind in KINDS}
        for _ in range(args.runs):
            for kind in KINDS:
                ms[kind].append(timed(kind, args.steps))
        g.wait()
        applied = int(sum(1 for r in g.base_adaptive_stats(0, len(shapes)) if r["flags"] & 1))
        med = {kind: statistics.median(v) for kind, v in ms.items()}
        spread = {kind: max(v) - min(v) for kind, v in ms.items()}
        wd = args.weight_decay > 0
        model = {"plain": (16 if wd else 8) * R + 24, "fused": (16 if wd else 8) * R + 36,
                 "discard": (12 if wd else 8) * R + 36}
        line = {"metric": "one synchronous-SGD clock: the plain fused call against the one with layer-wise adaptive rates",
                "process": args.process, "elements": n, "variables": len(shapes), "excluded_variables": len(bn),
                "variables_with_an_applied_ratio": applied, "replicas": R, "momentum": 0.9,
                "weight_decay": args.weight_decay, "steps": args.steps, "runs": args.runs, "warmup": args.warmup,
                "timing": "events around a run of back-to-back clocks",
                "code_object_digest": {"plain": build.code_object_digest(build.SSGD_STEPS_LIB),
                                       "fused": build.code_object_digest(build.SSGD_ADAPTIVE_LIB)},
                "kinds": [{"kind": kind, "median_ms": round(med[kind], 5), "spread_ms": round(spread[kind], 5),
                           "runs_ms": [round(x, 5) for x in ms[kind]],
                           "time_over_plain": round(med[kind] / med["plain"], 4),
                           "bytes_over_plain": round(model[kind] / model["plain"], 4),
                           "GB_per_s": round(model[kind] * n / med[kind] / 1e6, 1)} for kind in KINDS]}
        print(json.dumps(line))
    finally:
        g.free()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--record", nargs="?", default=None, metavar="FILE",
                    const=os.path.join(HERE, "profiles", "ssgd_adaptive", "bench.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--process", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    for k in range(args.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--process", str(k + 1), "--replicas",
               str(args.replicas), "--steps", str(args.steps), "--runs", str(args.runs), "--warmup", str(args.warmup),
               "--weight-decay", str(args.weight_decay)]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
        lines.append(json.loads(out.strip().splitlines()[-1]))
        print(json.dumps(lines[-1]), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        shared = ("process", "elements", "variables", "excluded_variables", "replicas", "weight_decay", "steps",
                  "warmup", "timing")
        with open(args.record, "w") as f:
            for line in lines:
                for kind in line["kinds"]:
                    for run, x in enumerate(kind["runs_ms"]):
                        f.write(json.dumps({**{key: line[key] for key in shared}, "kind": kind["kind"], "run": run,
                                            "ms_per_clock": x}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
