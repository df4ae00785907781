#!/usr/bin/env python3
"""Time one clock with layer-wise adaptive rates (cbx_set_adaptive_rate) under elastic averaging (update model
3, cbx_set_elastic_average) three ways at ResNet-50's shape: its 161 variables as bench.py registers them
(n = 25,557,032), one GPU, 8 replicas, momentum 0.9, weight decay 1e-4, the batch-norm variables excluded from
the scaling and at multiplier 2.

  sequence   8 x cbx_replica_optimise + cbx_synchronise               (44R + 8) n bytes, 3R + 1 launches
  fused      cbx_step_and_synchronise_elastic_adaptive, flags 0       (36R + 8) n bytes, 3 launches
  discard    the same with CBX_STEP_DISCARD_TASK_OUTPUTS              (28R + 8) n bytes

Every clock runs on the sync stream.  The script starts one fresh process per measurement (`--processes`,
default 2).  Per process: `--warmup` clocks of each kind, then `--runs` (3) runs of `--steps` back-to-back
clocks of each kind, the kinds alternating, each run between two events that wait for the step event.  The
sequence's kernels live in objects that the fused call's object does not touch, so it is the yardstick, timed
in the same process.  The byte model predicts 360/296 = 1.22 x (fused) and 360/232 = 1.55 x (discard).

Prints one JSON line per process and, with --record, writes every run of every kind to FILE (default
profiles/elastic_adaptive_steps/bench.jsonl), replacing it.

Usage: python scripts/bench_elastic_adaptive_steps.py [--processes 2] [--record [FILE]]
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
KINDS = ("sequence", "fused", "discard")


def worker(args) -> int:
    import torch

    from crossbow_amd import BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SYNCHRONOUSEAMSGD, TheGPU, build
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
            g.setModelVariableLearningRateMultiplier(k, 1, 2.0)
            g.set_model_variable_adaptive_rate(k, 1, False)
        g.setUpdateModelType(UPDATE_SYNCHRONOUSEAMSGD)
        g.setElasticAverage(True)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(0.05)
        R = args.replicas
        g.setModelManager(R, SYNC_BSP)
        g.set_variable_learning_rates(True)
        g.set_adaptive_rate(0.001, 1e-9, 0)
        g.fill_synthetic(20260101)
        grad = O.fill_normal(n, 77, 0.01)
        for i in range(R):
            g.replica_write(i, BUF_GRADIENT, grad)
            g.replica_write(i, BUF_LAST, grad)
        g.wait()
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0}

        def clock(kind):
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"] += 1
            if kind == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
            else:
                g.lockAny()
                g.step_and_synchronise_elastic_adaptive(0, state["clock"], 0, tasks, None,
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
            a = mark()
            for _ in range(count):
                clock(kind)
            b = mark()
            b.synchronize()
            return a.elapsed_time(b) / count

        for kind in KINDS:
            for _ in range(args.warmup):
                clock(kind)
        g.wait()
        ms = {kind: [] for kind in KINDS}
        for _ in range(args.runs):
            for kind in KINDS:
                ms[kind].append(timed(kind, args.steps))
        g.wait()
        med = {kind: statistics.median(v) for kind, v in ms.items()}
        spread = {kind: max(v) - min(v) for kind, v in ms.items()}
        line = {"metric": "one elastic-averaging clock with layer-wise adaptive rates: the two-call sequence against the fused call",
                "process": args.process, "elements": n, "variables": len(shapes), "excluded_variables": len(bn),
                "replicas": R, "momentum": 0.9, "weight_decay": 1e-4, "steps": args.steps, "runs": args.runs,
                "warmup": args.warmup, "timing": "events around a run of back-to-back clocks",
                "code_object_digest": {"sequence": build.code_object_digest(build.ADAPTIVE_LIB),
                                       "fused": build.code_object_digest(build.ELASTIC_ADAPTIVE_LIB)},
                "kinds": [{"kind": kind, "median_ms": round(med[kind], 5), "spread_ms": round(spread[kind], 5),
                           "runs_ms": [round(x, 5) for x in ms[kind]],
                           "speedup_over_sequence": round(med["sequence"] / med[kind], 4)} for kind in KINDS],
                "gate_both_fused_forms_beat_the_sequence_by_more_than_the_spread": all(
                    med["sequence"] - med[kind] > max(spread["sequence"], spread[kind]) for kind in KINDS[1:])}
        print(json.dumps(line))
    finally:
        g.free()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--record", nargs="?", default=None, metavar="FILE",
                    const=os.path.join(HERE, "profiles", "elastic_adaptive_steps", "bench.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--process", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    for k in range(args.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--process", str(k + 1), "--replicas",
               str(args.replicas), "--steps", str(args.steps), "--runs", str(args.runs), "--warmup", str(args.warmup)]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
        lines.append(json.loads(out.strip().splitlines()[-1]))
        print(json.dumps(lines[-1]), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        shared = ("process", "elements", "variables", "excluded_variables", "replicas", "steps", "warmup", "timing")
        with open(args.record, "w") as f:
            for line in lines:
                for kind in line["kinds"]:
                    for run, x in enumerate(kind["runs_ms"]):
                        f.write(json.dumps({**{key: line[key] for key in shared}, "kind": kind["kind"], "run": run,
                                            "ms_per_clock": x}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
