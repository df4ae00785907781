#!/usr/bin/env python3
"""Time the replica step with layer-wise adaptive rates (cbx_set_adaptive_rate)
against the per-variable step, at ResNet-50's shape: its 161 variables as
bench.py registers them (n = 25,557,032), one GPU, 8 replicas, momentum 0.9,
weight decay 1e-4, the 106 batch-norm variables (the 1-D ones but for the FC
bias) excluded from the scaling and at multiplier 2, so that the step with the
feature off is the per-variable kernel.

The script starts one fresh process per measurement (`--processes`, default 4)
and, given `--parent-tree DIR` (a built checkout of the parent commit),
alternates the two trees: parent, this tree, parent, ...  A process of the
parent's tree runs this file against that tree's package and times what that
tree has, the per-variable step.  Per process, on one task stream, steps going
round the replicas, `--warmup` steps (50) of each kind first, then `--runs` (3)
runs of `--steps` (200) of each kind, the kinds alternating:

  per-variable step   cbx_replica_optimise, feature off        28 n bytes   events around each run
  adaptive path       cbx_replica_optimise, feature on         36 n bytes   events around each run
  pass, trust kernel, step, and their sum                                   each dispatch's own timestamps
                      cbx_sma_plan_optimise_adaptive_timed over the replicas' buffers, going round
                      them, with plain and with nontemporal loads in the pass, alternating

The parent's tree stamps no dispatch of the per-variable step, so the yardstick
(the parent's per-variable step in the same session) and the two whole-path
figures come from events around a run of back-to-back steps; the split of the
adaptive path comes from the dispatches themselves and leaves the gaps between
them out.  The byte counts predict 36/28 = 1.286 x the per-variable step for
the path and 8/28 of it for the pass.

Prints one JSON line per process and, with --record, writes every run of every
kind to FILE (default profiles/adaptive_rate/bench.jsonl), replacing it.

Usage: python scripts/bench_adaptive_rate.py [--parent-tree DIR] [--processes 4] [--record [FILE]]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS, STAMPS = "events around a run of back-to-back steps", "the dispatch's own timestamps, median of the run's steps"


def worker(args) -> int:
    """One process: the tree at args.root, one JSON line with every run of every kind."""
    sys.path.insert(0, args.root)
    import torch

    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd import build
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.variables import MODELS, register

    adaptive = hasattr(TheGPU, "set_adaptive_rate")
    g = TheGPU()
    g.init([0])
    try:
        shapes = MODELS["resnet50"]()
        n = register(g, shapes)
        bn = [k for k, s in enumerate(shapes) if len(s) == 1 and k != len(shapes) - 1]
        mults = [2.0 if k in set(bn) else 1.0 for k in range(len(shapes))]
        for k in bn:
            g.setModelVariableLearningRateMultiplier(k, 1, 2.0)
            if adaptive:
                g.set_model_variable_adaptive_rate(k, 1, False)
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(0.05)
        g.setModelManager(args.replicas, SYNC_BSP)
        g.set_variable_learning_rates(True)
        g.fill_synthetic(20260101)
        g.wait()
        R = args.replicas
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        task = [0]
        kinds = ["per-variable step", "adaptive path"] if adaptive else ["per-variable step"]

        def switch(kind):
            if adaptive:
                g.set_adaptive_rate(0.001 if kind == "adaptive path" else 0.0, 1e-9, 0)

        def steps(count):
            for _ in range(count):
                g.replica_optimise(task[0] % R, task[0], st)
                task[0] += 1

        def timed(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            steps(count)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / count

        for kind in kinds:
            switch(kind)
            steps(args.warmup)
        stream.synchronize()
        ms = {kind: [] for kind in kinds}
        for _ in range(args.runs):
            for kind in kinds:
                switch(kind)
                ms[kind].append(timed(args.steps))
        switch("per-variable step")
        g.wait()
        timing = {kind: EVENTS for kind in kinds}
        digest = {kind: build.code_object_digest() for kind in kinds}
        if adaptive:
            own = build.code_object_digest(build.ADAPTIVE_LIB)
            digest["adaptive path"] = own
            ptrs = [[g.replica_buffer(i, kind) for kind in (BUF_DATA, BUF_GRADIENT, BUF_LAST, BUF_DIFF)]
                    for i in range(R)]
            split = {0: [], 1: []}  # loads -> per run, the medians of (pass, trust kernel, step, sum)
            with SmaPlan([0], n) as plan:
                plan.set_variables([math.prod(s) for s in shapes], mults)
                plan.set_adaptive([k not in set(bn) for k in range(len(shapes))], slots=1)
                at = [0]

                def stamped(count, loads):
                    rows = []
                    for _ in range(count):
                        w, gr, last, s = ptrs[at[0] % R]
                        at[0] += 1
                        p, t, x = plan.optimise_adaptive_timed(0, 0, st, w, gr, last, s, 0.05, 0.9, 1e-4, 0.001, 1e-9, 0,
                                                               loads)
                        rows.append((p, t, x, p + t + x))
                    return [statistics.median(col) for col in zip(*rows)]

                for loads in (0, 1):
                    stamped(args.warmup, loads)
                for _ in range(args.runs):
                    for loads in (0, 1):
                        split[loads].append(stamped(args.steps, loads))
            names = {0: "plain loads", 1: "nontemporal loads"}
            for loads in (0, 1):
                for col, part in enumerate(("pass", "trust kernel", "step", "sum")):
                    kind = f"{part} ({names[loads]} in the pass)"
                    ms[kind] = [row[col] for row in split[loads]]
                    timing[kind], digest[kind] = STAMPS, own
        line = {"metric": "replica optimiser step, layer-wise adaptive rates against the per-variable step",
                "process": args.process, "tree": args.tree, "elements": n, "variables": len(shapes),
                "excluded_variables": len(bn), "replicas": R, "momentum": 0.9, "weight_decay": 1e-4,
                "steps": args.steps, "runs": args.runs, "warmup": args.warmup,
                "kinds": [{"kind": kind, "timing": timing[kind], "code_object_digest": digest[kind],
                           "median_ms": round(statistics.median(v), 5), "runs_ms": [round(x, 5) for x in v]}
                          for kind, v in ms.items()]}
        print(json.dumps(line))
    finally:
        g.free()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--processes", type=int, default=4)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, to alternate with")
    ap.add_argument("--record", nargs="?", default=None, metavar="FILE",
                    const=os.path.join(HERE, "profiles", "adaptive_rate", "bench.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="this tree", help=argparse.SUPPRESS)
    ap.add_argument("--process", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    lines = []
    for k in range(args.processes):
        parent = args.parent_tree is not None and k % 2 == 0
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--process", str(k + 1),
               "--root", os.path.abspath(args.parent_tree) if parent else HERE, "--tree", "parent" if parent else "this tree",
               "--replicas", str(args.replicas), "--steps", str(args.steps), "--runs", str(args.runs),
               "--warmup", str(args.warmup)]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
        lines.append(json.loads(out.strip().splitlines()[-1]))
        print(json.dumps(lines[-1]), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        shared = ("process", "tree", "elements", "variables", "excluded_variables", "replicas", "steps", "warmup")
        with open(args.record, "w") as f:
            for line in lines:
                for kind in line["kinds"]:
                    for run, x in enumerate(kind["runs_ms"]):
                        f.write(json.dumps({**{key: line[key] for key in shared}, "kind": kind["kind"], "run": run,
                                            "ms_per_step": x, "timing": kind["timing"],
                                            "code_object_digest": kind["code_object_digest"]}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
