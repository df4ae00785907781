#!/usr/bin/env python3
"""Time the replica step with gradient clipping by global norm against the
plain step, at the C3 shape: ResNet-50's variables as bench.py registers them
(n = 25,557,032), 8 replicas, one GPU, momentum 0.9, weight decay 1e-4.

In one process, on one task stream, after a warm-up of every kind: 5 batches
of 20 back-to-back steps of each kind, the batches of the kinds interleaved;
device time from events around each batch; steps go round the replicas.

  plain        cbx_replica_optimise, the feature off
  never        max_norm 1e30: norm pass (plain loads of g, the library's
               choice), reduce, CLIP step with scale 1
  always       max_norm 1e-6 on gradients whose norm stays far above it
               (the replicas' `last` is filled, so 0.9 * last keeps g large)
  never_nt     `never` with nontemporal loads of g in the norm pass
  skip         a gradient with one infinity, skip_nonfinite on (timed last,
               alternating with plain batches of its own)

The norm pass and the reduce alone come from their own dispatch timestamps
(cbx_sma_plan_gradient_norm going round the replicas' gradients, both kinds
of loads alternating); the copy ceiling is cbx_bench_copy in the same process.

The yardstick is the plain step in the same process.  The clipped step reads
4 n more bytes than the plain step's 28 n, so its budget is
plain_ms * (1 + 4 / 28) + reduce_ms, with the plain step's own batch spread
plus 0.01 as the margin: `pass` says never_ms / budget_ms <= gate.

Prints one JSON line.
Usage: python scripts/bench_gradient_clip.py [--replicas 8] [--steps 20] [--batches 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--norm-samples", type=int, default=10)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    args = ap.parse_args()

    import numpy as np
    import torch

    from crossbow_amd import BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd.build import code_object_digest
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    g = TheGPU()
    g.init([0])
    try:
        n = register(g, MODELS[args.model]())
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(0.05)
        g.setModelManager(args.replicas, SYNC_BSP)
        g.fill_synthetic(20260101)
        R = args.replicas
        grad = O.fill_normal(n, 77, 0.01)
        for i in range(R):
            g.replica_write(i, BUF_GRADIENT, grad)
            g.replica_write(i, BUF_LAST, grad)
        g.wait()
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        task = [0]

        def run(count):
            for _ in range(count):
                g.replica_optimise(task[0] % R, task[0], st)
                task[0] += 1

        def timed(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            run(count)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / count

        def kind(name):
            os.environ["CBX_CLIP_NORM_LOADS"] = "nontemporal" if name == "never_nt" else "temporal"
            if name == "plain":
                g.set_gradient_clip(0.0, False)
            elif name in ("never", "never_nt"):
                g.set_gradient_clip(1e30, False)
            elif name == "always":
                g.set_gradient_clip(1e-6, False)
            else:
                g.set_gradient_clip(0.0, True)

        def counts():
            recs = [g.replica_clip_stats(i) for i in range(R)]
            return {k: sum(r[k] for r in recs) for k in ("steps", "clipped_steps", "skipped_steps")}

        kinds = ("plain", "never", "always", "never_nt")
        for k in kinds:
            kind(k)
            run(args.warmup)
        stream.synchronize()
        ms = {k: [] for k in kinds + ("skip", "plain2")}
        seen = {k: {"steps": 0, "clipped_steps": 0, "skipped_steps": 0} for k in kinds + ("skip",)}
        for _ in range(args.batches):
            for k in kinds:
                kind(k)
                before = counts()
                ms[k].append(timed(args.steps))
                after = counts()
                for f in before:
                    seen[k][f] += after[f] - before[f]
        # the skip path: one infinity in every replica's gradient; a skipped
        # step does not write g, and the plain step keeps an infinity infinite
        grad[0] = np.inf
        for i in range(R):
            g.replica_write(i, BUF_GRADIENT, grad)
        for k in ("skip", "plain"):
            kind(k)
            run(args.warmup)
        for _ in range(args.batches):
            kind("skip")
            before = counts()
            ms["skip"].append(timed(args.steps))
            after = counts()
            for f in before:
                seen["skip"][f] += after[f] - before[f]
            kind("plain")
            ms["plain2"].append(timed(args.steps))
        g.wait()

        # the two launches alone, and the copy ceiling
        # (going round the replicas' gradients, 8 x 102 MB, so that no pass
        # finds its input in the 256 MiB Infinity Cache)
        gptrs = [g.replica_buffer(i, BUF_GRADIENT) for i in range(R)]
        norm = {0: [], 1: []}
        red = []
        with SmaPlan([0], n) as plan:
            for loads in (0, 1):
                plan.gradient_norm(0, 0, st, gptrs[loads % R], 1e30, False, loads)
            for k in range(args.norm_samples):
                for loads in (0, 1):
                    _, p_ms, r_ms = plan.gradient_norm(0, 0, st, gptrs[(2 * k + loads + 2) % R], 1e30, False, loads)
                    norm[loads].append(p_ms)
                    red.append(r_ms)
        copy_GBs = g.bench_copy(4 * n, 20)

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        med = {k: statistics.median(v) for k, v in ms.items()}
        reduce_ms = statistics.median(red)
        budget = med["plain"] * (1 + 4 / 28) + reduce_ms
        gate = 1.0 + spread(ms["plain"]) + 0.01
        pass_nt, pass_t = statistics.median(norm[1]), statistics.median(norm[0])
        line = {
            "metric": "replica optimiser step with gradient clipping by global norm against the plain step",
            "model": args.model, "elements": n, "replicas": R, "momentum": 0.9, "weight_decay": 1e-4,
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "plain_ms": round(med["plain"], 5), "plain_batches_ms": [round(x, 5) for x in ms["plain"]],
            "plain_spread": round(spread(ms["plain"]), 5),
            "never_clips_ms": round(med["never"], 5), "never_clips_batches_ms": [round(x, 5) for x in ms["never"]],
            "always_clips_ms": round(med["always"], 5), "always_clips_batches_ms": [round(x, 5) for x in ms["always"]],
            "never_clips_nontemporal_norm_loads_ms": round(med["never_nt"], 5),
            "never_clips_nontemporal_norm_loads_batches_ms": [round(x, 5) for x in ms["never_nt"]],
            "skip_ms": round(med["skip"], 5), "skip_batches_ms": [round(x, 5) for x in ms["skip"]],
            "plain_beside_skip_ms": round(med["plain2"], 5),
            "counts": seen,
            "norm_pass_nontemporal_ms": round(pass_nt, 5), "norm_pass_temporal_ms": round(pass_t, 5),
            "reduce_ms": round(reduce_ms, 5), "tiles": (n + 4095) // 4096,
            "copy_ceiling_GBs": round(copy_GBs, 1),
            "norm_pass_nontemporal_GBs": round(4 * n / (pass_nt * 1e-3) / 1e9, 1),
            "norm_pass_temporal_GBs": round(4 * n / (pass_t * 1e-3) / 1e9, 1),
            "norm_pass_nontemporal_fraction_of_copy": round(4 * n / (pass_nt * 1e-3) / 1e9 / copy_GBs, 3),
            "norm_pass_temporal_fraction_of_copy": round(4 * n / (pass_t * 1e-3) / 1e9 / copy_GBs, 3),
            "budget_ms": round(budget, 5), "ratio_to_budget": round(med["never"] / budget, 5),
            "always_ratio_to_budget": round(med["always"] / budget, 5),
            "ratio_to_plain": round(med["never"] / med["plain"], 5),
            "gate": round(gate, 5), "pass": bool(med["never"] / budget <= gate),
            "bytes_per_plain_step": 28 * n, "bytes_per_clipped_step": 32 * n,
            "plain_GBs": round(28 * n / (med["plain"] * 1e-3) / 1e9, 1),
            "never_clips_GBs": round(32 * n / (med["never"] * 1e-3) / 1e9, 1),
            "code_object_digest": code_object_digest(),
        }
        print(json.dumps(line))
    finally:
        g.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
