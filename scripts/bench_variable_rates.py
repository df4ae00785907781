#!/usr/bin/env python3
"""Time the replica step with per-variable learning rates against the plain
step, at the C3 shape: ResNet-50's variables as bench.py registers them
(n = 25,557,032, 161 variables), 8 replicas, one GPU, momentum 0.9, weight
decay 1e-4.  Batch-norm variables (gamma, beta) get multiplier 2, the rest 1.

In one process, on one task stream, after a warm-up of both: 5 batches of 20
back-to-back steps of each kind, the batches of the two kinds interleaved;
device time from events around each batch; steps go round the replicas.  The
plain step is cbx_replica_optimise with cbx_set_variable_learning_rates off
(sma_optimise_kernel), the per-variable step the same call with it on
(sma_optimise_variables_kernel).  The per-operator form
(cbx_replica_optimise_variables, 161 calls per task on the same stream) is
timed the same way over 5 batches of 4 tasks; it is launch-bound.

Prints one JSON line:

  plain_ms / variables_ms      median over the 5 batches of (batch time / 20)
  *_spread                     (max - min) / median over the 5 batches
  ratio                        variables_ms / plain_ms
  gate                         1 + plain_spread + 0.01; `pass`: ratio <= gate
  *_GBs                        (20 + 8 m) n bytes over the median, m = 1
  per_operator_ms_per_task     161 launches, median over its batches
  mixed_chunks / chunks        table entries with a variable boundary inside

Usage: python scripts/bench_variable_rates.py [--replicas 8] [--steps 20] [--batches 5]
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
    ap.add_argument("--operator-tasks", type=int, default=4)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    args = ap.parse_args()

    import torch

    from crossbow_amd import SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd.build import code_object_digest
    from crossbow_amd.variables import MODELS, register

    g = TheGPU()
    g.init([0])
    try:
        shapes = MODELS[args.model]()
        n = register(g, shapes)
        # batch-norm gamma / beta: the 1-D variables, but for the last (the FC bias)
        bn = [k for k, s in enumerate(shapes) if len(s) == 1 and k != len(shapes) - 1]
        for k in bn:
            g.setModelVariableLearningRateMultiplier(k, 1, 2.0)
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(0.05)
        g.setModelManager(args.replicas, SYNC_BSP)
        g.fill_synthetic(20260101)
        g.wait()
        R = args.replicas
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        task = [0]

        def whole(count):
            for _ in range(count):
                g.replica_optimise(task[0] % R, task[0], st)
                task[0] += 1

        def per_operator(count):
            for _ in range(count):
                for op in range(len(shapes)):
                    g.replica_optimise_variables(task[0] % R, task[0], op, st)
                task[0] += 1

        def timed(fn, count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn(count)
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / count

        for on in (False, True):
            g.set_variable_learning_rates(on)
            whole(args.warmup)
        per_operator(1)
        stream.synchronize()
        ms = {False: [], True: []}
        for _ in range(args.batches):
            for on in (False, True):
                g.set_variable_learning_rates(on)
                ms[on].append(timed(whole, args.steps))
        op_ms = [timed(per_operator, args.operator_tasks) for _ in range(args.batches)]
        g.wait()

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        plain, var = statistics.median(ms[False]), statistics.median(ms[True])
        nbytes = (20 + 8 * 1) * n
        chunks = (n + 255) // 256
        bounds, at = set(), 0
        for s in shapes[:-1]:
            e = 1
            for d in s:
                e *= d
            at += e
            if at % 256:
                bounds.add(at // 256)
        gate = 1.0 + spread(ms[False]) + 0.01
        line = {
            "metric": "replica optimiser step, per-variable learning rates against the plain step",
            "model": args.model, "elements": n, "variables": len(shapes), "replicas": R,
            "multiplier_2_variables": len(bn), "momentum": 0.9, "weight_decay": 1e-4,
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "plain_ms": round(plain, 5), "plain_batches_ms": [round(x, 5) for x in ms[False]],
            "plain_spread": round(spread(ms[False]), 5),
            "variables_ms": round(var, 5), "variables_batches_ms": [round(x, 5) for x in ms[True]],
            "variables_spread": round(spread(ms[True]), 5),
            "ratio": round(var / plain, 5), "gate": round(gate, 5), "pass": bool(var / plain <= gate),
            "bytes_per_step": nbytes,
            "plain_GBs": round(nbytes / (plain * 1e-3) / 1e9, 1),
            "variables_GBs": round(nbytes / (var * 1e-3) / 1e9, 1),
            "per_operator_ms_per_task": round(statistics.median(op_ms), 5),
            "per_operator_batches_ms": [round(x, 5) for x in op_ms],
            "per_operator_launches_per_task": len(shapes), "per_operator_tasks_per_batch": args.operator_tasks,
            "chunks": chunks, "mixed_chunks": len(bounds),
            "code_object_digest": code_object_digest(),
        }
        print(json.dumps(line))
    finally:
        g.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
