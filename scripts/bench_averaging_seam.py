#!/usr/bin/env python3
"""Time the three fused model-averaging barriers through BOTH doors in one
process on one GPU: the context (cbx_synchronise over the library's padded
arena) and the sma.c seam (cbx_sma_plan_step, cbx_ea_plan_step,
cbx_pr_plan_step over separately allocated, unpadded buffers), on ResNet-50's
parameters (n = 25,557,032: a scalar tail of 40 elements) with R = 8 replicas.

Protocol of scripts/bench_averaging.py: per step and door, `--warmup` untimed
steps, then `--repeats` runs of `--steps` back-to-back steps; the figure is the
median step of each run, from the dispatches' own timestamps (the context's
cbx_timing_history, the plan's cbx_sma_plan_timing_history: each fused step is
one kernel whose dispatch stamps its own start and stop).

The yardstick is the SMA seam's gap over the SMA context in the same run: the
gap of a new seam step over its own context step is reported beside it, with
the spread of the runs.  The seam's tail rides the bulk launch on extra
workgroups (`tail_form`).  One JSON line on stdout.
Usage: python3 scripts/bench_averaging_seam.py [--steps 200] [--warmup 50] [--repeats 3] [--replicas 8]
                                               [--momentum 0.9]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_averaging as BA  # noqa: E402

ALPHA = 0.1
TAIL_QUANTUM = 1024  # floats: the seam's float4 bulk is whole 256-float4 chunks (kTailQuantum4)


def context_runs(model, R, momentum, args):
    from crossbow_amd._lib import T_KERNEL
    g, n = BA.make(model, R, momentum)
    try:
        g.set_timing(True)
        clock = BA.run_steps(g, args.warmup, 0)
        medians = []
        for _ in range(args.repeats):
            clock = BA.run_steps(g, args.steps, clock)
            t = g.timing_history(T_KERNEL, 0, args.steps)
            assert t.size == args.steps and np.all(t > 0), "a step kept no kernel time"
            medians.append(float(np.median(t)) * 1e3)
        return n, medians
    finally:
        g.free()


def seam_runs(model, n, R, momentum, args):
    """The caller's side: one allocation per buffer, exactly n floats each,
    filled as cbx_fill_synthetic fills the context's."""
    import torch

    from crossbow_amd.seam import SmaPlan
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    z = torch.randn(n, device=dev, generator=gen) * 0.05
    last = torch.randn(n, device=dev, generator=gen) * 0.001 if momentum > 0 else None
    s = [z + 0.01 * torch.randn(n, device=dev, generator=gen) for _ in range(R)]
    w = [si + 0.001 * torch.randn(n, device=dev, generator=gen) for si in s]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    streams, zp = [stream.cuda_stream], [z.data_ptr()]
    lp = [last.data_ptr()] if last is not None else None
    sma = [(0, w[i].data_ptr(), s[i].data_ptr(), 1, 0) for i in range(R)]
    ea = [(0, w[i].data_ptr(), None, 1) for i in range(R)]
    pr = [(0, w[i].data_ptr(), 1, 0) for i in range(R)]
    clock = 0

    with SmaPlan([0], n) as plan:
        def run(count):
            nonlocal clock
            for _ in range(count):
                if model == "sma":
                    plan.step(streams, zp, lp, sma, ALPHA, momentum)
                elif model == "elastic":
                    plan.elastic_step(streams, zp, ea, ALPHA)
                else:
                    plan.polyak_step(streams, zp, lp, pr, ALPHA, clock)
                clock += 1
            stream.synchronize()
        plan.set_timing(True)
        run(args.warmup)
        medians = []
        for _ in range(args.repeats):
            run(args.steps)
            t = np.asarray(plan.timing_history(args.steps))
            assert t.size == args.steps and np.all(t > 0), "a step kept no kernel time"
            medians.append(float(np.median(t)) * 1e3)
    del z, last, s, w
    torch.cuda.empty_cache()
    return medians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--momentum", type=float, default=0.9)
    args = ap.parse_args()
    if args.steps > 256:
        ap.error("the plan keeps the last 256 timed steps")
    R = args.replicas
    out = {"replicas": R, "momentum": args.momentum, "steps": args.steps, "warmup": args.warmup,
           "tail_form": "same launch", "models": {}}
    for model in ("sma", "elastic", "polyak"):
        n, ctx = context_runs(model, R, args.momentum, args)
        seam = seam_runs(model, n, R, args.momentum, args)
        c, s = float(np.median(ctx)), float(np.median(seam))
        out["n"] = n
        out["tail_elements"] = n - n // TAIL_QUANTUM * TAIL_QUANTUM
        out["models"][model] = {
            "context_us_runs": [round(x, 2) for x in ctx], "seam_us_runs": [round(x, 2) for x in seam],
            "context_us": round(c, 2), "seam_us": round(s, 2), "gap_us": round(s - c, 2),
            "gap_pct": round(100.0 * (s - c) / c, 3),
            "spread_us": round(max(max(ctx) - min(ctx), max(seam) - min(seam)), 2)}
    m = out["models"]
    for model in ("elastic", "polyak"):
        # the allowance: SMA's gap in this run plus the spread of the runs involved
        allow = m["sma"]["gap_us"] + max(m["sma"]["spread_us"], m[model]["spread_us"])
        m[model]["gap_over_allowance_us"] = round(max(0.0, m[model]["gap_us"] - allow), 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
