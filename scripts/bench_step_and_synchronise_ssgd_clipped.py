#!/usr/bin/env python3
"""Synchronous SGD with gradient clipping, per clock, on one GPU: the fused call
(cbx_step_and_synchronise_ssgd_clipped) against its two-call sequence and
against the unclipped fused call.

One process, ResNet-50's element count, R replicas all stepping and none
skipped, base momentum 0.9, work per clock R, at weight decay 0 and 1e-4.  Per
weight decay one context clips (max_norm far below the gradient's norm, so the
scale is not 1) and one does not.  The forms alternate in batches of
back-to-back clocks, each batch timed as device time between two events:

  fused              cbx_step_and_synchronise_ssgd_clipped       (12R + 24) n B + 4R n, (16R + 24) n + 4R n with weight decay
  discard            the same with CBX_STEP_DISCARD_TASK_OUTPUTS ( 8R + 24) n B + 4R n, (12R + 24) n + 4R n
  sequence           R x cbx_replica_accumulate_clipped, then cbx_synchronise
                                                                 (16R + 24) n B + 4R n, (20R + 24) n + 4R n
  unclipped          cbx_step_and_synchronise_ssgd               ( 8R + 24) n B,        (16R + 24) n
  unclipped_discard  the same with the discard flag              ( 8R + 24) n B,        (12R + 24) n
  norm passes alone: R x (norm pass + reduce) over one gradient, from the two
  dispatches' own timestamps (cbx_sma_plan_gradient_norm).

Reported, nothing gating: fused against sequence beside the ratio of their byte
counts, and fused against unclipped beside the norm passes' own time.

--unclipped-only times the two unclipped forms alone, twice over (``_again``):
the run that works on a tree without the clipped calls, and whose two halves
show the run-to-run spread of one tree.

Usage: python scripts/bench_step_and_synchronise_ssgd_clipped.py [--replicas 8] [--steps 20] [--batches 5]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, MOMENTUM = 0.05, 0.9
WDS = {"nowd": 0.0, "wd": 1e-4}
CLIPPED_FORMS = ("fused", "discard", "sequence")


def bytes_per_clock(form: str, wd: float, R: int, n: int) -> int:
    """Per element: a stepping replica reads g (and w with weight decay) and writes g where it is
    kept, which the clipped step does with or without weight decay; the sequence also reads and
    writes the base gradient per replica; every replica is written once; the base model reads and
    writes acc, z and last; a clipped form's norm passes read every g once more."""
    w = 4 if wd > 0 else 0
    if form == "sequence":
        return ((16 + w) * R + 24 + 4 * R) * n
    if form == "fused":
        return ((12 + w) * R + 24 + 4 * R) * n
    if form == "discard":
        return ((8 + w) * R + 24 + 4 * R) * n
    if form == "unclipped":
        return ((8 + 2 * w) * R + 24) * n
    return ((8 + w) * R + 24) * n  # unclipped_discard


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    ap.add_argument("--unclipped-only", action="store_true")
    args = ap.parse_args()

    import torch

    from crossbow_amd import BUF_DATA, BUF_GRADIENT, SYNC_BSP, UPDATE_WORKER, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import LIB, SSGD_STEPS_LIB, code_object_digest
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int

    shapes = MODELS[args.model]()
    R = args.replicas

    def context(wd):
        c = TheGPU()
        c.init([0])
        n_ = register(c, shapes)
        c.setModelWorkPerClock(R)
        c.setUpdateModelType(UPDATE_WORKER)
        c.setMomentum(MOMENTUM, 0)
        c.setWeightDecay(wd)
        c.setLearningRateDecayPolicyFixed(LR)
        c.setModelManager(R, SYNC_BSP)
        return c, n_

    forms = ("unclipped", "unclipped_discard")
    forms = forms + tuple(f + "_again" for f in forms) if args.unclipped_only else CLIPPED_FORMS + forms
    ctx, plan, n = {}, None, 0
    try:
        for key, wd in WDS.items():
            ctx[key, False], n = context(wd)
            if not args.unclipped_only:
                ctx[key, True], n = context(wd)
        grad = O.fill_normal(n, 77, 0.01)
        norm = float(torch.from_numpy(grad).double().norm())
        for (key, clip), c in ctx.items():
            if clip:
                c.set_gradient_clip(0.25 * norm, True)
            c.fill_synthetic(20260101)
            for i in range(R):
                c.replica_write(i, BUF_GRADIENT, grad)
            c.base_write(0, BUF_GRADIENT, 0.0 * grad)
            c.wait()
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": {k: 0 for k in ctx}}

        def clock_iteration(key, form):
            which = (key, form in CLIPPED_FORMS)
            g = ctx[which]
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"][which] += 1
            clock = state["clock"][which]
            discard = STEP_DISCARD_TASK_OUTPUTS if "discard" in form else 0
            if form == "sequence":
                for i in range(R):  # ascending id: the order the fused call equals
                    g.replica_accumulate_clipped(i, tasks[i])
                g.lockAny()
                g.synchronise(0, clock, 0, False)
                g.unlockAny()
                return
            g.lockAny()
            if form in CLIPPED_FORMS:
                g.step_and_synchronise_ssgd_clipped(0, clock, 0, tasks, None, discard)
            else:
                g.step_and_synchronise_ssgd(0, clock, 0, tasks, None, discard)
            g.unlockAny()

        def mark(key, form):
            """An event behind the end of the last step."""
            e = torch.cuda.Event(enable_timing=True)
            if hip.hipStreamWaitEvent(side.cuda_stream, ctx[key, form in CLIPPED_FORMS].step_event(0), 0) != 0:
                raise RuntimeError("hipStreamWaitEvent failed")
            e.record(side)
            return e

        def timed(key, form, count):
            a = mark(key, form)
            for _ in range(count):
                clock_iteration(key, form)
            b = mark(key, form)
            b.synchronize()
            return a.elapsed_time(b) / count

        pairs = [(key, f) for key in WDS for f in forms]
        ms = {p: [] for p in pairs}
        for p in pairs:
            timed(*p, args.warmup)
        for _ in range(args.batches):
            for p in pairs:
                ms[p].append(timed(*p, args.steps))
        for c in ctx.values():
            c.wait()
        torch.cuda.synchronize()

        finite = True
        for c in ctx.values():
            base, reps = c.modelStats(BUF_DATA)
            finite = finite and int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        line = {
            "metric": "synchronous SGD with gradient clipping: the fused call, its two-call sequence and the "
                      "unclipped fused call, per clock",
            "model": args.model, "elements": n, "replicas": R, "momentum": MOMENTUM, "work_per_clock": R,
            "weight_decay": WDS, "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "copy_ceiling_GBs": round(ctx["nowd", False].bench_copy(4 * n, 20), 1), "finite_at_the_end": finite,
        }
        if not args.unclipped_only:
            from crossbow_amd.build import SSGD_CLIPPED_LIB
            from crossbow_amd.seam import SmaPlan
            plan = SmaPlan([0], n)
            dev_grad = torch.from_numpy(grad).cuda()
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            passes = [plan.gradient_norm(0, 0, stream.cuda_stream, dev_grad.data_ptr(), 0.25 * norm, True)[1:]
                      for _ in range(3 + args.batches)][3:]
            line["norm_pass_ms"] = round(statistics.median(p for p, _ in passes), 5)
            line["norm_reduce_ms"] = round(statistics.median(r for _, r in passes), 5)
            line["norm_passes_ms_per_clock"] = round(R * (line["norm_pass_ms"] + line["norm_reduce_ms"]), 5)
            line["ssgd_clipped_code_object_digest"] = code_object_digest(SSGD_CLIPPED_LIB)
        for key, wd in WDS.items():
            out = {}
            for f in forms:
                v, b = ms[key, f], bytes_per_clock(f.replace("_again", ""), wd, R, n)
                med = statistics.median(v)
                out[f] = {"ms": round(med, 5), "batches_ms": [round(x, 5) for x in v],
                          "spread": round((max(v) - min(v)) / med, 5), "bytes_per_clock": b,
                          "GBs_over_own_bytes": round(b / (med * 1e-3) / 1e9, 1)}
            if not args.unclipped_only:
                for f, other in (("fused", "unclipped"), ("discard", "unclipped_discard")):
                    out[f]["speedup_over_sequence"] = round(out["sequence"]["ms"] / out[f]["ms"], 4)
                    out[f]["byte_ratio_to_sequence"] = round(out["sequence"]["bytes_per_clock"] / out[f]["bytes_per_clock"], 4)
                    out[f]["ms_over_" + other] = round(out[f]["ms"] - out[other]["ms"], 5)
            line[key] = out
        line["code_object_digest"] = code_object_digest(LIB)
        line["ssgd_steps_code_object_digest"] = code_object_digest(SSGD_STEPS_LIB)
        print(json.dumps(line))
        return 0 if finite else 1
    finally:
        if plan is not None:
            plan.free()
        for c in ctx.values():
            c.free()


if __name__ == "__main__":
    sys.exit(main())
