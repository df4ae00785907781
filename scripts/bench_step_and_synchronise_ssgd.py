#!/usr/bin/env python3
"""The task steps fused into the one-GPU synchronous-SGD barrier
(cbx_step_and_synchronise_ssgd, cbx_ssgd_plan_step_and_optimise) against the
two-call sequence under update model WORKER, per clock, on one GPU.

One process, ResNet-50's element count, R replicas, base momentum 0.9, work per
clock R, at weight decay 0 and 1e-4 (a context each: the replicas take their
weight decay when they are made).  The forms alternate in batches of
back-to-back clocks, each batch timed as device time between two events:

  (a)  sequence        cbx_replica_optimise per replica in ascending id, then
                       cbx_synchronise           (16R + 24) n B, (24R + 24) n with weight decay
  (b)  fused           cbx_step_and_synchronise_ssgd
                                                 (8R + 24) n B,  (16R + 24) n with weight decay
  (c)  discard         the same with CBX_STEP_DISCARD_TASK_OUTPUTS, with weight
                       decay only (without it the flag selects (b)'s kernel)
                                                 (12R + 24) n B
  (d)  seam_fused      cbx_ssgd_plan_step_and_optimise over caller-owned buffers
  (e)  seam_discard    the same with the discard flag, with weight decay only
  yardstick, same process: the float4 copy ceiling.

Required (exit status 1 otherwise): the slowest batch of each of (b)-(e) is
below the fastest batch of (a) of the same weight decay; every value is finite
at the end; from one start over --digest-clocks clocks, z and every w_i of
(b)-(e) carry (a)'s digest.  Reported, not gating: each form's GB/s over its own
bytes beside the copy ceiling, and the speed-ups against the byte ratios.

--sweep times (b) at both weight decays and (c) at one and two float4s per lane
and at waves per CU -1 (auto), 0 (uncapped), 2, 3, 4, 6 and 8 through
cbx_set_task_barrier_kernel_config and prints one JSON line per shape before the
result line.

Usage: python scripts/bench_step_and_synchronise_ssgd.py [--replicas 8] [--steps 20] [--batches 5] [--sweep]
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, MOMENTUM = 0.05, 0.9
WDS = {"nowd": 0.0, "wd": 1e-4}
SEAM_FORMS = ("seam_fused", "seam_discard")


def forms_of(wd: float):
    return ("sequence", "fused", "seam_fused") + (("discard", "seam_discard") if wd > 0 else ())


def bytes_per_clock(form: str, wd: float, R: int, n: int) -> int:
    """Per element: a stepping replica reads g (and w with weight decay) and writes g where it is
    kept; the sequence also reads and writes the base gradient per replica; every replica is
    written once; the base model reads and writes acc, z and last."""
    if form == "sequence":
        return ((24 if wd > 0 else 16) * R + 24) * n
    if form.endswith("discard"):
        return (12 * R + 24) * n
    return ((16 if wd > 0 else 8) * R + 24) * n


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--digest-clocks", type=int, default=2)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()

    import torch

    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_WORKER, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import (CLIPPED_LIB, CLIPPED_VARIABLES_LIB, ELASTIC_STEPS_LIB, LIB, SSGD_STEPS_LIB,
                                    VARIABLES_LIB, code_object_digest)
    from crossbow_amd.seam import SmaPlan
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

    ctx, plan, n = {}, None, 0
    try:
        for key, wd in WDS.items():
            ctx[key], n = context(wd)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": {k: 0 for k in WDS}}

        # the seam's buffers: exactly n floats each, on a stream of the caller's
        plan = SmaPlan([0], n)
        dev_grad = torch.from_numpy(grad).cuda()
        sz, sl, sa = (torch.empty(n, device="cuda") for _ in range(3))
        sw = [torch.empty(n, device="cuda") for _ in range(R)]
        sg = [torch.empty(n, device="cuda") for _ in range(R)]
        seam_stream = torch.cuda.Stream()

        def start(c):
            c.fill_synthetic(20260101)
            for i in range(R):
                c.replica_write(i, BUF_GRADIENT, grad)
            c.base_write(0, BUF_GRADIENT, 0.0 * grad)
            c.wait()

        def seam_start(c):
            """The context's start, copied into the caller-owned buffers."""
            start(c)
            sz.copy_(torch.from_numpy(c.base_read(0, BUF_DATA)))
            sl.copy_(torch.from_numpy(c.base_read(0, BUF_LAST)))
            sa.zero_()
            for i in range(R):
                sw[i].copy_(torch.from_numpy(c.replica_read(i, BUF_DATA)))
                sg[i].copy_(dev_grad)
            torch.cuda.synchronize()

        def clock_iteration(key, form):
            g, wd = ctx[key], WDS[key]
            discard = STEP_DISCARD_TASK_OUTPUTS if form.endswith("discard") else 0
            if form in SEAM_FORMS:
                reps = [(0, sw[i].data_ptr(), sg[i].data_ptr(), 1, 1, LR) for i in range(R)]
                plan.ssgd_step_and_optimise([seam_stream.cuda_stream], [sz.data_ptr()], [sl.data_ptr()], [sa.data_ptr()],
                                            reps, MOMENTUM, wd, R, 0, discard)
                return
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"][key] += 1
            if form == "sequence":
                for i in range(R):  # ascending id: the order the fused call equals
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"][key], 0, False)
                g.unlockAny()
                return
            g.lockAny()
            g.step_and_synchronise_ssgd(0, state["clock"][key], 0, tasks, None, discard)
            g.unlockAny()

        def mark(key, form):
            """An event behind the end of the last step."""
            e = torch.cuda.Event(enable_timing=True)
            if form in SEAM_FORMS:
                e.record(seam_stream)
                return e
            if hip.hipStreamWaitEvent(side.cuda_stream, ctx[key].step_event(0), 0) != 0:
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

        def digest(key, form):
            h = hashlib.sha256()
            if form in SEAM_FORMS:
                for t in [sz] + sw:
                    h.update(t.cpu().numpy().tobytes())
                return h.hexdigest()
            h.update(ctx[key].base_read(0, BUF_DATA).tobytes())
            for i in range(R):
                h.update(ctx[key].replica_read(i, BUF_DATA).tobytes())
            return h.hexdigest()

        def digest_run(key, form):
            seam = form in SEAM_FORMS
            (seam_start if seam else start)(ctx[key])
            for _ in range(args.digest_clocks):
                for i in range(R):  # the kept forms leave g = fma(wd, w, g) behind: a fresh gradient per clock
                    if seam:
                        sg[i].copy_(dev_grad)
                    else:
                        ctx[key].replica_write(i, BUF_GRADIENT, grad)
                torch.cuda.synchronize()
                clock_iteration(key, form)
                ctx[key].wait()
                torch.cuda.synchronize()
            return digest(key, form)

        digests = {key: {f: digest_run(key, f) for f in forms_of(wd)} for key, wd in WDS.items()}

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        pairs = [(key, f) for key, wd in WDS.items() for f in forms_of(wd)]
        for key in WDS:
            start(ctx[key])
        seam_start(ctx["wd"])
        ms = {p: [] for p in pairs}
        for p in pairs:
            timed(*p, args.warmup)
        for _ in range(args.batches):
            for p in pairs:
                ms[p].append(timed(*p, args.steps))
        for c in ctx.values():
            c.wait()
        torch.cuda.synchronize()

        sweep, best = 0, None
        if args.sweep:
            for unroll in (1, 2):
                for waves in (-1, 0, 2, 3, 4, 6, 8):
                    row = {"sweep": "task_barrier_ssgd", "block": 64, "float4s_per_lane": unroll, "waves_per_cu": waves}
                    for key, f in (("nowd", "fused"), ("wd", "fused"), ("wd", "discard")):
                        ctx[key].set_task_barrier_kernel_config(64, unroll, waves)
                        timed(key, f, 3)
                        row[f"{key}_{f}_us"] = round(1e3 * timed(key, f, args.steps), 2)
                    print(json.dumps(row), flush=True)
                    if best is None or row["nowd_fused_us"] < best["nowd_fused_us"]:
                        best = row
                    sweep += 1
            for c in ctx.values():
                c.set_task_barrier_kernel_config(64, 1, -1)  # the default
        finite = bool(torch.isfinite(sz).all()) and all(bool(torch.isfinite(t).all()) for t in sw)
        for c in ctx.values():
            base, reps = c.modelStats(BUF_DATA)
            finite = finite and int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        copy_GBs = ctx["nowd"].bench_copy(4 * n, 20)

        line = {
            "metric": "task steps fused into the one-GPU synchronous-SGD barrier against the two-call sequence, per clock",
            "model": args.model, "elements": n, "replicas": R, "momentum": MOMENTUM, "work_per_clock": R,
            "weight_decay": WDS, "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "copy_ceiling_GBs": round(copy_GBs, 1), "finite_at_the_end": finite, "digest_clocks": args.digest_clocks,
        }
        ok = finite
        for key, wd in WDS.items():
            seq = ms[(key, "sequence")]
            seq_med, seq_bytes = statistics.median(seq), bytes_per_clock("sequence", wd, R, n)
            out = {"digests_equal_sequence": {f: digests[key][f] == digests[key]["sequence"]
                                              for f in forms_of(wd) if f != "sequence"}}
            for f in forms_of(wd):
                v, b = ms[(key, f)], bytes_per_clock(f, wd, R, n)
                med = statistics.median(v)
                out[f] = {"ms": round(med, 5), "batches_ms": [round(x, 5) for x in v], "spread": round(spread(v), 5),
                          "bytes_per_clock": b, "GBs_over_own_bytes": round(b / (med * 1e-3) / 1e9, 1)}
                if f == "sequence":
                    continue
                out[f].update({"speedup": round(seq_med / med, 4), "byte_ratio": round(seq_bytes / b, 4),
                               # the share of the predicted gain that is there: (speed-up - 1) / (byte ratio - 1)
                               "share_of_predicted_gain": round((seq_med / med - 1.0) / (seq_bytes / b - 1.0), 4),
                               "faster_in_every_batch": bool(max(v) < min(seq))})
                ok = ok and out[f]["faster_in_every_batch"] and out["digests_equal_sequence"][f]
            line[key] = out
        if best is not None:
            line["sweep_best"] = best
            line["sweep_best_over_default"] = round(best["nowd_fused_us"] / (1e3 * line["nowd"]["fused"]["ms"]), 5)
        line["pass"] = bool(ok)
        line["sweep_rows"] = sweep
        line["code_object_digest"] = code_object_digest(LIB)
        line["variables_code_object_digest"] = code_object_digest(VARIABLES_LIB)
        line["clipped_code_object_digest"] = code_object_digest(CLIPPED_LIB)
        line["clipped_variables_code_object_digest"] = code_object_digest(CLIPPED_VARIABLES_LIB)
        line["elastic_steps_code_object_digest"] = code_object_digest(ELASTIC_STEPS_LIB)
        line["ssgd_steps_code_object_digest"] = code_object_digest(SSGD_STEPS_LIB)
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        if plan is not None:
            plan.free()
        for c in ctx.values():
            c.free()


if __name__ == "__main__":
    sys.exit(main())
