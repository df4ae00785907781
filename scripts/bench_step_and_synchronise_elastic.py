#!/usr/bin/env python3
"""The task steps fused into the one-GPU elastic-averaging barrier
(cbx_step_and_synchronise_elastic, cbx_ea_plan_step_and_optimise) against the
two-call sequence under elastic averaging, per clock, on one GPU.

One process, ResNet-50's element count, R replicas, alpha 0.1, momentum 0.9,
weight decay 1e-4.  The forms alternate in batches of back-to-back clocks, each
batch timed as device time between two events:

  (a)  sequence        cbx_replica_optimise per replica, then cbx_synchronise
                       (update model 3 with elastic averaging)   (36R + 8) n B
  (b)  fused           cbx_step_and_synchronise_elastic          (28R + 8) n B
  (c)  discard         the same with CBX_STEP_DISCARD_TASK_OUTPUTS
                                                                  (20R + 8) n B
  (d)  seam_fused      cbx_ea_plan_step_and_optimise over caller-owned buffers
  (e)  seam_discard    the same with the discard flag
  yardsticks, same process: cbx_step_and_synchronise under SMA on a second
  context ((28R + 16) n B), and the float4 copy ceiling.

Required (exit status 1 otherwise): the slowest batch of each of (b)-(e) is
below the fastest batch of (a); every value is finite at the end; from one
start over --digest-clocks clocks, z and every w_i of (b)-(e) carry (a)'s
digest.  Reported, not gating: each form's GB/s over its own bytes beside the
yardstick's, and the speed-ups against the byte ratios (36R + 8) / (28R + 8)
and (36R + 8) / (20R + 8).

--sweep times (b) and (c) at unroll 1 and 2 and at waves per CU -1 (auto), 0
(uncapped), 2, 3, 4 and 8 through cbx_set_task_barrier_kernel_config and
prints one JSON line per shape before the result line.  The automatic cap's
stream target is not swept apart from that: at R = 8 the SMA kernels' 56 and
the averaging kernels' 76 both resolve to 2 waves per CU for (b) (58 streams)
and for (c) (42 streams), the row "waves_per_cu": -1.

Usage: python scripts/bench_step_and_synchronise_elastic.py [--replicas 8] [--steps 20] [--batches 5] [--sweep]
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

CONTEXT_FORMS = ("sequence", "fused", "discard")
SEAM_FORMS = ("seam_fused", "seam_discard")
NEW_FORMS = ("fused", "discard") + SEAM_FORMS
FORMS = CONTEXT_FORMS + SEAM_FORMS + ("sma_fused",)  # the last: the yardstick on a context of its own
LR, ALPHA, MOMENTUM, WD = 0.05, 0.1, 0.9, 1e-4


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

    from crossbow_amd import (BUF_DATA, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, UPDATE_SYNCHRONOUSEAMSGD,
                              TheGPU)
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import (CLIPPED_LIB, CLIPPED_VARIABLES_LIB, ELASTIC_STEPS_LIB, LIB, VARIABLES_LIB,
                                    code_object_digest)
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int

    shapes = MODELS[args.model]()
    R = args.replicas

    def context(update_type, elastic):
        c = TheGPU()
        c.init([0])
        n_ = register(c, shapes)
        c.setUpdateModelType(update_type)
        if elastic:
            c.setElasticAverage(True)
        c.setEamsgdAlpha(ALPHA)
        c.setMomentum(MOMENTUM, 0)
        c.setWeightDecay(WD)
        c.setLearningRateDecayPolicyFixed(LR)
        c.setModelManager(R, SYNC_BSP)
        return c, n_

    g, n = context(UPDATE_SYNCHRONOUSEAMSGD, True)
    sma, plan = None, None
    try:
        sma, _ = context(UPDATE_SMA, False)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0, "sma_clock": 0}

        # the seam's buffers: exactly n floats each, on a stream of the caller's
        plan = SmaPlan([0], n)
        dev_grad = torch.from_numpy(grad).cuda()
        sz = torch.empty(n, device="cuda")
        sw = [torch.empty(n, device="cuda") for _ in range(R)]
        ss = [torch.empty(n, device="cuda") for _ in range(R)]
        sg = [torch.empty(n, device="cuda") for _ in range(R)]
        sl = [torch.empty(n, device="cuda") for _ in range(R)]
        seam_stream = torch.cuda.Stream()

        def start(c=None):
            c = c or g
            c.fill_synthetic(20260101)
            for i in range(R):
                c.replica_write(i, BUF_GRADIENT, grad)
                c.replica_write(i, BUF_LAST, grad)
            c.wait()

        def seam_start():
            """The context's start, copied into the caller-owned buffers."""
            start()
            sz.copy_(torch.from_numpy(g.base_read(0, BUF_DATA)))
            for i in range(R):
                sw[i].copy_(torch.from_numpy(g.replica_read(i, BUF_DATA)))
                ss[i].zero_()
                sg[i].copy_(dev_grad)
                sl[i].copy_(dev_grad)
            torch.cuda.synchronize()

        def clock_iteration(form):
            discard = STEP_DISCARD_TASK_OUTPUTS if form.endswith("discard") else 0
            if form in SEAM_FORMS:
                reps = [(0, sw[i].data_ptr(), ss[i].data_ptr(), sg[i].data_ptr(), sl[i].data_ptr(), 1, 1, LR)
                        for i in range(R)]
                plan.elastic_step_and_optimise([seam_stream.cuda_stream], [sz.data_ptr()], reps, ALPHA, MOMENTUM, WD, 0,
                                               discard)
                return
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            if form == "sma_fused":
                state["sma_clock"] += 1
                sma.lockAny()
                sma.step_and_synchronise(0, state["sma_clock"], 0, tasks, None, 0)
                sma.unlockAny()
                return
            state["clock"] += 1
            if form == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
                g.unlockAny()
                return
            g.lockAny()
            g.step_and_synchronise_elastic(0, state["clock"], 0, tasks, None, discard)
            g.unlockAny()

        def mark(form):
            """An event behind the end of the last step."""
            e = torch.cuda.Event(enable_timing=True)
            if form in SEAM_FORMS:
                e.record(seam_stream)
                return e
            c = sma if form == "sma_fused" else g
            if hip.hipStreamWaitEvent(side.cuda_stream, c.step_event(0), 0) != 0:
                raise RuntimeError("hipStreamWaitEvent failed")
            e.record(side)
            return e

        def timed(form, count):
            a = mark(form)
            for _ in range(count):
                clock_iteration(form)
            b = mark(form)
            b.synchronize()
            return a.elapsed_time(b) / count

        def digest(form):
            h = hashlib.sha256()
            if form in SEAM_FORMS:
                for t in [sz] + sw:
                    h.update(t.cpu().numpy().tobytes())
                return h.hexdigest()
            h.update(g.base_read(0, BUF_DATA).tobytes())
            for i in range(R):
                h.update(g.replica_read(i, BUF_DATA).tobytes())
            return h.hexdigest()

        def digest_run(form):
            seam = form in SEAM_FORMS
            (seam_start if seam else start)()
            for _ in range(args.digest_clocks):
                for i in range(R):
                    if seam:
                        sg[i].copy_(dev_grad)
                    else:
                        g.replica_write(i, BUF_GRADIENT, grad)
                torch.cuda.synchronize()
                clock_iteration(form)
                g.wait()
                torch.cuda.synchronize()
            return digest(form)

        digests = {f: digest_run(f) for f in ("sequence",) + NEW_FORMS}

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        seam_start()
        start(sma)
        ms = {f: [] for f in FORMS}
        for f in FORMS:
            timed(f, args.warmup)
        for _ in range(args.batches):
            for f in FORMS:
                ms[f].append(timed(f, args.steps))
        g.wait()
        sma.wait()
        torch.cuda.synchronize()

        sweep, best = 0, None
        if args.sweep:
            for unroll in (1, 2):
                for waves in (-1, 0, 2, 3, 4, 8):
                    g.set_task_barrier_kernel_config(64, unroll, waves)
                    row = {"sweep": "task_barrier_elastic", "block": 64, "unroll": unroll, "waves_per_cu": waves}
                    for f in ("fused", "discard"):
                        timed(f, 3)
                        row[f + "_us"] = round(1e3 * timed(f, args.steps), 2)
                    print(json.dumps(row), flush=True)
                    if best is None or row["fused_us"] < best["fused_us"]:
                        best = row
                    sweep += 1
            g.set_task_barrier_kernel_config(64, 1, -1)  # the default
        base, reps = g.modelStats(BUF_DATA)
        finite = int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        finite = finite and bool(torch.isfinite(sz).all()) and all(bool(torch.isfinite(t).all()) for t in sw)
        copy_GBs = g.bench_copy(4 * n, 20)

        seq_bytes, fused_bytes, discard_bytes = (36 * R + 8) * n, (28 * R + 8) * n, (20 * R + 8) * n
        bytes_per = {"sequence": seq_bytes, "fused": fused_bytes, "discard": discard_bytes, "seam_fused": fused_bytes,
                     "seam_discard": discard_bytes, "sma_fused": (28 * R + 16) * n}
        med = {f: statistics.median(ms[f]) for f in FORMS}
        line = {
            "metric": "task steps fused into the one-GPU elastic-averaging barrier against the two-call sequence, "
                      "per clock",
            "model": args.model, "elements": n, "replicas": R, "alpha": ALPHA, "momentum": MOMENTUM,
            "weight_decay": WD, "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "copy_ceiling_GBs": round(copy_GBs, 1), "finite_at_the_end": finite,
            "digest_clocks": args.digest_clocks,
            "digests_equal_sequence": {f: digests[f] == digests["sequence"] for f in NEW_FORMS},
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
        for f in NEW_FORMS:
            line[f + "_speedup"] = round(med["sequence"] / med[f], 4)
            line[f + "_byte_ratio"] = round(seq_bytes / bytes_per[f], 4)
            # the share of the predicted gain that is there: (speed-up - 1) / (byte ratio - 1)
            line[f + "_share_of_predicted_gain"] = round((med["sequence"] / med[f] - 1.0) /
                                                         (seq_bytes / bytes_per[f] - 1.0), 4)
            line[f + "_faster_in_every_batch"] = bool(max(ms[f]) < min(ms["sequence"]))
        if best is not None:
            line["sweep_best"] = best
            line["sweep_best_over_default"] = round(best["fused_us"] / (1e3 * med["fused"]), 5)
        line["pass"] = bool(finite and all(line[f + "_faster_in_every_batch"] for f in NEW_FORMS)
                            and all(line["digests_equal_sequence"].values()))
        line["sweep_rows"] = sweep
        line["code_object_digest"] = code_object_digest(LIB)
        line["variables_code_object_digest"] = code_object_digest(VARIABLES_LIB)
        line["clipped_code_object_digest"] = code_object_digest(CLIPPED_LIB)
        line["clipped_variables_code_object_digest"] = code_object_digest(CLIPPED_VARIABLES_LIB)
        line["elastic_steps_code_object_digest"] = code_object_digest(ELASTIC_STEPS_LIB)
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        if plan is not None:
            plan.free()
        if sma is not None:
            sma.free()
        g.free()


if __name__ == "__main__":
    sys.exit(main())
