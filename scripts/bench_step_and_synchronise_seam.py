#!/usr/bin/env python3
"""Time the seam door of the fused task steps, cbx_sma_plan_step_and_optimise
over separately allocated caller buffers of exactly n floats, against the
seam's two-call sequence and against the context's cbx_step_and_synchronise
over its padded arena: ResNet-50's variables as bench.py registers them
(n = 25,557,032 = a bulk of 6,389,248 float4s and a 40-float tail), 8 replicas,
one GPU, alpha 0.1, momentum 0.9, weight decay 1e-4, rate 0.05.

In one process, after a warm-up of every form: 5 batches of 20 back-to-back
clocks of each form, the batches of the forms alternating.

  seam_sequence  R x cbx_sma_optimise_buffers, then cbx_sma_plan_step, all on
                 one stream: (40R + 16) n bytes per clock
  seam_fused     cbx_sma_plan_step_and_optimise, flags 0: (28R + 16) n
  seam_discard   the same with CBX_STEP_DISCARD_TASK_OUTPUTS: (20R + 16) n
  ctx_fused      cbx_step_and_synchronise, flags 0, the context's arena
  ctx_discard    the same with the discard flag

A seam batch is device time between two events on the caller's stream; a
context batch between two events on a side stream behind the step events
(scripts/bench_step_and_synchronise.py).  A second pass of the same batches
with the timing rings on (cbx_sma_plan_set_timing, cbx_set_timing) reads each
launch's own time.

Required: every seam_fused and seam_discard batch is faster than every
seam_sequence batch, and the values are finite at the end.  Target (reported):
each fused seam form's median per clock within 1 + (the context form's own
batch spread in this run) + 0.01 of the context form's with the same flag.

Once per form, from the same start and with the gradients rewritten before
every clock, a digest of z, the base `last` and every w_i is compared with the
seam sequence's.

Prints one JSON line.
Usage: python scripts/bench_step_and_synchronise_seam.py [--replicas 8] [--steps 20] [--batches 5]
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

SEAM = ("seam_sequence", "seam_fused", "seam_discard")
CTX = ("ctx_fused", "ctx_discard")
FORMS = SEAM + CTX
ALPHA, MOMENTUM, WD, RATE = 0.1, 0.9, 1e-4, 0.05


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--digest-clocks", type=int, default=2)
    ap.add_argument("--model", choices=["resnet50", "lenet"], default="resnet50")
    args = ap.parse_args()

    import torch

    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import code_object_digest
    from crossbow_amd.seam import SmaPlan, optimise_buffers
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int

    g = TheGPU()
    g.init([0])
    plan = None
    try:
        n = register(g, MODELS[args.model]())
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(ALPHA)
        g.setMomentum(MOMENTUM, 0)
        g.setWeightDecay(WD)
        g.setLearningRateDecayPolicyFixed(RATE)
        R = args.replicas
        g.setModelManager(R, SYNC_BSP)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        stream = torch.cuda.Stream()  # the caller's modelSynchronisationStream
        state = {"task": 0, "clock": 0}

        # the caller's side: one allocation of exactly n floats per model buffer
        dev = torch.device("cuda:0")
        new = lambda: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
        z, blast = new(), new()
        w, s, gr, rl = ([new() for _ in range(R)] for _ in range(4))
        grad_dev = torch.from_numpy(grad).to(dev)
        plan = SmaPlan([0], n)
        streams, zp, lp = [stream.cuda_stream], [z.data_ptr()], [blast.data_ptr()]
        plain = [(0, w[i].data_ptr(), s[i].data_ptr(), 1, 0) for i in range(R)]
        fused = [(0, w[i].data_ptr(), s[i].data_ptr(), gr[i].data_ptr(), rl[i].data_ptr(), 1, 0, 1, RATE)
                 for i in range(R)]

        def d2d(dst, src):
            if hip.hipMemcpy(dst, src, 4 * n, 3) != 0:
                raise RuntimeError("hipMemcpy failed")

        def start():
            """The same values in the context's arena and in the caller's buffers."""
            g.fill_synthetic(20260101)
            for i in range(R):
                g.replica_write(i, BUF_GRADIENT, grad)
                g.replica_write(i, BUF_LAST, grad)
            g.wait()
            torch.cuda.synchronize()
            d2d(z.data_ptr(), g.base_buffer(0, BUF_DATA))
            d2d(blast.data_ptr(), g.base_buffer(0, BUF_LAST))
            for i in range(R):
                for mine, kind in ((w, BUF_DATA), (s, BUF_DIFF), (gr, BUF_GRADIENT), (rl, BUF_LAST)):
                    d2d(mine[i].data_ptr(), g.replica_buffer(i, kind))
            torch.cuda.synchronize()

        def rewrite_gradients():
            for i in range(R):
                g.replica_write(i, BUF_GRADIENT, grad)
                with torch.cuda.stream(stream):
                    gr[i].copy_(grad_dev)
            g.wait()
            stream.synchronize()

        def clock_iteration(form):
            if form == "seam_sequence":
                for i in range(R):
                    optimise_buffers(stream.cuda_stream, w[i].data_ptr(), gr[i].data_ptr(), rl[i].data_ptr(),
                                     s[i].data_ptr(), n, RATE, MOMENTUM, WD)
                plan.step(streams, zp, lp, plain, ALPHA, MOMENTUM)
            elif form in SEAM:
                plan.step_and_optimise(streams, zp, lp, fused, ALPHA, MOMENTUM, MOMENTUM, WD, 0,
                                       STEP_DISCARD_TASK_OUTPUTS if form == "seam_discard" else 0)
            else:
                tasks = list(range(state["task"], state["task"] + R))
                state["task"] += R
                state["clock"] += 1
                g.lockAny()
                g.step_and_synchronise(0, state["clock"], 0, tasks, None,
                                       STEP_DISCARD_TASK_OUTPUTS if form == "ctx_discard" else 0)
                g.unlockAny()

        def mark(form):
            e = torch.cuda.Event(enable_timing=True)
            if form in SEAM:
                e.record(stream)
            else:  # behind the end of the context's last step
                if hip.hipStreamWaitEvent(side.cuda_stream, g.step_event(0), 0) != 0:
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
            if form in SEAM:
                stream.synchronize()
                for t in [z, blast] + w:
                    h.update(t.cpu().numpy().tobytes())
            else:
                g.wait()
                h.update(g.base_read(0, BUF_DATA).tobytes())
                h.update(g.base_read(0, BUF_LAST).tobytes())
                for i in range(R):
                    h.update(g.replica_read(i, BUF_DATA).tobytes())
            return h.hexdigest()

        # same start, same fresh gradient before every clock: the five forms must agree
        digests = {}
        for form in FORMS:
            start()
            for _ in range(args.digest_clocks):
                rewrite_gradients()
                clock_iteration(form)
            digests[form] = digest(form)

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        def ring_median(form):
            if form in SEAM:
                return statistics.median(plan.timing_history(args.steps)[1:])
            return statistics.median(g.timing_history()[1:])

        def rounds(timing):
            start()
            ms = {f: [] for f in FORMS}
            ring = {f: [] for f in FORMS}
            for f in FORMS:
                timed(f, args.warmup)
            for _ in range(args.batches):
                for f in FORMS:
                    if timing:  # an empty ring per batch
                        plan.set_timing(True)
                        g.set_timing(True)
                    ms[f].append(timed(f, args.steps))
                    if timing:
                        ring[f].append(ring_median(f))
            if timing:
                plan.set_timing(False)
                g.set_timing(False)
            return ms, ring

        ms, _ = rounds(False)
        ms_t, ring = rounds(True)
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(t).all().item()) for t in [z, blast] + w + s + gr + rl)
        base, reps = g.modelStats(BUF_DATA)
        finite = finite and int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        copy_GBs = g.bench_copy(4 * n, 20)

        bytes_per = {"seam_sequence": (40 * R + 16) * n, "seam_fused": (28 * R + 16) * n,
                     "seam_discard": (20 * R + 16) * n, "ctx_fused": (28 * R + 16) * n,
                     "ctx_discard": (20 * R + 16) * n}
        med = {f: statistics.median(ms[f]) for f in FORMS}
        launch = {f: statistics.median(ring[f]) for f in FORMS}
        line = {
            "metric": "the fused task steps through the sma.c seam against the seam's two-call sequence and the "
                      "context's fused call, per clock",
            "model": args.model, "elements": n, "bulk_float4s": (n // 4) // 256 * 256,
            "tail_floats": n - (n // 4) // 256 * 1024, "replicas": R, "alpha": ALPHA, "momentum": MOMENTUM,
            "weight_decay": WD, "learning_rate": RATE,
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "copy_ceiling_GBs": round(copy_GBs, 1),
            "finite_at_the_end": finite, "digest_clocks": args.digest_clocks,
            "digests_equal_seam_sequence": {f: digests[f] == digests["seam_sequence"] for f in FORMS[1:]},
            "sma_step_launch_ms": round(launch["seam_sequence"], 5),
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_batches_ms_timing_on"] = [round(x, 5) for x in ms_t[f]]
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
            if f != "seam_sequence":
                line[f + "_launch_ms"] = round(launch[f], 5)
                line[f + "_launch_batches_ms"] = [round(x, 5) for x in ring[f]]
        for f, yard in (("seam_fused", "ctx_fused"), ("seam_discard", "ctx_discard")):
            gate = 1.0 + spread(ms[yard]) + 0.01
            line[f + "_speedup"] = round(med["seam_sequence"] / med[f], 4)
            line[f + "_faster_in_every_batch"] = bool(max(ms[f]) < min(ms["seam_sequence"]) and
                                                      max(ms_t[f]) < min(ms_t["seam_sequence"]))
            line[f + "_over_context"] = round(med[f] / med[yard], 5)
            line[f + "_launch_over_context"] = round(launch[f] / launch[yard], 5)
            line[f + "_target_gate"] = round(gate, 5)
            line[f + "_meets_target"] = bool(med[f] / med[yard] <= gate)
        line["pass"] = bool(line["seam_fused_faster_in_every_batch"] and line["seam_discard_faster_in_every_batch"]
                            and finite and all(line["digests_equal_seam_sequence"].values()))
        line["code_object_digest"] = code_object_digest()
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        if plan is not None:
            plan.free()
        g.free()


if __name__ == "__main__":
    sys.exit(main())
