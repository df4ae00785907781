#!/usr/bin/env python3
"""Time the task steps fused into the one-GPU SMA barrier
(cbx_step_and_synchronise) against the two-call sequence, at the C3 shape:
ResNet-50's variables as bench.py registers them (n = 25,557,032), 8 replicas,
one GPU, alpha 0.1, momentum 0.9, weight decay 1e-4.

In one process, after a warm-up of every form: 5 batches of 20 back-to-back
clock iterations of each form, the batches of the forms alternating.

  sequence   R x cbx_replica_optimise on the sync stream, then cbx_synchronise
             (one stream carries everything): (40R + 16) n bytes per clock
  fused      cbx_step_and_synchronise, flags 0: (28R + 16) n bytes
  discard    cbx_step_and_synchronise, CBX_STEP_DISCARD_TASK_OUTPUTS: (20R + 16) n

Each batch is device time between two events on a side stream: the first
recorded behind the step event of the step before the batch, the second
behind the step event of its last step.  A second pass of the same batches
with cbx_set_timing on reads each barrier launch's own time from the timing
ring (the sequence's barrier starts at a marker of its own, a fused launch
queued behind a busy GPU at the stop of the launch before it: stop to stop,
an upper bound).  The copy ceiling is cbx_bench_copy in the same process.

The yardstick is the sequence in the same process.  Required: every fused and
discard batch is faster than every sequence batch of the same round.  Target
(reported): each fused form's GB/s over its algorithmic bytes within
1 + (the SMA step's batch spread) + 0.01 of the SMA step's own GB/s.

Once per form, from the same start and with the gradients rewritten before
every clock, a digest of z, the base `last` and every w_i is compared with the
sequence's.

--sweep adds float4s per lane x waves per CU through
cbx_set_task_barrier_kernel_config (ring times of 20 launches per shape).

Prints one JSON line (and one per swept shape before it).
Usage: python scripts/bench_step_and_synchronise.py [--replicas 8] [--steps 20] [--batches 5] [--sweep]
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

FORMS = ("sequence", "fused", "discard")


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

    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import code_object_digest
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int

    g = TheGPU()
    g.init([0])
    try:
        n = register(g, MODELS[args.model]())
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(0.05)
        R = args.replicas
        g.setModelManager(R, SYNC_BSP)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0}

        def start():
            g.fill_synthetic(20260101)
            for i in range(R):
                g.replica_write(i, BUF_GRADIENT, grad)
                g.replica_write(i, BUF_LAST, grad)
            g.wait()

        def clock_iteration(form):
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"] += 1
            if form == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
            else:
                g.lockAny()
                g.step_and_synchronise(0, state["clock"], 0, tasks, None,
                                       STEP_DISCARD_TASK_OUTPUTS if form == "discard" else 0)
            g.unlockAny()

        def mark():
            """An event on the side stream behind the end of the last step."""
            if hip.hipStreamWaitEvent(side.cuda_stream, g.step_event(0), 0) != 0:
                raise RuntimeError("hipStreamWaitEvent failed")
            e = torch.cuda.Event(enable_timing=True)
            e.record(side)
            return e

        def timed(form, count):
            a = mark()
            for _ in range(count):
                clock_iteration(form)
            b = mark()
            b.synchronize()
            return a.elapsed_time(b) / count

        def digest():
            h = hashlib.sha256()
            h.update(g.base_read(0, BUF_DATA).tobytes())
            h.update(g.base_read(0, BUF_LAST).tobytes())
            for i in range(R):
                h.update(g.replica_read(i, BUF_DATA).tobytes())
            return h.hexdigest()

        # same start, same fresh gradient before every clock: the three forms must agree
        digests = {}
        for form in FORMS:
            start()
            for _ in range(args.digest_clocks):
                for i in range(R):
                    g.replica_write(i, BUF_GRADIENT, grad)
                clock_iteration(form)
                g.wait()
            digests[form] = digest()

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        def rounds(timing):
            start()
            ms = {f: [] for f in FORMS}
            ring = {f: [] for f in FORMS}
            for f in FORMS:
                timed(f, args.warmup)
            for _ in range(args.batches):
                for f in FORMS:
                    if timing:
                        g.set_timing(True)  # an empty ring per batch
                    ms[f].append(timed(f, args.steps))
                    if timing:
                        ring[f].append(statistics.median(g.timing_history()[1:]))
            if timing:
                g.set_timing(False)
            return ms, ring

        ms, _ = rounds(False)
        ms_t, ring = rounds(True)
        base, reps = g.modelStats(BUF_DATA)
        finite = int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        copy_GBs = g.bench_copy(4 * n, 20)

        sweep = []
        if args.sweep:
            for unroll in (1, 2):
                for waves in (-1, 0, 2, 3, 4, 6, 8):
                    g.set_task_barrier_kernel_config(64, unroll, waves)
                    row = {"sweep": "task_barrier", "block": 64, "unroll": unroll, "waves_per_cu": waves}
                    for f in ("fused", "discard"):
                        for _ in range(3):
                            clock_iteration(f)
                        g.set_timing(True)
                        for _ in range(args.steps):
                            clock_iteration(f)
                        g.wait()
                        row[f + "_launch_us"] = round(1e3 * statistics.median(g.timing_history()[1:]), 3)
                        g.set_timing(False)
                    sweep.append(row)
                    print(json.dumps(row), flush=True)
            g.set_task_barrier_kernel_config(64, 1, -1)  # the default

        bytes_per = {"sequence": (40 * R + 16) * n, "fused": (28 * R + 16) * n, "discard": (20 * R + 16) * n}
        sma_bytes = (12 * R + 16) * n
        med = {f: statistics.median(ms[f]) for f in FORMS}
        launch = {f: statistics.median(ring[f]) for f in FORMS}
        sma_GBs = sma_bytes / (launch["sequence"] * 1e-3) / 1e9
        gate = 1.0 + spread(ring["sequence"]) + 0.01
        line = {
            "metric": "task steps fused into the one-GPU SMA barrier against the two-call sequence, per clock",
            "model": args.model, "elements": n, "replicas": R, "alpha": 0.1, "momentum": 0.9, "weight_decay": 1e-4,
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "sma_step_bytes": sma_bytes,
            "copy_ceiling_GBs": round(copy_GBs, 1),
            "finite_at_the_end": finite,
            "digest_clocks": args.digest_clocks,
            "digests_equal_sequence": {f: digests[f] == digests["sequence"] for f in ("fused", "discard")},
            "sma_step_launch_ms": round(launch["sequence"], 5),
            "sma_step_launch_batches_ms": [round(x, 5) for x in ring["sequence"]],
            "sma_step_spread": round(spread(ring["sequence"]), 5),
            "sma_step_GBs": round(sma_GBs, 1),
            "target_gate": round(gate, 5),
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_batches_ms_timing_on"] = [round(x, 5) for x in ms_t[f]]
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
        for f in ("fused", "discard"):
            gbs = bytes_per[f] / (launch[f] * 1e-3) / 1e9
            line[f + "_launch_ms"] = round(launch[f], 5)
            line[f + "_launch_batches_ms"] = [round(x, 5) for x in ring[f]]
            line[f + "_launch_GBs"] = round(gbs, 1)
            line[f + "_launch_fraction_of_copy"] = round(gbs / copy_GBs, 4)
            line[f + "_sma_GBs_over_own"] = round(sma_GBs / gbs, 5)
            line[f + "_meets_target"] = bool(sma_GBs / gbs <= gate)
            line[f + "_speedup"] = round(med["sequence"] / med[f], 4)
            line[f + "_faster_in_every_batch"] = bool(all(x < y for x, y in zip(ms[f], ms["sequence"])) and
                                                      all(x < y for x, y in zip(ms_t[f], ms_t["sequence"])))
        line["pass"] = bool(line["fused_faster_in_every_batch"] and line["discard_faster_in_every_batch"] and finite
                            and all(line["digests_equal_sequence"].values()))
        line["sweep_rows"] = len(sweep)
        line["code_object_digest"] = code_object_digest()
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        g.free()


if __name__ == "__main__":
    sys.exit(main())
