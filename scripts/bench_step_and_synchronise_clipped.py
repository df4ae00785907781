#!/usr/bin/env python3
"""Time the fused task-step barrier with gradient clipping
(cbx_step_and_synchronise_clipped, cbx_sma_plan_step_and_optimise_clipped)
against the clipped two-call sequence it replaces, with the protocol of
scripts/bench_step_and_synchronise_variables.py: one process, ResNet-50's
variables as bench.py registers them (n = 25,557,032), 8 replicas, one GPU,
alpha 0.1, momentum 0.9, weight decay 1e-4.

After a warm-up of every form: 5 batches of 20 back-to-back clock iterations of
each form, the batches of the forms alternating, device time from events.

  (a)  sequence        R x cbx_replica_optimise with clipping on (a max_norm
                       that never clips), then cbx_synchronise: the yardstick
  (b)  plain           cbx_step_and_synchronise with clipping off: (28R + 16) n
  (b') plain_discard   the same with CBX_STEP_DISCARD_TASK_OUTPUTS: (20R + 16) n
  (c)  fused           cbx_step_and_synchronise_clipped, the same max_norm
  (d)  discard         the same with the discard flag
  (c") fused_clipping  cbx_step_and_synchronise_clipped with a max_norm that
                       clips every step
  (e)  seam_fused, seam_discard
                       cbx_sma_plan_step_and_optimise_clipped over buffers of
                       exactly n floats, timed by events on the caller's stream
  (f)  norm            the norm pass and the reduce alone, by their own
                       timestamps (cbx_sma_plan_gradient_norm), median of 9

Once per form, from the same start and with the gradients rewritten before
every clock, a digest of z, the base `last` and every w_i is compared with
(a)'s; (c")'s with that of the sequence at its own max_norm.

Required: (c), (c"), (d) and both seam forms are faster than (a) in every
batch (the slowest batch of each beats the fastest batch of (a)), values are
finite at the end, and the digests are (a)'s.  Target, reported: (c) within
1 + (b)'s batch spread + 0.01 of (b) + R x ((f)'s pass + reduce), and (d)
likewise with (b').

--sweep adds float4s per lane x waves per CU through
cbx_set_task_barrier_kernel_config: one batch of (b), (b'), (c) and (d) per
shape, one JSON line each, before the result line.

Prints one JSON line (and one per swept shape before it).
Usage: python scripts/bench_step_and_synchronise_clipped.py [--replicas 8] [--steps 20] [--batches 5] [--sweep]
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

CONTEXT_FORMS = ("sequence", "plain", "plain_discard", "fused", "discard", "fused_clipping")
SEAM_FORMS = ("seam_fused", "seam_discard")
FORMS = CONTEXT_FORMS + SEAM_FORMS
LR = 0.05
NEVER, ALWAYS = 1e30, 1e-3  # max_norm: above and below the norm of every gradient here


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

    from crossbow_amd import BUF_DATA, BUF_DIFF, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import CLIPPED_LIB, LIB, code_object_digest
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int

    shapes = MODELS[args.model]()
    g = TheGPU()
    g.init([0])
    plan = None
    try:
        n = register(g, shapes)
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(LR)
        R = args.replicas
        g.setModelManager(R, SYNC_BSP)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0}

        # the seam's buffers: exactly n floats each, on a stream of the caller's
        plan = SmaPlan([0], n)
        dev_grad = torch.from_numpy(grad).cuda()
        sz, slast = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        sw = [torch.empty(n, device="cuda") for _ in range(R)]
        ss = [torch.empty(n, device="cuda") for _ in range(R)]
        sg = [torch.empty(n, device="cuda") for _ in range(R)]
        sl = [torch.empty(n, device="cuda") for _ in range(R)]
        seam_stream = torch.cuda.Stream()

        def start():
            g.fill_synthetic(20260101)
            for i in range(R):
                g.replica_write(i, BUF_GRADIENT, grad)
                g.replica_write(i, BUF_LAST, grad)
            g.wait()

        def seam_start():
            """The context's start, copied into the caller-owned buffers."""
            start()
            sz.copy_(torch.from_numpy(g.base_read(0, BUF_DATA)))
            slast.copy_(torch.from_numpy(g.base_read(0, BUF_LAST)))
            for i in range(R):
                sw[i].copy_(torch.from_numpy(g.replica_read(i, BUF_DATA)))
                ss[i].copy_(torch.from_numpy(g.replica_read(i, BUF_DIFF)))
                sg[i].copy_(dev_grad)
                sl[i].copy_(dev_grad)
            torch.cuda.synchronize()

        def clock_iteration(form, max_norm=NEVER):
            if form in SEAM_FORMS:
                reps = [(0, sw[i].data_ptr(), ss[i].data_ptr(), sg[i].data_ptr(), sl[i].data_ptr(), 1, 0, 1, LR)
                        for i in range(R)]
                plan.step_and_optimise_clipped([seam_stream.cuda_stream], [sz.data_ptr()], [slast.data_ptr()], reps,
                                               0.1, 0.9, 0.9, 1e-4, 0,
                                               STEP_DISCARD_TASK_OUTPUTS if form == "seam_discard" else 0,
                                               slots=list(range(R)), max_norm=max_norm, skip_nonfinite=True)
                return
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"] += 1
            if form in ("plain", "plain_discard"):
                g.set_gradient_clip(0.0, False)
                g.lockAny()
                g.step_and_synchronise(0, state["clock"], 0, tasks, None,
                                       STEP_DISCARD_TASK_OUTPUTS if form == "plain_discard" else 0)
                g.unlockAny()
                return
            g.set_gradient_clip(ALWAYS if form == "fused_clipping" else max_norm, True)
            if form == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
            else:
                g.lockAny()
                g.step_and_synchronise_clipped(0, state["clock"], 0, tasks, None,
                                               STEP_DISCARD_TASK_OUTPUTS if form == "discard" else 0)
            g.unlockAny()

        def mark(form):
            """An event behind the end of the last step."""
            e = torch.cuda.Event(enable_timing=True)
            if form in SEAM_FORMS:
                e.record(seam_stream)
                return e
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
            if form in SEAM_FORMS:
                for t in [sz, slast] + sw:
                    h.update(t.cpu().numpy().tobytes())
                return h.hexdigest()
            h.update(g.base_read(0, BUF_DATA).tobytes())
            h.update(g.base_read(0, BUF_LAST).tobytes())
            for i in range(R):
                h.update(g.replica_read(i, BUF_DATA).tobytes())
            return h.hexdigest()

        def digest_run(form, max_norm=NEVER):
            seam = form in SEAM_FORMS
            (seam_start if seam else start)()
            for _ in range(args.digest_clocks):
                for i in range(R):
                    if seam:
                        sg[i].copy_(dev_grad)
                    else:
                        g.replica_write(i, BUF_GRADIENT, grad)
                torch.cuda.synchronize()
                clock_iteration(form, max_norm)
                g.wait()
                torch.cuda.synchronize()
            return digest(form)

        digests = {f: digest_run(f) for f in FORMS if f not in ("plain", "plain_discard")}
        digests["sequence_clipping"] = digest_run("sequence", ALWAYS)
        clipped_steps = g.replica_clip_stats(0)["clipped_steps"]

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        seam_start()
        ms = {f: [] for f in FORMS}
        for f in FORMS:
            timed(f, args.warmup)
        for _ in range(args.batches):
            for f in FORMS:
                ms[f].append(timed(f, args.steps))
        g.wait()
        torch.cuda.synchronize()

        # (f): the norm pass and the reduce alone, over one of the seam's gradients
        norm = [plan.gradient_norm(0, 63, seam_stream.cuda_stream, sg[0].data_ptr(), NEVER, True)[1:] for _ in range(9)]
        norm_pass, norm_reduce = (statistics.median(x[k] for x in norm) for k in (0, 1))

        sweep = 0
        if args.sweep:
            for unroll in (1, 2):
                for waves in (-1, 0, 2, 3, 4, 8):
                    g.set_task_barrier_kernel_config(64, unroll, waves)
                    row = {"sweep": "task_barrier_clipped", "block": 64, "unroll": unroll, "waves_per_cu": waves}
                    for f in ("plain", "plain_discard", "fused", "discard"):
                        timed(f, 3)
                        row[f + "_us"] = round(1e3 * timed(f, args.steps), 2)
                    print(json.dumps(row), flush=True)
                    sweep += 1
            g.set_task_barrier_kernel_config(64, 1, -1)  # the default
        base, reps = g.modelStats(BUF_DATA)
        finite = int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        copy_GBs = g.bench_copy(4 * n, 20)

        fused_bytes, discard_bytes = (28 * R + 16) * n, (20 * R + 16) * n
        norm_bytes = 4 * R * n  # the norm passes read every stepping replica's g once more
        bytes_per = {"sequence": (40 * R + 16) * n + norm_bytes, "plain": fused_bytes, "plain_discard": discard_bytes,
                     "fused": fused_bytes + norm_bytes, "discard": discard_bytes + norm_bytes,
                     "fused_clipping": fused_bytes + norm_bytes, "seam_fused": fused_bytes + norm_bytes,
                     "seam_discard": discard_bytes + norm_bytes}
        med = {f: statistics.median(ms[f]) for f in FORMS}
        line = {
            "metric": "clipped task steps fused into the one-GPU SMA barrier against the clipped two-call sequence, "
                      "per clock",
            "model": args.model, "elements": n, "variables": len(shapes), "replicas": R, "alpha": 0.1,
            "momentum": 0.9, "weight_decay": 1e-4, "max_norm_never": NEVER, "max_norm_always": ALWAYS,
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "copy_ceiling_GBs": round(copy_GBs, 1), "finite_at_the_end": finite,
            "digest_clocks": args.digest_clocks,
            "digests_equal_sequence": {f: digests[f] == digests["sequence_clipping" if f == "fused_clipping" else "sequence"]
                                       for f in digests if not f.startswith("sequence")},
            "clipping_digest_differs_from_never": digests["sequence_clipping"] != digests["sequence"],
            "clipped_steps_of_replica_0_after_the_digest_runs": int(clipped_steps),
            "norm_pass_ms": round(norm_pass, 5), "norm_reduce_ms": round(norm_reduce, 5),
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
        new_forms = ("fused", "discard", "fused_clipping", "seam_fused", "seam_discard")
        for f in new_forms:
            line[f + "_speedup"] = round(med["sequence"] / med[f], 4)
            line[f + "_faster_in_every_batch"] = bool(max(ms[f]) < min(ms["sequence"]))
        for f, ceiling in (("fused", "plain"), ("discard", "plain_discard")):
            budget = med[ceiling] + R * (norm_pass + norm_reduce)
            gate = 1.0 + spread(ms["plain"]) + 0.01
            line[f + "_budget_ms"] = round(budget, 5)
            line[f + "_over_budget"] = round(med[f] / budget, 5)
            line[f + "_target_gate"] = round(gate, 5)
            line[f + "_meets_target"] = bool(med[f] / budget <= gate)
        line["pass"] = bool(finite and all(line[f + "_faster_in_every_batch"] for f in new_forms)
                            and all(line["digests_equal_sequence"].values()))
        line["sweep_rows"] = sweep
        line["code_object_digest"] = code_object_digest(LIB)
        line["clipped_code_object_digest"] = code_object_digest(CLIPPED_LIB)
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        if plan is not None:
            plan.free()
        g.free()


if __name__ == "__main__":
    sys.exit(main())
