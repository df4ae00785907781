#!/usr/bin/env python3
"""Time the fused task-step barrier with gradient clipping and a learning rate
per variable (cbx_step_and_synchronise_clipped_variables,
cbx_sma_plan_step_and_optimise_clipped_variables) against the two-call sequence
it replaces, with the protocol of scripts/bench_step_and_synchronise_clipped.py:
one process, ResNet-50's variables as bench.py registers them (n = 25,557,032,
161 variables), the 106 batch-norm variables at multiplier 2 as
scripts/bench_step_and_synchronise_variables.py builds them, 8 replicas, one
GPU, alpha 0.1, momentum 0.9, weight decay 1e-4, a max_norm that clips every
step.

After a warm-up of every form: 5 batches of 20 back-to-back clock iterations of
each form, the batches of the forms alternating, device time from events.

  (a)  sequence        R x cbx_replica_optimise with both features on, then
                       cbx_synchronise: the yardstick
  (k)  clipped         cbx_step_and_synchronise_clipped, variable rates off
  (v)  variables       cbx_step_and_synchronise_variables, clipping off
  (b)  plain           cbx_step_and_synchronise, both off
       clipped_discard, variables_discard, plain_discard
                       (k), (v) and (b) with CBX_STEP_DISCARD_TASK_OUTPUTS
  (c)  fused           cbx_step_and_synchronise_clipped_variables
  (d)  discard         the same with CBX_STEP_DISCARD_TASK_OUTPUTS
  (e)  seam_fused, seam_discard
                       cbx_sma_plan_step_and_optimise_clipped_variables over
                       buffers of exactly n floats, timed by events on the
                       caller's stream

Once per form, from the same start and with the gradients rewritten before
every clock, a digest of z, the base `last` and every w_i is compared with
(a)'s.

Required: the slowest batch of (c), of (d) and of each seam form is below the
fastest batch of (a), values are finite at the end, and the digests are (a)'s.
Reported: (c) against the additive budget (k) + ((v) - (b)) with a margin of
1 + (k)'s batch spread + 0.01, the same for (d) from the discarding forms of
(k), (v) and (b), and with --sweep the best launch shape against the default.
The same kernel has moved by 8 % between runs of one machine, so only ratios
inside one process mean anything.

--sweep adds float4s per lane x waves per CU through
cbx_set_task_barrier_kernel_config: one batch of (c) and (d) per shape, one
JSON line each, before the result line.

Prints one JSON line (and one per swept shape before it).
Usage: python scripts/bench_step_and_synchronise_clipped_variables.py [--replicas 8] [--steps 20] [--batches 5] [--sweep]
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONTEXT_FORMS = ("sequence", "clipped", "variables", "plain", "clipped_discard", "variables_discard", "plain_discard",
                 "fused", "discard")
SEAM_FORMS = ("seam_fused", "seam_discard")
FORMS = CONTEXT_FORMS + SEAM_FORMS
NEW_FORMS = ("fused", "discard") + SEAM_FORMS
LR = 0.05
BN_MULTIPLIER = 2.0
BOTH = ("sequence", "fused", "discard")  # the forms with clipping and variable rates on
MAX_NORM = 1e-3  # below the norm of every gradient here: every step clips


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
    from crossbow_amd.build import CLIPPED_LIB, CLIPPED_VARIABLES_LIB, LIB, VARIABLES_LIB, code_object_digest
    from crossbow_amd.seam import SmaPlan
    from crossbow_amd.variables import MODELS, register
    from oracle import oracle as O

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    hip.hipStreamWaitEvent.restype = ctypes.c_int

    shapes = MODELS[args.model]()
    # the batch-norm variables: every 1-D shape but the last layer's bias
    bn = [k for k, s in enumerate(shapes) if len(s) == 1 and k != len(shapes) - 1]
    var_elements = [int(np.prod(s)) for s in shapes]
    mults = [BN_MULTIPLIER if k in set(bn) else 1.0 for k in range(len(shapes))]

    g = TheGPU()
    g.init([0])
    plan = None
    try:
        n = register(g, shapes)
        for k in bn:
            g.setModelVariableLearningRateMultiplier(k, 1, BN_MULTIPLIER)
        g.setUpdateModelType(UPDATE_SMA)
        g.setEamsgdAlpha(0.1)
        g.setMomentum(0.9, 0)
        g.setWeightDecay(1e-4)
        g.setLearningRateDecayPolicyFixed(LR)
        R = args.replicas
        g.setModelManager(R, SYNC_BSP)
        grad = O.fill_normal(n, 77, 0.01)
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0, "clip": None, "rates": None}

        # the seam's buffers: exactly n floats each, on a stream of the caller's
        plan = SmaPlan([0], n)
        plan.set_variables(var_elements, mults)
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

        def clock_iteration(form):
            if form in SEAM_FORMS:
                reps = [(0, sw[i].data_ptr(), ss[i].data_ptr(), sg[i].data_ptr(), sl[i].data_ptr(), 1, 0, 1, LR)
                        for i in range(R)]
                plan.step_and_optimise_clipped_variables(
                    [seam_stream.cuda_stream], [sz.data_ptr()], [slast.data_ptr()], reps, 0.1, 0.9, 0.9, 1e-4, 0,
                    STEP_DISCARD_TASK_OUTPUTS if form == "seam_discard" else 0, slots=list(range(R)),
                    max_norm=MAX_NORM, skip_nonfinite=True)
                return
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            state["clock"] += 1
            kind = form.replace("_discard", "")
            clip, rates = kind in BOTH + ("clipped",), kind in BOTH + ("variables",)
            if clip != state["clip"]:  # the setters are called where a form differs from the one before it only
                g.set_gradient_clip(MAX_NORM if clip else 0.0, clip)
            if rates != state["rates"]:
                g.set_variable_learning_rates(rates)
            state["clip"], state["rates"] = clip, rates
            if form == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
                g.unlockAny()
                return
            call = {"clipped": g.step_and_synchronise_clipped, "variables": g.step_and_synchronise_variables,
                    "plain": g.step_and_synchronise}.get(kind, g.step_and_synchronise_clipped_variables)
            g.lockAny()
            call(0, state["clock"], 0, tasks, None, STEP_DISCARD_TASK_OUTPUTS if form.endswith("discard") else 0)
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
        digests["clipped"] = digest_run("clipped")  # the multipliers matter: another digest
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

        sweep, best = 0, None
        if args.sweep:
            for unroll in (1, 2):
                for waves in (-1, 0, 2, 3, 4, 8):
                    g.set_task_barrier_kernel_config(64, unroll, waves)
                    row = {"sweep": "task_barrier_clipped_variables", "block": 64, "unroll": unroll,
                           "waves_per_cu": waves}
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
        copy_GBs = g.bench_copy(4 * n, 20)

        fused_bytes, discard_bytes = (28 * R + 16) * n, (20 * R + 16) * n
        norm_bytes = 4 * R * n  # the norm passes read every stepping replica's g once more
        bytes_per = {"sequence": (40 * R + 16) * n + norm_bytes, "clipped": fused_bytes + norm_bytes,
                     "variables": fused_bytes, "plain": fused_bytes, "clipped_discard": discard_bytes + norm_bytes,
                     "variables_discard": discard_bytes, "plain_discard": discard_bytes,
                     "fused": fused_bytes + norm_bytes,
                     "discard": discard_bytes + norm_bytes, "seam_fused": fused_bytes + norm_bytes,
                     "seam_discard": discard_bytes + norm_bytes}
        med = {f: statistics.median(ms[f]) for f in FORMS}
        line = {
            "metric": "clipped task steps with per-variable rates fused into the one-GPU SMA barrier against the "
                      "two-call sequence, per clock",
            "model": args.model, "elements": n, "variables": len(shapes), "irregular_variables": len(bn),
            "multiplier": BN_MULTIPLIER, "replicas": R, "alpha": 0.1, "momentum": 0.9, "weight_decay": 1e-4,
            "max_norm": MAX_NORM, "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "copy_ceiling_GBs": round(copy_GBs, 1), "finite_at_the_end": finite,
            "digest_clocks": args.digest_clocks,
            "digests_equal_sequence": {f: digests[f] == digests["sequence"] for f in NEW_FORMS},
            "clipped_digest_differs": digests["clipped"] != digests["sequence"],
            "clipped_steps_of_replica_0_after_the_digest_runs": int(clipped_steps),
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
        for f in NEW_FORMS:
            line[f + "_speedup"] = round(med["sequence"] / med[f], 4)
            line[f + "_faster_in_every_batch"] = bool(max(ms[f]) < min(ms["sequence"]))
        # reported, not gating: the additive budget (k) + ((v) - (b)), for (d) from the discarding forms
        for f, sfx in (("fused", ""), ("discard", "_discard")):
            budget = med["clipped" + sfx] + (med["variables" + sfx] - med["plain" + sfx])
            gate = 1.0 + spread(ms["clipped" + sfx]) + 0.01
            line[f + "_budget_ms"] = round(budget, 5)
            line[f + "_over_budget"] = round(med[f] / budget, 5)
            line[f + "_target_gate"] = round(gate, 5)
            line[f + "_meets_target"] = bool(med[f] / budget <= gate)
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
        print(json.dumps(line))
        return 0 if line["pass"] else 1
    finally:
        if plan is not None:
            plan.free()
        g.free()


if __name__ == "__main__":
    sys.exit(main())
