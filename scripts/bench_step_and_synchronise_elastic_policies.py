#!/usr/bin/env python3
"""The clipped and per-variable task steps fused into the one-GPU
elastic-averaging barrier (cbx_step_and_synchronise_elastic_clipped_variables,
cbx_ea_plan_step_and_optimise_clipped_variables) against the two-call sequence
under elastic averaging, per clock, on one GPU, with the protocol of
scripts/bench_step_and_synchronise_elastic.py.

One process, ResNet-50's 161 variables as bench.py registers them
(n = 25,557,032), the 106 batch-norm variables at multiplier 2, R replicas,
alpha 0.1, momentum 0.9, weight decay 1e-4.  Replica i's gradient is the same
normal data scaled by 0.5 + i / 8 and max_norm is 0.9 of the unscaled norm, so
the replicas from i = 4 on clip and the others do not.  The forms alternate in
batches of back-to-back clocks, each batch timed as device time between two
events.  For each policy P in variables, clipped, clipped_variables (what is
on):

  P_sequence      cbx_replica_optimise per replica, then cbx_synchronise
                  (update model 3 with elastic averaging): the yardstick
  P_fused         cbx_step_and_synchronise_elastic_clipped_variables
  P_discard       the same with CBX_STEP_DISCARD_TASK_OUTPUTS
  P_seam_fused, P_seam_discard
                  cbx_ea_plan_step_and_optimise_clipped_variables over buffers
                  of exactly n floats, timed on the caller's stream
  yardsticks, same process: plain_fused (cbx_step_and_synchronise_elastic, both
  features off), the four SMA calls on a second context (sma_plain,
  sma_variables, sma_clipped, sma_clipped_variables), and the float4 copy rate.

Bytes per clock: variables (36R + 8) n / (28R + 8) n / (20R + 8) n for the
sequence, the fused call and the discarding one; clipped (either) 4R n more in
each, the norm passes.

Required (exit status 1 otherwise), for each policy through both doors: the
slowest batch of the fused call, kept and discarding, is below the fastest
batch of that policy's sequence; every value is finite at the end; from one
start over --digest-clocks clocks, z, every w_i and every record (S, K, scale,
flags and the counts added) carry the sequence's digest.  Reported, not gating:
the speed-ups beside the byte ratios, and each new kernel's excess over
plain_fused beside the SMA policies' excess over sma_plain.

Usage: python scripts/bench_step_and_synchronise_elastic_policies.py [--replicas 8] [--steps 20] [--batches 5]
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

POLICIES = ("variables", "clipped", "clipped_variables")
KINDS = ("sequence", "fused", "discard", "seam_fused", "seam_discard")
NEW_KINDS = KINDS[1:]
SMA_FORMS = ("sma_plain", "sma_variables", "sma_clipped", "sma_clipped_variables")
FORMS = tuple(f"{p}_{k}" for p in POLICIES for k in KINDS) + ("plain_fused",) + SMA_FORMS
LR, ALPHA, MOMENTUM, WD = 0.05, 0.1, 0.9, 1e-4
BN_MULTIPLIER = 2.0


def split(form):
    """(policy, kind) of a form of the elastic context or the seam."""
    for p in sorted(POLICIES, key=len, reverse=True):
        if form.startswith(p + "_"):
            return p, form[len(p) + 1:]
    return None, form


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

    from crossbow_amd import BUF_DATA, BUF_GRADIENT, BUF_LAST, SYNC_BSP, UPDATE_SMA, UPDATE_SYNCHRONOUSEAMSGD, TheGPU
    from crossbow_amd._abi import STEP_DISCARD_TASK_OUTPUTS
    from crossbow_amd.build import (CLIPPED_LIB, CLIPPED_VARIABLES_LIB, ELASTIC_POLICIES_LIB, ELASTIC_STEPS_LIB, LIB,
                                    SSGD_STEPS_LIB, VARIABLES_LIB, code_object_digest)
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
    R = args.replicas

    def context(update_type, elastic):
        c = TheGPU()
        c.init([0])
        n_ = register(c, shapes)
        for k in bn:
            c.setModelVariableLearningRateMultiplier(k, 1, BN_MULTIPLIER)
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
        unit = O.fill_normal(n, 77, 0.01)
        grads = [(unit * np.float32(0.5 + i / 8.0)).astype(np.float32) for i in range(R)]
        max_norm = float(np.float32(0.9 * np.sqrt(float(np.dot(unit.astype(np.float64), unit.astype(np.float64))))))
        side = torch.cuda.Stream()
        state = {"task": 0, "clock": 0, "sma_clock": 0}
        on = {id(g): None, id(sma): None}  # (clipping, variable rates) as last set on each context

        # the seam's buffers: exactly n floats each, on a stream of the caller's
        plan = SmaPlan([0], n)
        plan.set_variables(var_elements, mults)
        dev_grads = [torch.from_numpy(a).cuda() for a in grads]
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
                c.replica_write(i, BUF_GRADIENT, grads[i])
                c.replica_write(i, BUF_LAST, unit)
            c.wait()

        def seam_start():
            """The context's start, copied into the caller-owned buffers."""
            start()
            sz.copy_(torch.from_numpy(g.base_read(0, BUF_DATA)))
            for i in range(R):
                sw[i].copy_(torch.from_numpy(g.replica_read(i, BUF_DATA)))
                ss[i].zero_()
                sg[i].copy_(dev_grads[i])
                sl[i].copy_(torch.from_numpy(unit))
            torch.cuda.synchronize()

        def features(c, clip, rates):
            """The setters are called where a form differs from the one before it on that context only."""
            if (clip, rates) != on[id(c)]:
                c.set_gradient_clip(max_norm if clip else 0.0, clip)
                c.set_variable_learning_rates(rates)
                on[id(c)] = (clip, rates)

        def clock_iteration(form):
            policy, kind = split(form)
            discard = STEP_DISCARD_TASK_OUTPUTS if kind.endswith("discard") else 0
            clip = policy in ("clipped", "clipped_variables") or form in ("sma_clipped", "sma_clipped_variables")
            rates = policy in ("variables", "clipped_variables") or form in ("sma_variables", "sma_clipped_variables")
            if kind.startswith("seam"):
                reps = [(0, sw[i].data_ptr(), ss[i].data_ptr(), sg[i].data_ptr(), sl[i].data_ptr(), 1, 1, LR)
                        for i in range(R)]
                plan.elastic_step_and_optimise_clipped_variables(
                    [seam_stream.cuda_stream], [sz.data_ptr()], reps, ALPHA, MOMENTUM, WD, 0, discard,
                    slots=list(range(R)) if clip else None, max_norm=max_norm, skip_nonfinite=True, use_variables=rates)
                return
            tasks = list(range(state["task"], state["task"] + R))
            state["task"] += R
            if form in SMA_FORMS:
                features(sma, clip, rates)
                state["sma_clock"] += 1
                sma.lockAny()
                sma.step_and_synchronise_clipped_variables(0, state["sma_clock"], 0, tasks, None, 0)
                sma.unlockAny()
                return
            features(g, clip, rates)
            state["clock"] += 1
            if kind == "sequence":
                for i in range(R):
                    g.replica_optimise(i, tasks[i])
                g.lockAny()
                g.synchronise(0, state["clock"], 0, False)
                g.unlockAny()
                return
            g.lockAny()
            if form == "plain_fused":
                g.step_and_synchronise_elastic(0, state["clock"], 0, tasks, None, 0)
            else:
                g.step_and_synchronise_elastic_clipped_variables(0, state["clock"], 0, tasks, None, discard)
            g.unlockAny()

        def mark(form):
            """An event behind the end of the last step."""
            e = torch.cuda.Event(enable_timing=True)
            if split(form)[1].startswith("seam"):
                e.record(seam_stream)
                return e
            c = sma if form in SMA_FORMS else g
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

        def records(form):
            policy, kind = split(form)
            if policy == "variables":
                return None
            if kind.startswith("seam"):
                return [plan.clip_stats(0, i, seam_stream.cuda_stream) for i in range(R)]
            return [g.replica_clip_stats(i) for i in range(R)]

        def digest(form, before):
            h = hashlib.sha256()
            if split(form)[1].startswith("seam"):
                for t in [sz] + sw:
                    h.update(t.cpu().numpy().tobytes())
            else:
                h.update(g.base_read(0, BUF_DATA).tobytes())
                for i in range(R):
                    h.update(g.replica_read(i, BUF_DATA).tobytes())
            after = records(form)
            if after is not None:  # what the run left in every record, and the counts it added
                for a, b in zip(after, before):
                    row = [a["sum_sq"], a["nonfinite"], a["scale"], a["flags"]] + \
                          [a[k] - b[k] for k in ("steps", "clipped_steps", "skipped_steps")]
                    h.update(json.dumps(row).encode())
            return h.hexdigest()

        def digest_run(form):
            policy, kind = split(form)
            seam = kind.startswith("seam")
            (seam_start if seam else start)()
            if not seam:
                features(g, policy in ("clipped", "clipped_variables"), policy in ("variables", "clipped_variables"))
            elif policy != "variables":  # the slots exist before they are read
                for i in range(R):
                    plan.gradient_norm(0, i, seam_stream.cuda_stream, sg[i].data_ptr(), max_norm, True)
            before = records(form)
            for _ in range(args.digest_clocks):
                for i in range(R):
                    if seam:
                        sg[i].copy_(dev_grads[i])
                    else:
                        g.replica_write(i, BUF_GRADIENT, grads[i])
                torch.cuda.synchronize()
                clock_iteration(form)
                g.wait()
                torch.cuda.synchronize()
            return digest(form, before)

        digests = {f"{p}_{k}": digest_run(f"{p}_{k}") for p in POLICIES for k in KINDS}
        clipped_steps = [g.replica_clip_stats(i)["clipped_steps"] for i in range(R)]

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

        base, reps = g.modelStats(BUF_DATA)
        finite = int(base["nonfinite"].sum()) == 0 and int(reps["nonfinite"].sum()) == 0
        finite = finite and bool(torch.isfinite(sz).all()) and all(bool(torch.isfinite(t).all()) for t in sw)
        copy_GBs = g.bench_copy(4 * n, 20)

        def nbytes(policy, kind):
            per = {"sequence": 36, "fused": 28, "discard": 20, "seam_fused": 28, "seam_discard": 20}[kind]
            return (per * R + 8) * n + (4 * R * n if policy != "variables" else 0)  # the norm passes read g once more
        bytes_per = {f"{p}_{k}": nbytes(p, k) for p in POLICIES for k in KINDS}
        bytes_per["plain_fused"] = (28 * R + 8) * n
        for f in SMA_FORMS:
            bytes_per[f] = (28 * R + 16) * n + (4 * R * n if "clipped" in f else 0)
        med = {f: statistics.median(ms[f]) for f in FORMS}
        line = {
            "metric": "clipped and per-variable task steps fused into the one-GPU elastic-averaging barrier against "
                      "the two-call sequence, per clock",
            "model": args.model, "elements": n, "variables": len(shapes), "irregular_variables": len(bn),
            "multiplier": BN_MULTIPLIER, "replicas": R, "alpha": ALPHA, "momentum": MOMENTUM, "weight_decay": WD,
            "max_norm": max_norm, "clipped_steps_per_replica_after_the_digest_runs": [int(x) for x in clipped_steps],
            "steps_per_batch": args.steps, "batches": args.batches, "warmup": args.warmup,
            "bytes_per_clock": bytes_per, "copy_ceiling_GBs": round(copy_GBs, 1), "finite_at_the_end": finite,
            "digest_clocks": args.digest_clocks,
            "digests_equal_sequence": {f"{p}_{k}": digests[f"{p}_{k}"] == digests[f"{p}_sequence"]
                                       for p in POLICIES for k in NEW_KINDS},
            "policies_digests_differ": len({digests[f"{p}_sequence"] for p in POLICIES}) == len(POLICIES),
        }
        for f in FORMS:
            line[f + "_ms"] = round(med[f], 5)
            line[f + "_batches_ms"] = [round(x, 5) for x in ms[f]]
            line[f + "_spread"] = round(spread(ms[f]), 5)
            line[f + "_GBs_per_clock"] = round(bytes_per[f] / (med[f] * 1e-3) / 1e9, 1)
        faster = {}
        for p in POLICIES:
            seq = f"{p}_sequence"
            for k in NEW_KINDS:
                f = f"{p}_{k}"
                line[f + "_speedup"] = round(med[seq] / med[f], 4)
                line[f + "_byte_ratio"] = round(bytes_per[seq] / bytes_per[f], 4)
                faster[f] = bool(max(ms[f]) < min(ms[seq]))
            # reported: the kernel's excess over the plain fused elastic kernel, norm passes included where it clips,
            # beside the same policy's excess over the plain fused SMA kernel
            line[p + "_excess_over_plain_fused"] = round(med[f"{p}_fused"] / med["plain_fused"], 4)
            line["sma_" + p + "_excess_over_sma_plain"] = round(med["sma_" + p] / med["sma_plain"], 4)
        line["faster_in_every_batch"] = faster
        line["pass"] = bool(finite and all(faster.values()) and all(line["digests_equal_sequence"].values()))
        line["code_object_digest"] = code_object_digest(LIB)
        line["variables_code_object_digest"] = code_object_digest(VARIABLES_LIB)
        line["clipped_code_object_digest"] = code_object_digest(CLIPPED_LIB)
        line["clipped_variables_code_object_digest"] = code_object_digest(CLIPPED_VARIABLES_LIB)
        line["elastic_steps_code_object_digest"] = code_object_digest(ELASTIC_STEPS_LIB)
        line["ssgd_steps_code_object_digest"] = code_object_digest(SSGD_STEPS_LIB)
        line["elastic_policies_code_object_digest"] = code_object_digest(ELASTIC_POLICIES_LIB)
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
