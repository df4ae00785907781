"""Which compiled kernel instantiation does a call reach?

The library compiles some 1,600 device kernels, nearly all of them template
instantiations picked by hand-written ``switch`` ladders and ``if / else``
chains.  This module is the suite's account of them:

``CASES``         one call through a public door each (the context through
                  ``TheGPU``, the seam through ``SmaPlan``), with everything
                  the dispatch looks at.  tests/test_gpu_instantiations.py
                  runs every one against the oracle, bit for bit.
``expected_kernels(case, num_cus)``
                  the dispatch restated in Python: the demangled names of the
                  instantiations the call launches.
``UNREACHABLE``   instantiations no door can produce, with the line that says so.
``ELSEWHERE``     kernels this table does not drive, with the test that runs them.
``UNTESTED``      the two copy kernels of the copy-ceiling measurement: no test
                  runs them, and the list says so.
``INCIDENTAL``    the ELSEWHERE kernels that a case launches on its way (the
                  norm pass in front of a clipped step).

tests/test_instantiations.py keeps the sets an exact, disjoint cover of what
the library compiles.  Plain Python: no torch, no GPU.

Line numbers are those of crossbow_amd/csrc at the commit that added this file.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, List, Tuple

K_PAD_FLOAT4 = 1024     # sma_internal.h:55: the context pads every buffer to whole kPadFloat4s
K_TAIL_QUANTUM4 = 256   # sma_seam.hip:65-67: the seam's bulk is whole kTailQuantum4s, the rest is the tail
K_CHUNK = 8             # sma_internal.h:14
CTX_REPLICAS = 9        # one context of 9 replicas reaches R = 9 (the chunked form) .. 0 through `first`


STUB = "__device_stub__"


def normalise(symbol: str) -> str:
    """`void cbx::(anonymous namespace)::__device_stub__k<1, true>(cbx::SmaArgs)` -> `k<1, true>`;
    a traced `void cbx::(anonymous namespace)::k<1, true>(cbx::SmaArgs)` likewise."""
    s = symbol.strip()
    s = re.sub(r"\s+\[clone [^\]]*\]$", "", s)
    s = re.sub(r"\.kd$", "", s)
    depth, cut = 0, len(s)
    for k in range(len(s) - 1, -1, -1):  # drop the parameter list: the last top-level (...)
        ch = s[k]
        if ch == ")":
            depth += 1
        elif ch == "(":
            depth -= 1
            if depth == 0:
                cut = k
                break
        elif depth == 0 and ch not in " &*" and not s[k:].startswith("const"):
            break
    s = s[:cut] if s.endswith(")") else s
    s = re.sub(r"^(void|static void)\s+", "", s)
    s = s.replace("(anonymous namespace)::", "").replace(STUB, "")
    s = re.sub(r"^cbx::", "", s)
    s = re.sub(r"\s*,\s*", ", ", s)
    s = re.sub(r"<\s+", "<", s)
    s = re.sub(r"\s+>", ">", s)
    return re.sub(r"\(int\)|\(bool\)", "", s)


def _b(v: bool) -> str:
    return "true" if v else "false"


@dataclass(frozen=True)
class Case:
    """One call.  ``cfg`` is (block, blocks_per_cu, unroll, waves_per_cu) of the
    launch configuration the family's main kernel takes, as the setters leave
    it (None: the default, untouched); ``apply_cfg`` is (block, unroll,
    waves_per_cu) of kernel B of a split step."""
    family: str            # "sma" | "task_barrier" | "elastic" | "polyak": the barriers; the task steps "optimise"
                           # (SMA's), "optimise_vars" (with per-variable rates), "default_task", "ssgd_task";
                           # the barriers "ssgd" and "default_sync"
    door: str              # "context" | "seam"
    n: object              # floats, or "ragged" / "seam_u2": a rule of the device's CU count (elements())
    nrep: int              # participating replicas (context: the last nrep of CTX_REPLICAS, through `first`)
    form: str = "fused"    # "fused" | "split" (cbx_set_force_split, all-reduce) | "rsag" (reduce-scatter form)
                           # | "staged" / "staged_split": cbx_synchronise_staged through the zero-copy kernels
    base_mom: bool = False     # base-model momentum on (Polyak-Ruppert: base->last exists)
    copy: bool = False         # a participating replica asks for a copy (Polyak-Ruppert: is flagged)
    steps: str = "none"        # task barrier: "all" | "some" | "none" of the participating replicas step
    rep_mom: bool = False      # task barrier: the stepping replicas' momentum
    wd: bool = False           # task barrier: their weight decay
    keep: bool = True          # task barrier: False = CBX_STEP_DISCARD_TASK_OUTPUTS
    alpha0: bool = False       # Polyak-Ruppert: alpha == 0, the replicas are not moved
    clip: bool = False         # the task step: gradient clipping on (cbx_set_gradient_clip / optimise_clipped)
    policy: int = 1
    cfg: object = None
    apply_cfg: object = None

    def elements(self, num_cus: int) -> int:
        if self.n == "ragged":
            # 12 * CUs one-wave trips of float4s: between the 8 * CUs blocks of
            # small_launch_shape's grid and the 16 * CUs waves from which it
            # leaves the shape alone, so a third of the blocks make a second trip.
            return 4 * (12 * num_cus * 64) - 2045
        if self.n == "seam_u2":
            # the smallest caller-owned buffer whose bulk small_launch_shape leaves at unroll 2
            # (sma_internal.h:182-183: ceil(n4 / 128) >= 16 * CUs), plus a 3-float tail
            n4 = ((16 * num_cus - 1) * 128 + 1 + K_TAIL_QUANTUM4 - 1) // K_TAIL_QUANTUM4 * K_TAIL_QUANTUM4
            return 4 * n4 + 3
        return int(self.n)

    def name(self) -> str:
        parts = [self.family, self.door, self.form, f"n={self.n}", f"nrep={self.nrep}"]
        for f in ("base_mom", "copy", "rep_mom", "wd", "alpha0", "clip"):
            if getattr(self, f):
                parts.append(f)
        if self.family == "task_barrier":
            parts += [f"steps={self.steps}", "keep" if self.keep else "discard"]
        parts.append(f"P={self.policy}")
        if self.cfg:
            parts.append("cfg=%s" % (self.cfg,))
        if self.apply_cfg:
            parts.append("apply=%s" % (self.apply_cfg,))
        return " ".join(parts)


# ---------------------------------------------------------------------------
# The dispatch, restated.
# ---------------------------------------------------------------------------
class Refused(Exception):
    """The launcher returns hipErrorInvalidValue for this configuration."""


def bulk_float4s(case: Case, num_cus: int) -> int:
    n = case.elements(num_cus)
    if case.door == "context":  # context.hip:480
        return ((n + 3) // 4 + K_PAD_FLOAT4 - 1) // K_PAD_FLOAT4 * K_PAD_FLOAT4
    return (n // 4) // K_TAIL_QUANTUM4 * K_TAIL_QUANTUM4  # sma_seam.hip:67


def has_tail(case: Case, num_cus: int) -> bool:
    # sma_seam.hip with_tail: [4 * bulk, n); the context's padded buffers have none
    return case.door == "seam" and case.elements(num_cus) > 4 * bulk_float4s(case, num_cus)


def small_launch_shape(block: int, blocks_per_cu: int, unroll: int, waves_per_cu: int, n4: int, num_cus: int) -> int:
    """The unroll a launcher that calls small_launch_shape ends up with (sma_internal.h:180-188)."""
    if waves_per_cu >= 0 or blocks_per_cu != 0 or block != 64:  # :181
        return unroll
    waves = (n4 + 64 * unroll - 1) // (64 * unroll)  # :182
    if waves >= 16 * num_cus:  # :183
        return unroll
    return 1  # :185


def _ladder(nrep: int, rungs) -> int:
    return nrep if nrep in rungs else -1


def _unroll_tail(u: int, tail: bool, allow4: bool) -> int:
    """The `if (cfg.unroll == ...)` chains behind every launcher."""
    if tail:  # e.g. sma_kernels.hip:924-929: a tail launch has unroll 2 or 1, else hipErrorInvalidValue
        if u not in (1, 2):
            raise Refused(f"unroll {u} with a tail")
        return u
    if allow4:  # sma_kernels.hip:934-939: 4, 2, else 1
        return u if u in (4, 2) else 1
    return u


# The default launch configurations (block, blocks_per_cu, unroll, waves_per_cu).
SMA_CFG = (64, 0, 2, -1)            # sma_internal.h:59-72: LaunchConfig's own defaults
APPLY_CFG = (64, 2, -1)             # sma_internal.h:104-110: sma_apply_launch_config (block, unroll, waves)
AVERAGING_CFG = (64, 0, 1, -1)      # sma_internal.h:128-134
TASK_BARRIER_CFG = (64, 0, 1, -1)   # sma_internal.h:380-386
AUX_CFG = (64, 0, 1, -1)            # sma_internal.h:82-88: the task steps, both doors
BROADCAST_CFG = (256, 0, 1, 8)      # sma_internal.h:95-101
SSGD_APPLY_CFG = (64, 0, 2, 3)      # sma_internal.h:135-141, both doors
STAGED_CFG = (64, 4, 2, 0)          # sma_internal.h:114-121; context_internal.h:559 is its one use: no setter
N_VARS = 21523                      # the floats of tests/test_optimise_plan.py's seven variables V


def _main_cfg(case: Case):
    if case.cfg is not None:
        if case.door == "seam":
            raise ValueError("the seam has no launch-configuration setter")
        return case.cfg
    return {"sma": SMA_CFG, "task_barrier": TASK_BARRIER_CFG, "elastic": AVERAGING_CFG, "polyak": AVERAGING_CFG,
            "optimise": AUX_CFG, "optimise_vars": AUX_CFG, "default_task": AUX_CFG, "ssgd_task": AUX_CFG, "ssgd": SSGD_APPLY_CFG,
            "default_sync": BROADCAST_CFG}[case.family]


def _policy(case: Case) -> int:
    if case.door == "seam" and case.policy != 1:
        raise ValueError("the seam's plan keeps policy 1")
    return case.policy


def _sma_fused(case: Case, num_cus: int) -> str:
    block, bpc, unroll, waves = _main_cfg(case)
    n4, tail, P = bulk_float4s(case, num_cus), has_tail(case, num_cus), _policy(case)
    R = _ladder(case.nrep, range(0, K_CHUNK + 1))  # fused_r, sma_kernels.hip:945-956
    u = small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # fused_u, :914
    if tail and P != 1:
        raise Refused("a tail needs policy 1")  # :918-919
    U = _unroll_tail(u, tail, allow4=True)  # :924-939
    return f"sma_fused_kernel<{R}, {_b(case.base_mom)}, {_b(case.copy)}, {P}, {_b(tail)}, {U}>"  # launch_sma_fused, :1163-1171


def _sma_split(case: Case, num_cus: int) -> List[str]:
    block, bpc, unroll, waves = _main_cfg(case)
    ablock, aunroll, awaves = case.apply_cfg if case.apply_cfg is not None else APPLY_CFG
    n4, P = bulk_float4s(case, num_cus), _policy(case)  # one rank, no bucket size set: one bucket (bucket_pipeline.h:80-89)
    if case.door != "context":
        raise ValueError("a one-rank plan never splits (sma_seam.hip:477-485)")
    R = _ladder(case.nrep, range(0, K_CHUNK + 1))  # acc_r, sma_kernels.hip:992-1003
    u = _unroll_tail(small_launch_shape(block, bpc, unroll, waves, n4, num_cus), False, allow4=True)  # acc_u, :961, :981-986
    names = [f"sma_accumulate_kernel<{R}, {P}, false, {u}>"]
    rsag = case.form == "rsag"
    if rsag and case.base_mom:
        names.append(f"sma_shard_momentum_kernel<{P}>")  # sync_steps.hip:1052-1058; launch_sma_shard_momentum, sma_kernels.hip:1211-1220
    # kernel B takes apply_cfg (sync_steps.hip:1135) with the shared policy (context.hip:2079);
    # the reduce-scatter form has applied the momentum on the shard already (:1169)
    au = _unroll_tail(small_launch_shape(ablock, 0, aunroll, awaves, n4, num_cus), False, allow4=True)  # apply_u, :1008, :1028-1033
    names.append(f"sma_apply_kernel<{_b(case.base_mom and not rsag)}, {P}, false, {au}>")
    return names


def _task_barrier(case: Case, num_cus: int) -> str:
    block, bpc, unroll, waves = _main_cfg(case)
    n4, tail, P = bulk_float4s(case, num_cus), has_tail(case, num_cus), _policy(case)
    if case.steps != "none" and case.nrep == 0:
        raise ValueError("nobody to step")
    stepping = case.steps != "none"
    mom = case.rep_mom and stepping  # context.hip:775, sma_seam.hip:561: the first stepping replica's, else 0
    wd = case.wd and stepping        # context.hip:776, sma_seam.hip:562
    # the ladders are task_barrier_launch.h's, named here by function (the three barrier objects share them): tb_form
    if case.nrep > 0 and case.steps == "all" and case.base_mom == mom:
        R, mixed, bmom = _ladder(case.nrep, range(1, K_CHUNK + 1)), False, mom  # tb_form's switch
    else:
        R, mixed, bmom = -1, True, case.base_mom  # tb_form's last return
    u = small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # tb_u
    if tail and P != 1:
        raise Refused("a tail needs policy 1")  # task_barrier_compiled
    if u not in (1, 2):
        raise Refused(f"unroll {u}")  # tb_u
    return (f"task_barrier_kernel<{R}, {_b(mixed)}, {_b(mom)}, {_b(bmom)}, {_b(wd)}, {_b(case.keep)}, {P}, "
            f"{_b(tail)}, {u}>")  # tb_conf / task_barrier_launch


def _averaging(case: Case, num_cus: int) -> List[str]:
    block, bpc, unroll, waves = _main_cfg(case)
    n4, tail, P = bulk_float4s(case, num_cus), has_tail(case, num_cus), _policy(case)
    polyak = case.family == "polyak"
    model = 2 if polyak else 0  # one rank: kElasticW (sync_steps.hip:1764, sma_seam.hip:232)
    last = polyak and case.base_mom  # sync_steps.hip:1783, sma_seam.hip:262
    R = _ladder(case.nrep, range(1, K_CHUNK + 1))  # avg_r, averaging_kernels.hip:282-292 (0 goes to the chunked form)
    u = small_launch_shape(block, bpc, unroll, waves, n4, num_cus)  # avg_u, :232
    if tail and P != 1:
        raise Refused("a tail needs policy 1")  # :256-257
    U = _unroll_tail(u, tail, allow4=True)  # :262-276
    if case.form == "fused":  # launch_averaging_fused, :307-311
        return [f"averaging_kernel<{model}, 0, {R}, {_b(last)}, {P}, {_b(tail)}, {U}>"]
    if case.door != "context":
        raise ValueError("a one-rank plan never splits (sma_seam.hip:273-279)")
    # launch_averaging_accumulate, :313-321: no LAST form; launch_averaging_apply, :323-326: both
    # elastic forms apply as kElasticW, R = 0 (avg_p, :298-299), apply_cfg with the shared policy
    ablock, aunroll, awaves = case.apply_cfg if case.apply_cfg is not None else APPLY_CFG
    au = _unroll_tail(small_launch_shape(ablock, 0, aunroll, awaves, n4, num_cus), False, allow4=True)
    return [f"averaging_kernel<{model}, 1, {R}, false, {P}, false, {U}>",
            f"averaging_kernel<{model}, 2, 0, {_b(last)}, {P}, false, {au}>"]


def _sma_staged(case: Case) -> List[str]:
    """cbx_synchronise_staged in the zero-copy mode (the default; sync_steps.hip:1377-1519): staged_cfg has
    no setter, its unroll stays 2, and the staged launchers do not call small_launch_shape."""
    if case.door != "context" or case.cfg is not None or case.policy != 1:
        raise ValueError("the staged step is the context's, with no setter for its shape or policy")
    U = 2 if STAGED_CFG[2] == 2 else 1  # sma_kernels.hip:1077-1080, :1099-1102, :1109-1112
    R = _ladder(case.nrep, (0, 1, 2, 4, 8))  # fused_staged_r, :1086-1093; launch_sma_accumulate_staged, :1128-1135
    if case.form == "staged":  # one device, not forced to split: one launch (sync_steps.hip:1379, :1463-1473)
        return [f"sma_fused_staged_kernel<{R}, {_b(case.base_mom)}, {_b(case.copy)}, {U}>"]  # :1118-1122
    return [f"sma_accumulate_staged_kernel<{R}, {U}>",
            f"sma_apply_staged_kernel<{_b(case.base_mom)}, {U}>"]  # launch_sma_apply_staged, :1138-1141


def _task_side(case: Case, num_cus: int) -> str:
    """The task steps and the two small barriers: no ladder and no small_launch_shape, the
    configured unroll as it stands (CBX_LAUNCH_U / CBX_LAUNCH_TAIL, sma_kernels.hip:1225-1233,
    :1314-1332; optimise_p, :1236-1261).  No setter touches the policy of their configurations
    (context.hip:2093-2119; cbx_set_kernel_config shares it with kernel B, the averaging and the
    task-barrier shapes only, :2078-2081), and the seam's are the defaults: policy 1 throughout."""
    if case.policy != 1:
        raise ValueError("no door sets a policy for this family")
    _, bpc, unroll, _ = _main_cfg(case)
    tail = has_tail(case, num_cus)
    if unroll not in (1, 2) or bpc != 0:
        raise ValueError("the setters take unroll 1 or 2 (context.hip:2096, :2109)")
    mom, wd, U = _b(case.rep_mom), _b(case.wd), unroll
    if case.family == "optimise":  # optimise_c, :1264-1272; launch_sma_optimise(_clipped), :1274-1282
        return f"sma_optimise_kernel<{mom}, {wd}, 1, {_b(tail)}, {U}, {_b(case.clip)}>"
    if case.family == "optimise_vars":  # variables_p / variables_c, variable_rate_kernels.hip:163-207: no TAIL form
        return f"sma_optimise_variables_kernel<{mom}, {wd}, 1, {U}, {_b(case.clip)}>"
    if case.family == "default_task":  # launch_default_optimise, :1291-1299
        return f"default_optimise_kernel<{mom}, {wd}, 1, {U}>"
    if case.family == "ssgd_task":  # launch_ssgd_accumulate, :1343-1347
        return f"ssgd_accumulate_kernel<{wd}, 1, {_b(tail)}, {U}>"
    if case.family == "ssgd":  # launch_ssgd_apply, :1358-1362
        return f"ssgd_apply_kernel<{_b(case.base_mom)}, 1, {_b(tail)}, {U}>"
    return f"broadcast_kernel<1, {U}>"  # launch_broadcast, :1308-1310


def expected_kernels(case: Case, num_cus: int) -> Tuple[str, ...]:
    """The demangled instantiations the call launches, in launch order."""
    if case.family in ("optimise", "optimise_vars", "default_task", "ssgd_task", "ssgd", "default_sync"):
        return (_task_side(case, num_cus),)
    if case.family == "sma" and case.form in ("staged", "staged_split"):
        return tuple(_sma_staged(case))
    if case.family == "sma":
        return (_sma_fused(case, num_cus),) if case.form == "fused" else tuple(_sma_split(case, num_cus))
    if case.family == "task_barrier":
        return (_task_barrier(case, num_cus),)
    if case.family in ("elastic", "polyak"):
        return tuple(_averaging(case, num_cus))
    raise ValueError(case.family)


def expected_kernel(case: Case, num_cus: int) -> str:
    """The instantiation of the call's main kernel (a split step's kernel A)."""
    return expected_kernels(case, num_cus)[0]


# ---------------------------------------------------------------------------
# The cases.
# ---------------------------------------------------------------------------
N_CTX = 4099           # two kPadFloat4 pads, the last float4 only partly inside n
N_SEAM = (1027, 64 * 2 * 4 * 5 + 259)  # one bulk quantum + 3 floats; two quanta + 771 floats (4 blocks of 256, 13 of 64)
N_TAIL_ONLY = 771  # below the seam's quantum of 1,024 floats: an empty bulk (n4 == 0), 13 tail blocks of 64
R_ALL = (9, 8, 7, 6, 5, 4, 3, 2, 1, 0)
# A shape per unroll, each of which leaves auto mode (block != 64 or waves_per_cu >= 0):
# (block, blocks_per_cu, unroll, waves_per_cu); block * unroll divides kPadFloat4.
FORCED = {1: (256, 0, 1, 0), 2: (64, 0, 2, 0), 4: (128, 0, 4, 2)}
FORCED_APPLY = {1: (256, 1, 0), 2: (64, 2, 0), 4: (128, 4, 2)}
TB_FORCED = {1: (256, 0, 1, 0), 2: (64, 0, 2, 2)}


def _sma_cases() -> List[Case]:
    out = []
    for nrep in R_ALL:
        for mom in (False, True):
            for copy in (False, True):
                if copy and nrep == 0:
                    continue  # nobody to ask for a copy: see UNREACHABLE
                for P in (0, 1):
                    for U in (1, 2, 4):
                        out.append(Case("sma", "context", N_CTX, nrep, base_mom=mom, copy=copy, policy=P, cfg=FORCED[U]))
                for n in N_SEAM + (N_TAIL_ONLY,):
                    out.append(Case("sma", "seam", n, nrep, base_mom=mom, copy=copy))
                out.append(Case("sma", "seam", "seam_u2", nrep, base_mom=mom, copy=copy))
        # the default configuration, rewritten by small_launch_shape at this n
        out.append(Case("sma", "context", N_CTX, nrep, base_mom=True))
    # a caller-owned buffer of whole quanta has no tail: the context's instantiations
    out.append(Case("sma", "seam", 2048, 3, base_mom=True))
    # ragged trip counts of the grid-stride loop (auto mode, and one block per CU)
    out.append(Case("sma", "context", "ragged", 2, base_mom=True))
    out.append(Case("sma", "context", "ragged", 2, base_mom=True, cfg=(64, 1, 2, -1)))
    # the host-staged step through the zero-copy kernels: their own ladder {0, 1, 2, 4, 8, -1}
    for nrep in (9, 8, 4, 2, 1, 0):
        for mom in (False, True):
            for copy in (False, True):
                if not (copy and nrep == 0):
                    out.append(Case("sma", "context", N_CTX, nrep, form="staged", base_mom=mom, copy=copy))
            if mom == (nrep % 2 == 0) or nrep == 4:
                out.append(Case("sma", "context", N_CTX, nrep, form="staged_split", base_mom=mom, copy=nrep == 8))
    out.append(Case("sma", "context", N_CTX, 3, form="staged", base_mom=True))  # a count between the rungs
    # kernels A and B of the split path on one rank
    for nrep in R_ALL:
        for P in (0, 1):
            for U in (1, 2, 4):
                mom = (nrep + U) % 2 == 0
                out.append(Case("sma", "context", N_CTX, nrep, form="split", base_mom=mom, copy=nrep in (9, 4, 1),
                                policy=P, cfg=FORCED[U], apply_cfg=FORCED_APPLY[U]))
    for mom in (False, True):
        for P in (0, 1):
            for U in (1, 2, 4):
                out.append(Case("sma", "context", N_CTX, 3, form="split", base_mom=mom, copy=U == 2, policy=P,
                                cfg=FORCED[2], apply_cfg=FORCED_APPLY[U]))
            out.append(Case("sma", "context", N_CTX, 3, form="rsag", base_mom=mom, policy=P, cfg=FORCED[2],
                            apply_cfg=FORCED_APPLY[1]))
    out.append(Case("sma", "context", "ragged", 2, form="split", base_mom=True))
    return out


def _task_barrier_cases() -> List[Case]:
    out = []
    for rep_mom in (False, True):
        for wd in (False, True):
            for keep in (True, False):
                # every replica steps, base momentum as theirs (what the setters produce): tb_all
                for nrep in R_ALL[:-1]:
                    for P in (0, 1):
                        for U in (1, 2):
                            out.append(Case("task_barrier", "context", N_CTX, nrep, base_mom=rep_mom, steps="all",
                                            rep_mom=rep_mom, wd=wd, keep=keep, copy=nrep == 5, policy=P, cfg=TB_FORCED[U]))
                    out.append(Case("task_barrier", "seam", N_SEAM[nrep % 2], nrep, base_mom=rep_mom, steps="all",
                                    rep_mom=rep_mom, wd=wd, keep=keep, copy=nrep == 6))
                    if nrep in (9, 8, 3):
                        out.append(Case("task_barrier", "seam", N_TAIL_ONLY, nrep, base_mom=rep_mom, steps="all",
                                        rep_mom=rep_mom, wd=wd, keep=keep, copy=nrep == 3))
                # some step, and base momentum unlike theirs: tb_mixed
                for base_mom in (False, True):
                    for steps in ("some", "all"):
                        if steps == "all" and base_mom == rep_mom:
                            continue  # that is tb_all
                        # A context has base->last iff its replicas were made with momentum
                        # (context.hip:485, :519): base momentum without theirs has no context door.
                        if not (base_mom and not rep_mom):
                            for P in (0, 1):
                                for U in (1, 2):
                                    out.append(Case("task_barrier", "context", N_CTX, 4, base_mom=base_mom, steps=steps,
                                                    rep_mom=rep_mom, wd=wd, keep=keep, policy=P, cfg=TB_FORCED[U]))
                        out.append(Case("task_barrier", "seam", N_SEAM[steps == "all"], 9 if steps == "some" else 3,
                                        base_mom=base_mom, steps=steps, rep_mom=rep_mom, wd=wd, keep=keep,
                                        copy=steps == "some"))
                        if steps == "some":
                            out.append(Case("task_barrier", "seam", N_TAIL_ONLY, 9, base_mom=base_mom, steps=steps,
                                            rep_mom=rep_mom, wd=wd, keep=keep))
                        if base_mom and not rep_mom:
                            # without a tail the seam launches the context's form (policy 1, unroll 1)
                            out.append(Case("task_barrier", "seam", 2048, 4, base_mom=True, steps=steps, rep_mom=False,
                                            wd=wd, keep=keep))
    # nobody steps: the barrier alone, through the mixed form; nobody at all
    for base_mom in (False, True):
        for keep in (True, False):
            for nrep in (3, 0):
                for P in (0, 1):
                    for U in (1, 2):
                        out.append(Case("task_barrier", "context", N_CTX, nrep, base_mom=base_mom, steps="none",
                                        rep_mom=True, wd=True, keep=keep, policy=P, cfg=TB_FORCED[U]))
                out.append(Case("task_barrier", "seam", N_SEAM[0], nrep, base_mom=base_mom, steps="none", keep=keep))
    # the default configuration (its ragged trip counts at a larger n are
    # tests/test_gpu_step_and_synchronise.py::test_grid_stride_shape_bitexact's, not repeated here)
    out.append(Case("task_barrier", "context", N_CTX, 9, base_mom=True, steps="all", rep_mom=True, wd=True))
    return out


def _averaging_cases() -> List[Case]:
    out = []
    for family, lasts in (("elastic", (False,)), ("polyak", (False, True))):
        for last in lasts:
            for nrep in R_ALL:
                copy = family == "polyak" and nrep in (9, 5, 2)
                alpha0 = family == "polyak" and nrep == 7
                for P in (0, 1):
                    for U in (1, 2, 4):
                        out.append(Case(family, "context", N_CTX, nrep, base_mom=last, copy=copy, alpha0=alpha0, policy=P,
                                        cfg=FORCED[U]))
                        if not last:  # kernel A has no LAST form; kernel B's two are below
                            out.append(Case(family, "context", N_CTX, nrep, form="split", base_mom=False, copy=copy,
                                            alpha0=alpha0, policy=P, cfg=FORCED[U], apply_cfg=FORCED_APPLY[U]))
                for n in N_SEAM + (N_TAIL_ONLY,):
                    out.append(Case(family, "seam", n, nrep, base_mom=last, copy=copy, alpha0=alpha0))
            out.append(Case(family, "context", N_CTX, 3, base_mom=last))  # the default configuration
            out.append(Case(family, "context", "ragged", 2, base_mom=last))
    for P in (0, 1):  # kernel B of Polyak-Ruppert with base->last
        for U in (1, 2, 4):
            out.append(Case("polyak", "context", N_CTX, 3, form="split", base_mom=True, copy=True, policy=P,
                            cfg=FORCED[2], apply_cfg=FORCED_APPLY[U]))
    out.append(Case("elastic", "context", "ragged", 2, form="split"))
    return out


def _task_side_cases() -> List[Case]:
    out = []
    shapes = (None, (128, 0, 2, 4))  # the default (unroll 1, auto occupancy) and two float4s per lane
    for cfg in shapes:
        for mom in (False, True):
            for wd in (False, True):
                out.append(Case("optimise", "context", N_CTX, 1, rep_mom=mom, wd=wd, cfg=cfg))
                out.append(Case("default_task", "context", N_CTX, 1, rep_mom=mom, wd=wd, cfg=cfg))
        for wd in (False, True):
            out.append(Case("ssgd_task", "context", N_CTX, 1, wd=wd, cfg=cfg))
    for mom in (False, True):
        for wd in (False, True):
            for clip in (False, True):
                for n in N_SEAM + (N_TAIL_ONLY, 2048):
                    out.append(Case("optimise", "seam", n, 1, rep_mom=mom, wd=wd, clip=clip))
                for cfg in shapes:
                    if clip:
                        out.append(Case("optimise", "context", N_CTX, 1, rep_mom=mom, wd=wd, clip=True, cfg=cfg))
                    # every variable with its own rate: the whole model through cbx_replica_optimise
                    out.append(Case("optimise_vars", "context", N_VARS, 1, rep_mom=mom, wd=wd, clip=clip, cfg=cfg))
                out.append(Case("optimise_vars", "seam", N_VARS, 1, rep_mom=mom, wd=wd, clip=clip))
    for wd in (False, True):
        for n in N_SEAM + (N_TAIL_ONLY,):
            out.append(Case("ssgd_task", "seam", n, 1, wd=wd))
    for mom in (False, True):
        for cfg, nrep in ((None, 9), ((256, 0, 1, 0), 3)):
            out.append(Case("ssgd", "context", N_CTX, nrep, base_mom=mom, cfg=cfg))
        for n in N_SEAM + (N_TAIL_ONLY,):
            out.append(Case("ssgd", "seam", n, 3, base_mom=mom))
    for cfg, nrep in ((None, 9), ((64, 0, 2, 4), 4)):
        out.append(Case("default_sync", "context", N_CTX, nrep, cfg=cfg))
    return out


CASES: List[Case] = _sma_cases() + _task_barrier_cases() + _averaging_cases() + _task_side_cases()


def case_names(num_cus: int):
    """{instantiation: [cases that reach it]} over CASES."""
    out: Dict[str, List[Case]] = {}
    for c in CASES:
        for k in expected_kernels(c, num_cus):
            out.setdefault(k, []).append(c)
    return out


# ---------------------------------------------------------------------------
# What no door can produce.
# ---------------------------------------------------------------------------
def _unreachable():
    """(no door reaches it, only a door of several ranks reaches it)."""
    out: Dict[str, str] = {}
    one_rank = out
    multi: Dict[str, str] = {}
    tf = ("false", "true")
    rungs = (0, 1, 2, 3, 4, 5, 6, 7, 8, -1)
    # Phase D with nobody in the step: copies are counted over the participating replicas only
    why = ("COPY is copies_total > 0, counted over the participating replicas (sync_steps.hip:20-27, "
           "sma_seam.hip:447-454): with none of them (R = 0) it is false")
    for mom in tf:
        for P, forms in ((0, ("false, 1", "false, 2", "false, 4")), (1, ("false, 1", "false, 2", "false, 4", "true, 1", "true, 2"))):
            for f in forms:
                out[f"sma_fused_kernel<0, {mom}, true, {P}, {f}>"] = why
    # kernels A and B over caller-owned buffers belong to plans of several ranks
    out = multi
    why = ("G > 1 only: a TAIL launch of kernel A or B needs a plan of several ranks (sma_seam.hip:477-486, :273-280); "
           "the family is run by tests/test_gpu_seam.py and tests/test_gpu_seam_averaging_devices.py")
    for R in rungs:
        for U in (1, 2):
            out[f"sma_accumulate_kernel<{R}, 1, true, {U}>"] = why
    for mom in tf:
        for U in (1, 2):
            out[f"sma_apply_kernel<{mom}, 1, true, {U}>"] = why
    for model, lasts in ((0, ("false",)), (2, ("false", "true"))):
        for U in (1, 2):
            for R in rungs[1:]:
                if "false" in lasts:
                    out[f"averaging_kernel<{model}, 1, {R}, false, 1, true, {U}>"] = why
            for last in lasts:
                out[f"averaging_kernel<{model}, 2, 0, {last}, 1, true, {U}>"] = why
    # the snapshot form of elastic averaging
    why = ("G > 1 only: kElasticS is chosen only with more than one rank (sync_steps.hip:1764, sma_seam.hip:232); the "
           "family is run by tests/test_gpu_averaging_multidevice.py and tests/test_gpu_seam_averaging_devices.py")
    for R in rungs[1:]:
        for P, forms in ((0, ("false, 1", "false, 2", "false, 4")), (1, ("false, 1", "false, 2", "false, 4", "true, 1", "true, 2"))):
            for f in forms:
                out[f"averaging_kernel<1, 1, {R}, false, {P}, {f}>"] = why
    # the seam's fixed unroll 1
    out = one_rank
    why = ("the seam has no launch-configuration setter and averaging_launch_config() sets unroll = 1 "
           "(sma_internal.h:128-134, sma_seam.hip:108): a TAIL launch never has unroll 2")
    for model, lasts in ((0, ("false",)), (2, ("false", "true"))):
        for last in lasts:
            for R in rungs[1:]:
                out[f"averaging_kernel<{model}, 0, {R}, {last}, 1, true, 2>"] = why
    why = ("the seam has no launch-configuration setter and task_barrier_launch_config() sets unroll = 1 "
           "(sma_internal.h:380-386, sma_seam.hip:109, :568): a TAIL launch never has unroll 2")
    for R, mixed, pairs in [(r, "false", (("false", "false"), ("true", "true"))) for r in rungs[1:]] + \
                           [(-1, "true", tuple((m, b) for m in tf for b in tf))]:
        for mom, bmom in pairs:
            for wd in tf:
                for keep in tf:
                    out[f"task_barrier_kernel<{R}, {mixed}, {mom}, {bmom}, {wd}, {keep}, 1, true, 2>"] = why
    # base momentum with stepping replicas that have none, weight decay on
    why = ("MOM = false with WD = true needs a stepping replica without momentum, BMOM = true a base->last; a context has "
           "base->last iff its replicas were made with momentum (context.hip:485, :519), so only the seam reaches this "
           "form, at policy 1 and unroll 1 (sma_seam.hip:109)")
    for keep in tf:
        for f in ("0, false, 1", "0, false, 2", "1, false, 2"):
            out[f"task_barrier_kernel<-1, true, false, true, true, {keep}, {f}>"] = why
    # the task steps and the two small barriers: policy 0, and the seam's fixed unroll
    why0 = ("no setter touches the policy of aux_cfg, broadcast_cfg or ssgd_apply_cfg (context.hip:2093-2119; "
            "cbx_set_kernel_config shares it with kernel B, the averaging and the task-barrier shapes only, :2078-2081), "
            "and the seam takes the defaults: policy 0 has no door")
    why1 = ("the seam's task steps take aux_launch_config() as it is, unroll = 1 (sma_seam.hip:646, :725; "
            "sma_internal.h:82-88): a TAIL launch never has unroll 2")
    why2 = ("the seam's S-SGD barrier takes ssgd_apply_launch_config() as it is, unroll = 2 (sma_seam.hip:107; "
            "sma_internal.h:135-141): a TAIL launch never has unroll 1")
    for mom in tf:
        for wd in tf:
            for U in (1, 2):
                out[f"sma_optimise_kernel<{mom}, {wd}, 0, false, {U}, false>"] = why0
                out[f"default_optimise_kernel<{mom}, {wd}, 0, {U}>"] = why0
            out[f"sma_optimise_kernel<{mom}, {wd}, 1, true, 2, false>"] = why1
    for a in tf:
        for U in (1, 2):
            out[f"ssgd_accumulate_kernel<{a}, 0, false, {U}>"] = why0
            out[f"ssgd_apply_kernel<{a}, 0, false, {U}>"] = why0
        out[f"ssgd_accumulate_kernel<{a}, 1, true, 2>"] = why1
        out[f"ssgd_apply_kernel<{a}, 1, true, 1>"] = why2
    for U in (1, 2):
        out[f"broadcast_kernel<0, {U}>"] = why0
    why3 = ("staged_cfg has no setter (context_internal.h:559 and sync_steps.hip:1466, :1480, :1505 are its only uses) "
            "and staged_launch_config() sets unroll = 2 (sma_internal.h:114-121): no staged launch has unroll 1")
    for mom in tf:
        for wd in tf:
            for U in (1, 2):
                out[f"sma_optimise_kernel<{mom}, {wd}, 0, false, {U}, true>"] = why0
                for clip in tf:
                    out[f"sma_optimise_variables_kernel<{mom}, {wd}, 0, {U}, {clip}>"] = why0
            out[f"sma_optimise_kernel<{mom}, {wd}, 1, true, 2, true>"] = why1
    for R in (0, 1, 2, 4, 8, -1):
        for mom in tf:
            for copy in tf:
                out[f"sma_fused_staged_kernel<{R}, {mom}, {copy}, 1>"] = why3
        out[f"sma_accumulate_staged_kernel<{R}, 1>"] = why3
    for mom in tf:
        out[f"sma_apply_staged_kernel<{mom}, 1>"] = why3
        out[f"sma_fused_staged_kernel<0, {mom}, true, 2>"] = (
            "COPY is copies_total > 0, counted over the participating replicas (sync_steps.hip:20-27): with none of "
            "them (R = 0) it is false")
    return one_rank, multi


UNREACHABLE, _MULTI_RANK = _unreachable()

# ---------------------------------------------------------------------------
# Kernels this table does not drive, with the test that runs them.
# ---------------------------------------------------------------------------
def _elsewhere() -> Dict[str, str]:
    out: Dict[str, str] = {}
    for G in (2, 4, 8, -1):
        for P in (0, 1):
            for U in (1, 2):
                out[f"sma_peer_reduce_kernel<{G}, {P}, {U}>"] = "G > 1 only: tests/test_gpu_multidevice.py, tests/test_gpu_peer_ipc.py"
    for mom in ("false", "true"):
        for P in (0, 1):
            for U in (1, 2):
                out[f"sma_peer_apply_kernel<{mom}, {P}, {U}>"] = "G > 1 only: tests/test_gpu_multidevice.py, tests/test_gpu_peer_ipc.py"
    out["peer_poison_check_kernel"] = "one process per GPU: tests/test_gpu_peer_ipc.py"
    out["order_probe_kernel"] = "cbx_set_order_check: tests/test_gpu_parity.py, tests/test_gpu_realrccl.py"
    out["delay_kernel"] = ("fault injection only ($CBX_FAULT_ONE_STREAM_COMM_WAIT, $CBX_FAULT_SKIP_PEER_WAIT): "
                           "tests/test_gpu_parity.py, tests/test_gpu_peer_ipc.py")
    out["fill_normal_kernel"] = "cbx_fill_synthetic, compared with the oracle's fill: tests/test_gpu_parity.py"
    out["bn_pack_kernel"] = "cbx_average_batchnorm_stats: tests/test_gpu_parity.py, tests/test_gpu_seam.py"
    out["bn_unpack_kernel"] = "cbx_average_batchnorm_stats: tests/test_gpu_parity.py, tests/test_gpu_seam.py"
    # the two reductions: each of their few instantiations has a test of its own
    out["gradient_norm_kernel<0>"] = out["gradient_norm_kernel<1>"] = (
        "tests/test_gpu_reduction_edges.py::test_norm_regimes_through_both_doors_and_both_load_policies "
        "(the loads argument of cbx_sma_plan_gradient_norm picks the instantiation)")
    out["gradient_norm_reduce_kernel"] = "tests/test_gpu_reduction_edges.py, tests/test_gpu_gradient_clip.py: every norm pass ends in it"
    out["stats_pass_kernel<8>"] = "tests/test_gpu_reduction_edges.py::test_statistics_regimes_context_and_seam[wide-unrolled-8]"
    out["stats_pass_kernel<-1>"] = "tests/test_gpu_reduction_edges.py::test_statistics_regimes_context_and_seam[wide-chunked-9]"
    out["stats_reduce_kernel"] = "tests/test_gpu_reduction_edges.py, tests/test_gpu_stats.py: every statistics pass ends in it"
    out.update(_MULTI_RANK)  # the forms only a door of several ranks reaches: out of this table's scope
    return out


ELSEWHERE: Dict[str, str] = _elsewhere()

# ---------------------------------------------------------------------------
# No test runs these two: cbx_bench_copy returns a rate and leaves nothing to
# compare; the copy ceiling of `bench.py --full` is its only caller.
# ---------------------------------------------------------------------------
UNTESTED: Dict[str, str] = {
    "copy_kernel<0>": "no test: cbx_bench_copy (context.hip:2278-2289), a measurement, is its only caller",
    "copy_kernel<1>": "no test: cbx_bench_copy (context.hip:2278-2289), a measurement, is its only caller",
}

# The ELSEWHERE kernels a case launches on its way: the norm pass and its reduce
# in front of every clipped step (context.hip:1327, sma_seam.hip:831), with the
# default plain loads (clip_internal.h:48).
INCIDENTAL = ("gradient_norm_kernel<0>", "gradient_norm_reduce_kernel")
