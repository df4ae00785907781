// task_ssgd_adaptive_internal.h -- the launcher of the replicas' pending task
// steps with layer-wise adaptive rates (LARS, LARC) fused into the one-GPU
// synchronous-SGD barrier (cbx_step_and_synchronise_ssgd_adaptive,
// cbx_ssgd_plan_step_and_optimise_adaptive; task_ssgd_adaptive_kernels.hip, a
// shared object of its own: libcrossbow_sma_ssgd_adaptive.so).  A header of its
// own, read by that file and by the two doors only: no other object's text
// changes with it.  Not part of the C-ABI; see include/crossbow_sma.h for the
// semantics, adaptive_internal.h for the tables, the scratch and the records and
// task_ssgd_internal.h for the arguments, which are the plain fused call's.
#pragma once

#include "adaptive_internal.h"
#include "task_ssgd_internal.h"

namespace cbx {

// launch_task_ssgd with the base model's update scaled per variable by the
// trust ratio of the base model's norm and the norm of the mean of the stepping
// replicas' raw gradients.  Three launches on `stream`:
//   pass   over the pieces of `t` (floats [0, t.elements) only): acc += the
//          stepping replicas' steps, exactly task_ssgd_kernel's sequence, g_i
//          written with weight decay and kept outputs, and per piece the sums
//          of z^2 and of (a.ratio * sum of raw g_i)^2 into s.slab();
//   trust  one wave per variable: s.records() and s.trust(), variable_trust_kernel's rule;
//   apply  over a.n4 float4s (and the tail range): a = t_v * acc, then
//          task_ssgd_kernel's apply and broadcast on a; base gradient +0.
// What the base gradient held on entry joins the update and not the norm.
// `vt`: the chunk table over the swept length (the context's padded tables,
// whose pad is pseudo-variable t.nvars and steps at 1, or the plan's); a
// variable at or past s.nvars steps at 1.  At least one replica steps (with
// nobody stepping the door launches launch_task_ssgd).  The compiled forms of
// the apply kernel are launch_task_ssgd's: no tail with unroll 1 or 2 and
// either policy; a tail with unroll 1 and policy 1.  Anything else is
// hipErrorInvalidValue.  tm.start stamps the pass, tm.stop the apply kernel.
hipError_t launch_task_ssgd_adaptive(const TaskSsgdArgs &a, const AdaptiveTables &t, const AdaptiveScratch &s,
                                     const AdaptiveParams &p, const VarTables &vt, bool keep_task_outputs,
                                     const LaunchConfig &cfg, hipStream_t stream, Timing tm = {});

}  // namespace cbx
