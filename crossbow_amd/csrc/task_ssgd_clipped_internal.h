// task_ssgd_clipped_internal.h -- the launchers of the synchronous-SGD task
// step and of the fused synchronous-SGD barrier with gradient clipping by
// global L2 norm (cbx_replica_accumulate_clipped,
// cbx_step_and_synchronise_ssgd_clipped, cbx_ssgd_plan_accumulate_clipped,
// cbx_ssgd_plan_step_and_optimise_clipped; task_ssgd_clipped_kernels.hip, a
// shared object of its own: libcrossbow_sma_ssgd_clipped.so).  A header of its
// own, read by that file and by the two doors only: no other object's text
// changes with it.  Not part of the C-ABI.
#pragma once

#include "clip_internal.h"
#include "task_ssgd_internal.h"

namespace cbx {

// The arguments block and the records travel side by side as two kernel
// parameters.
static_assert(sizeof(TaskSsgdArgs) + sizeof(ClipRecordPtrs) < 4096, "kernel arguments are limited to 4 KB");

// launch_task_ssgd with the clipped step.  rec.p[k] is the record of STEPPING
// replica k (the order of a.sw, a.g and a.rate, not of a.w), left by
// launch_gradient_norm earlier on the stream; the other entries are not read.
// Stepping replica k with the record's skip bit contributes nothing: none of
// g_k, w_k or its rate is loaded, acc takes no fma from it (not one with 0), g_k
// is not written.  Otherwise gv = scale_k * g_k, one fp32 multiply before the
// weight decay, a kept g_k is written whether or not there is weight decay, and
// acc = fma(rate_k, gv, acc).  a.ratio stays 1 / wpc: a skipped replica is a
// zero in the mean.  Everything behind the accumulator, and the receiving list,
// are launch_task_ssgd's.  At least one replica steps (without one there is
// nothing to clip: launch_task_ssgd).  Compiled forms and refusals as there.
hipError_t launch_task_ssgd_clipped(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                    const LaunchConfig &cfg, hipStream_t stream, Timing t = {});

// launch_ssgd_accumulate for one replica with its record: on the skip bit the
// kernel returns having read and written no buffer; otherwise g = scale * g
// before the weight decay, g is written always, acc = fma(rate, g, acc).  Of
// SsgdArgs it reads wsrc, g, acc, n4, rate, wd and the tail range.  Compiled
// forms: unroll 1 or 2; without a tail either policy, with one policy 1.
hipError_t launch_ssgd_accumulate_clipped(const SsgdArgs &a, const ClipRecord *rec, const LaunchConfig &cfg,
                                          hipStream_t stream, Timing t = {});

}  // namespace cbx
