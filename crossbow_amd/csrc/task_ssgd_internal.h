// task_ssgd_internal.h -- the kernel arguments and the launcher of the
// replicas' pending task steps fused into the one-GPU synchronous-SGD barrier
// (cbx_step_and_synchronise_ssgd, cbx_ssgd_plan_step_and_optimise;
// task_ssgd_kernels.hip, a shared object of its own:
// libcrossbow_sma_ssgd_steps.so).  A header of its own, read by that file and by
// the two doors only: no other object's text changes with it.  Not part of the
// C-ABI.
#pragma once

#include "sma_internal.h"

namespace cbx {

// launch_ssgd_accumulate on every stepping replica in list order, then
// launch_ssgd_apply at G = 1 (D == acc), in one pass.  The stepping and the
// receiving replicas are two lists: a replica that steps and is broadcast to
// stands in both, one that only joins in the second.  About 1.9 KB of kernel
// arguments at kMaxReplicas = 64.
struct TaskSsgdArgs {
  const v4f *sw[kMaxReplicas];  // stepping replicas, ascending id: replica->data, read with weight decay only
  v4f *g[kMaxReplicas];         // their replica->gradient (written with weight decay and kept outputs only)
  float rate[kMaxReplicas];     // -learning rate of the replica's task (synchronoussgd.cu:46)
  v4f *w[kMaxReplicas];         // receiving replicas (locked, id >= first): replica->data, written only
  v4f *z;                       // base->data
  v4f *last;                    // base->last (momentum > 0 only)
  v4f *acc;                     // base->gradient: read as the call finds it, left +0
  int64_t n4;                   // float4s (whole 64 x unroll chunks; the context's: kPadFloat4s)
  float wd;                     // the stepping replicas' conf->weightDecay
  float ratio;                  // 1 / wpc (synchronoussgd.c:55)
  float momentum;               // base conf->momentum (synchronoussgd.c:64)
  int nstep;
  int nrecv;
  int pad_;
  int64_t tail_lo, tail_hi;  // caller-owned buffers: elements past the last whole trip (see SmaArgs)
  int tail_blocks;
};
static_assert(sizeof(TaskSsgdArgs) < 4096, "kernel arguments are limited to 4 KB");

// keep_task_outputs: g of the stepping replicas is written as
// launch_ssgd_accumulate writes it (with weight decay only); otherwise it is
// not touched.  a.wd is 0 when nobody steps.  Compiled forms: no tail with
// unroll 1 or 2 and either policy; a tail with unroll 1 and policy 1.  Anything
// else is hipErrorInvalidValue, as is a block over 256 or no multiple of 64, or
// an n4 that is no whole number of 64 x unroll chunks.  a.n4 == 0 with a tail
// range launches the tail workgroups only.  The launch shape is
// launch_task_barrier's (task_barrier_launch_config).
hipError_t launch_task_ssgd(const TaskSsgdArgs &a, bool keep_task_outputs, const LaunchConfig &cfg, hipStream_t stream,
                            Timing t = {});

}  // namespace cbx
