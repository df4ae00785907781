// task_barrier_variables_kernels.hip -- the replicas' pending task steps with a
// learning rate per variable, fused into the one-GPU SMA barrier
// (cbx_step_and_synchronise_variables, cbx_sma_plan_step_and_optimise_variables),
// for CDNA4 (gfx950).
//
// task_barrier_kernel (task_barrier_kernels.hip) with the rate lookup of
// sma_optimise_variables_kernel (variable_rate_kernels.hip): the same text
// (task_barrier_body.inc, task_barrier_step.h) behind the VariablesStep
// policy, which puts r_iv = rate_i * mult[v] in place of rate_i, and the same
// launch (task_barrier_launch.h).
//
// The context's buffers are padded to kPadFloat4: its table is built over the
// padded length, the pad floats a last pseudo-variable of multiplier 1
// (build_padded_optimise_plan), so the kernel knows nothing of the pad and a
// zero pad stays zero.  Buffers the caller owns take the TAIL instantiations:
// the last elements one per lane, each float's variable from the same tables.
//
// This file is a shared object of its own (libcrossbow_sma_variables.so): the
// device code of libcrossbow_sma.so is not touched by it.
#include <hip/hip_ext.h>

#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {
namespace {

// The template parameters are task_barrier_kernel's.  chunks / bounds / mult:
// the tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi).
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_variables_kernel(const TaskBarrierArgs a,
                                                                     const uint32_t *__restrict__ chunks,
                                                                     const uint32_t *__restrict__ bounds,
                                                                     const float *__restrict__ mult,
                                                                     const uint32_t nvars) {
  const typename step_policy<VariablesStep, R>::type step{chunks, bounds, mult, nvars};
#include "task_barrier_body.inc"
}

struct VariablesLauncher {
  typedef VariablesStep Step;
  static constexpr bool kSideObject = true;
  // Base momentum beside stepping replicas that have none, weight decay on: a
  // context has base->last iff its replicas were made with momentum, so only
  // the seam reaches this form (a caller-owned buffer of whole chunks has no
  // tail).
  template <bool MIXED, bool MOM, bool BMOM, bool WD>
  static constexpr bool seam_only() {
    return MIXED && !MOM && BMOM && WD;
  }
  const VarTables &vt;
  template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_barrier_variables_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>), g, b, lds, s,
                          t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars);
  }
};

}  // namespace

hipError_t launch_task_barrier_variables(const TaskBarrierArgs &a, const VarTables &vt, bool keep_task_outputs,
                                         const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  return task_barrier_launch(VariablesLauncher{vt}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
