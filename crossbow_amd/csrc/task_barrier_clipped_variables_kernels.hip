// task_barrier_clipped_variables_kernels.hip -- the replicas' pending task
// steps, clipped by global L2 norm and with a learning rate per variable, fused
// into the one-GPU SMA barrier (cbx_step_and_synchronise_clipped_variables,
// cbx_sma_plan_step_and_optimise_clipped_variables), for CDNA4 (gfx950).
//
// task_barrier_kernel (task_barrier_kernels.hip) with both the CLIP arithmetic
// of sma_optimise_kernel and the rate lookup of sma_optimise_variables_kernel,
// as launch_sma_optimise_variables_clipped has them per replica: the same text
// (task_barrier_body.inc, task_barrier_step.h) behind the ClippedVariablesStep
// policy, and the same launch (task_barrier_launch.h).  The tables and the
// record pointers are kernel parameters of their own beside TaskBarrierArgs.
//
// This file is a shared object of its own (libcrossbow_sma_clipped_variables.so):
// the device code of libcrossbow_sma.so, libcrossbow_sma_variables.so and
// libcrossbow_sma_clipped.so is not touched by it.
#include <hip/hip_ext.h>

#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) + sizeof(ClipRecordPtrs) + 3 * sizeof(void *) + 8 <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

// The template parameters are task_barrier_kernel's.  chunks / bounds / mult:
// the tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi).
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_clipped_variables_kernel(const TaskBarrierArgs a,
                                                                             const uint32_t *__restrict__ chunks,
                                                                             const uint32_t *__restrict__ bounds,
                                                                             const float *__restrict__ mult,
                                                                             const uint32_t nvars,
                                                                             const ClipRecordPtrs rec) {
  const typename step_policy<ClippedVariablesStep, R>::type step{chunks, bounds, mult, nvars, rec};
#include "task_barrier_body.inc"
}

struct ClippedVariablesLauncher {
  typedef ClippedVariablesStep Step;
  static constexpr bool kSideObject = true;
  // The clipped object's rule: base momentum beside stepping replicas that
  // have none is the seam's shape only (a context has base->last iff its
  // replicas were made with momentum).  A call in which nobody steps never
  // comes here, so weight decay does not narrow it as in the variables object.
  template <bool MIXED, bool MOM, bool BMOM, bool WD>
  static constexpr bool seam_only() {
    return MIXED && !MOM && BMOM;
  }
  const VarTables &vt;
  const ClipRecordPtrs &rec;
  template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_barrier_clipped_variables_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>), g, b,
                          lds, s, t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars, rec);
  }
};

}  // namespace

hipError_t launch_task_barrier_clipped_variables(const TaskBarrierArgs &a, const VarTables &vt,
                                                 const ClipRecordPtrs &rec, bool keep_task_outputs,
                                                 const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  ClipRecordPtrs full;
  if (!task_barrier_fill_records(a, rec, full)) return hipErrorInvalidValue;
  return task_barrier_launch(ClippedVariablesLauncher{vt, full}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
