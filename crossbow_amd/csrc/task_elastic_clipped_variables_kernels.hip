// task_elastic_clipped_variables_kernels.hip -- the replicas' pending task
// steps, clipped by global L2 norm and with a learning rate per variable, fused
// into the one-GPU elastic-averaging barrier
// (cbx_step_and_synchronise_elastic_clipped_variables,
// cbx_ea_plan_step_and_optimise_clipped_variables with both on), for CDNA4
// (gfx950).
//
// task_elastic_kernel (task_elastic_kernels.hip) with both the CLIP arithmetic
// of sma_optimise_kernel and the rate lookup of sma_optimise_variables_kernel:
// the shared text (task_elastic_policy_body.inc, task_elastic_policy.h) behind
// the ClippedVariablesStep policy.  The tables and the record pointers are
// kernel parameters of their own beside TaskBarrierArgs.
//
// One of the three compilation units of libcrossbow_sma_elastic_policies.so:
// the device code of the other shared objects is not touched by it.
#include <hip/hip_ext.h>

#include "task_elastic_policy.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) + sizeof(ClipRecordPtrs) + 3 * sizeof(void *) + 8 <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

// The template parameters are task_elastic_kernel's; the other parameters are
// those of the two kernels beside this one.
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_clipped_variables_kernel(const TaskBarrierArgs a,
                                                                             const uint32_t *__restrict__ chunks,
                                                                             const uint32_t *__restrict__ bounds,
                                                                             const float *__restrict__ mult,
                                                                             const uint32_t nvars,
                                                                             const ClipRecordPtrs rec) {
  const typename step_policy<ClippedVariablesStep, R>::type step{chunks, bounds, mult, nvars, rec};
#include "task_elastic_policy_body.inc"
}

struct ElasticClippedVariablesLauncher {
  typedef ClippedVariablesStep Step;
  const VarTables &vt;
  const ClipRecordPtrs &rec;
  template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_elastic_clipped_variables_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, b, lds, s,
                          t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars, rec);
  }
};

}  // namespace

hipError_t launch_task_elastic_clipped_variables(const TaskBarrierArgs &a, const VarTables &vt,
                                                 const ClipRecordPtrs &rec, bool keep_task_outputs,
                                                 const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  ClipRecordPtrs full;
  if (!task_barrier_fill_records(a, rec, full)) return hipErrorInvalidValue;
  return task_elastic_policy_launch(ElasticClippedVariablesLauncher{vt, full}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
