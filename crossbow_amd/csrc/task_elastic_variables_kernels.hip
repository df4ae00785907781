// task_elastic_variables_kernels.hip -- the replicas' pending task steps with
// a learning rate per variable, fused into the one-GPU elastic-averaging
// barrier (cbx_step_and_synchronise_elastic_clipped_variables,
// cbx_ea_plan_step_and_optimise_clipped_variables with only the rates on), for
// CDNA4 (gfx950).
//
// task_elastic_kernel (task_elastic_kernels.hip) with the rate lookup of
// sma_optimise_variables_kernel: the shared text (task_elastic_policy_body.inc,
// task_elastic_policy.h) behind the VariablesStep policy.  The tables are
// kernel parameters of their own beside TaskBarrierArgs.
//
// One of the three compilation units of libcrossbow_sma_elastic_policies.so:
// the device code of the other shared objects is not touched by it.
#include <hip/hip_ext.h>

#include "task_elastic_policy.h"

namespace cbx {

namespace {

// The template parameters are task_elastic_kernel's.  chunks / bounds / mult:
// the tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi).
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_variables_kernel(const TaskBarrierArgs a,
                                                                     const uint32_t *__restrict__ chunks,
                                                                     const uint32_t *__restrict__ bounds,
                                                                     const float *__restrict__ mult,
                                                                     const uint32_t nvars) {
  const typename step_policy<VariablesStep, R>::type step{chunks, bounds, mult, nvars};
#include "task_elastic_policy_body.inc"
}

struct ElasticVariablesLauncher {
  typedef VariablesStep Step;
  const VarTables &vt;
  template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_elastic_variables_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, b, lds, s, t.start,
                          t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars);
  }
};

}  // namespace

hipError_t launch_task_elastic_variables(const TaskBarrierArgs &a, const VarTables &vt, bool keep_task_outputs,
                                         const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  return task_elastic_policy_launch(ElasticVariablesLauncher{vt}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
