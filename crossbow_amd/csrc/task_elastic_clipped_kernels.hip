// task_elastic_clipped_kernels.hip -- the replicas' pending task steps, clipped
// by global L2 norm, fused into the one-GPU elastic-averaging barrier
// (cbx_step_and_synchronise_elastic_clipped_variables,
// cbx_ea_plan_step_and_optimise_clipped_variables with only clipping on), for
// CDNA4 (gfx950).
//
// task_elastic_kernel (task_elastic_kernels.hip) with the CLIP arithmetic of
// sma_optimise_kernel: the shared text (task_elastic_policy_body.inc,
// task_elastic_policy.h) behind the ClippedStep policy.  The record pointers
// are a kernel parameter of their own beside TaskBarrierArgs.
//
// One of the three compilation units of libcrossbow_sma_elastic_policies.so:
// the device code of the other shared objects is not touched by it.
#include <hip/hip_ext.h>

#include "task_elastic_policy.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) + sizeof(ClipRecordPtrs) <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

// The template parameters are task_elastic_kernel's.  rec.p[k]: the record of
// participating replica k, loaded for every one of them.
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_clipped_kernel(const TaskBarrierArgs a, const ClipRecordPtrs rec) {
  const typename step_policy<ClippedStep, R>::type step{rec};
#include "task_elastic_policy_body.inc"
}

struct ElasticClippedLauncher {
  typedef ClippedStep Step;
  const ClipRecordPtrs &rec;
  template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_elastic_clipped_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, b, lds, s, t.start,
                          t.stop, 0, a, rec);
  }
};

}  // namespace

hipError_t launch_task_elastic_clipped(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                       const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  // every stepping replica has a record, somebody steps, and the entries of
  // the replicas that only join hold a valid one: the kernel loads them all
  ClipRecordPtrs full;
  if (!task_barrier_fill_records(a, rec, full)) return hipErrorInvalidValue;
  return task_elastic_policy_launch(ElasticClippedLauncher{full}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
