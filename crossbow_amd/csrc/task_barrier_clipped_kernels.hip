// task_barrier_clipped_kernels.hip -- the replicas' pending task steps, clipped
// by global L2 norm, fused into the one-GPU SMA barrier
// (cbx_step_and_synchronise_clipped, cbx_sma_plan_step_and_optimise_clipped),
// for CDNA4 (gfx950).
//
// task_barrier_kernel (task_barrier_kernels.hip) with the CLIP arithmetic of
// sma_optimise_kernel (sma_kernels.hip): the same text (task_barrier_body.inc,
// task_barrier_step.h) behind the ClippedStep policy, and the same launch
// (task_barrier_launch.h).  Stepping replica i has a record of its own
// (cbx_clip_stats), left by the norm reduce (clip_kernels.hip) in front of
// this launch; the record pointers are a kernel parameter of their own beside
// TaskBarrierArgs.
//
// This file is a shared object of its own (libcrossbow_sma_clipped.so): the
// device code of libcrossbow_sma.so is not touched by it.
#include <hip/hip_ext.h>

#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) + sizeof(ClipRecordPtrs) <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

// The template parameters are task_barrier_kernel's.
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_clipped_kernel(const TaskBarrierArgs a, const ClipRecordPtrs rec) {
  const typename step_policy<ClippedStep, R>::type step{rec};
#include "task_barrier_body.inc"
}

struct ClippedLauncher {
  typedef ClippedStep Step;
  static constexpr bool kSideObject = true;
  // Base momentum beside stepping replicas that have none: a context has
  // base->last iff its replicas were made with momentum, so only the seam
  // reaches this form (a caller-owned buffer of whole chunks has no tail).
  template <bool MIXED, bool MOM, bool BMOM, bool WD>
  static constexpr bool seam_only() {
    return MIXED && !MOM && BMOM;
  }
  const ClipRecordPtrs &rec;
  template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_barrier_clipped_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>), g, b, lds, s,
                          t.start, t.stop, 0, a, rec);
  }
};

}  // namespace

hipError_t launch_task_barrier_clipped(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                       const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  ClipRecordPtrs full;
  if (!task_barrier_fill_records(a, rec, full)) return hipErrorInvalidValue;
  return task_barrier_launch(ClippedLauncher{full}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
