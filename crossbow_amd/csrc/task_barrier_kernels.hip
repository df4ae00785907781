// task_barrier_kernels.hip -- the replicas' pending task steps fused into the
// one-GPU SMA barrier (cbx_step_and_synchronise), for CDNA4 (gfx950).
//
// With tau = 1 every task step (sma_optimise_kernel) is followed by a barrier
// (sma_fused_kernel) before the replica is read again.  The two passes read
// and write w_i twice, and the barrier reads back an s_i the step wrote only
// for it.  Per element, with R replicas and momentum on:
//
//   R x step, then the barrier      (28R + 12R + 16) n B = (40R + 16) n
//   this kernel, s and g kept       (28R + 16) n
//   this kernel, s and g discarded  (20R + 16) n
//
// One streaming pass in the shape of the kernels it fuses: 16-byte float4s per
// lane behind an SGPR base and a 32-bit offset, every load of a replica chunk
// issued before the first arithmetic, acc in registers, no LDS.  The context's
// buffers are padded to kPadFloat4 and need no tail; buffers the caller owns
// (cbx_sma_plan_step_and_optimise) take the TAIL instantiations.
//
// The kernel's text, with the fp32 sequence it keeps to, is
// task_barrier_body.inc and task_barrier_step.h, shared with the per-variable
// and the clipped kernel; the launch is task_barrier_launch.h.  This object
// holds the plain step (PlainStep) and compiles every form.
#include <hip/hip_ext.h>

#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) <= 4096, "the kernel argument block must stay under HIP's 4 KB");

namespace {

// R > 0: that many replicas, fully unrolled (R <= kChunk); R == -1 takes
// a.nrep and walks the replicas in register-resident chunks of kChunk.
// MIXED: a.step_mask says which replicas step (a wave-uniform branch per
// replica); otherwise all of them do.  MOM / WD: the stepping replicas'
// momentum and weight decay; BMOM: the base model's momentum (a.blast).
// KEEP: s_i and g_i of the stepping replicas are written as the plain step
// writes them; otherwise they are not touched.  a.copy is wave-uniform too.
// TAIL: the launch's first a.tail_blocks workgroups do the caller's last
// elements (task_barrier_tail_elem); without it the kernel is the context's.
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_kernel(const TaskBarrierArgs a) {
  const typename step_policy<PlainStep, R>::type step{};
#include "task_barrier_body.inc"
}

struct PlainLauncher {
  typedef PlainStep Step;
  static constexpr bool kSideObject = false;
  template <bool MIXED, bool MOM, bool BMOM, bool WD>
  static constexpr bool seam_only() {
    return false;
  }
  template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_barrier_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>), g, b, lds, s, t.start, t.stop,
                          0, a);
  }
};

}  // namespace

hipError_t launch_task_barrier(const TaskBarrierArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                               hipStream_t stream, Timing t) {
  return task_barrier_launch(PlainLauncher{}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
