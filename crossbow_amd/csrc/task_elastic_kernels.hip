// task_elastic_kernels.hip -- the replicas' pending task steps fused into the
// one-GPU elastic-averaging barrier (cbx_step_and_synchronise_elastic,
// cbx_ea_plan_step_and_optimise), for CDNA4 (gfx950).
//
// EA-SGD (update model 3 with cbx_set_elastic_average): with tau = 1 every
// task step (kernels/optimisers/synchronouseamsgd.cu, whose call sequence is
// sma.cu's: sma_optimise_kernel) is followed by the elastic barrier
// (synch/synchronouseamsgd.c:42-90: averaging_kernel<kElasticW>), which on one
// device reads the replica's data AFTER the step and no snapshot.  Per
// element, with R replicas and momentum on:
//
//   R x step, then the barrier      (28R + 8R + 8) n B = (36R + 8) n
//   this kernel, s and g kept       (28R + 8) n
//   this kernel, s and g discarded  (20R + 8) n
//
// One streaming pass in the shape of the kernels it fuses (task_barrier_body.inc,
// averaging_kernels.hip): 16-byte float4s per lane behind an SGPR base and a
// 32-bit offset, every load of a replica chunk issued before the first
// arithmetic, acc in registers, no LDS.  The context's buffers are padded to
// kPadFloat4 and need no tail; buffers the caller owns take the TAIL
// instantiations.
//
// The kernel's text, with the fp32 sequence it keeps to, is
// task_elastic_body.inc, shared with the per-variable and the clipped kernels
// (libcrossbow_sma_elastic_policies.so); the tail and the launch are
// task_elastic_launch.h.  This object (libcrossbow_sma_elastic_steps.so) holds
// the plain step (PlainStep) in every form a door reaches.
#include <hip/hip_ext.h>

#include "task_elastic_launch.h"

namespace cbx {

static_assert(kMaxReplicas <= 64, "step_mask holds one bit per replica");

namespace {

// R > 0: that many replicas, fully unrolled (R <= kChunk), all of them
// stepping; R == -1 takes a.nrep and walks the replicas in register-resident
// chunks of kChunk.  MIXED: a.step_mask says which replicas step (a
// wave-uniform choice per replica); otherwise all of them do.  MOM / WD: the
// stepping replicas' momentum and weight decay.  KEEP: s_i and g_i of the
// stepping replicas are written as the plain step writes them; otherwise they
// are not touched.  TAIL: the launch's first a.tail_blocks workgroups do the
// caller's last elements (task_elastic_tail_elem); without it the kernel is the
// context's.  a.s of a replica that only joins, a.blast and a.copy are not read.
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_kernel(const TaskBarrierArgs a) {
  const typename step_policy<PlainStep, R>::type step{};
#include "task_elastic_body.inc"
}

struct ElasticPlainLauncher {
  typedef PlainStep Step;
  template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_elastic_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, b, lds, s, t.start, t.stop, 0,
                          a);
  }
};

}  // namespace

hipError_t launch_task_elastic(const TaskBarrierArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                               hipStream_t stream, Timing t) {
  return task_elastic_launch(ElasticPlainLauncher{}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
