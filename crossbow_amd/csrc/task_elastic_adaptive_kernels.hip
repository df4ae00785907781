// task_elastic_adaptive_kernels.hip -- the replicas' pending task steps with
// layer-wise adaptive rates (LARS, and LARC as its capped form) fused into the
// one-GPU elastic-averaging barrier (cbx_step_and_synchronise_elastic_adaptive,
// cbx_ea_plan_step_and_optimise_adaptive), for CDNA4 (gfx950).
//
// The call is three launches.  The first two are launch_replica_norms
// (libcrossbow_sma_adaptive_steps.so), called by the door and not copied here:
// every stepping replica's norm pass in one launch, every trust ratio in a
// second, which leaves the records, the dense trust tables and the rate matrix
// M[v * kMaxReplicas + k] = (rate_k * mult[v]) * t_kv, k the replica's slot
// among the participating ones.  The third is this file's:
//
//   task_elastic_adaptive_kernel
//       task_elastic_kernel (task_elastic_kernels.hip) behind the AdaptiveStep
//       policy (task_barrier_step.h): the fifth policy of the shared elastic
//       text (task_elastic_body.inc, task_elastic_launch.h).  The rate comes
//       finished out of the matrix and the barrier multiplies nothing.  A
//       uniform 256-float chunk reads the RR rates of a replica chunk in one
//       scalar load of 1, 2, 4 or 8 dwords, once per replica chunk; a chunk
//       with a variable boundary inside finds each lane's four rows once per
//       trip and gathers four rates per replica inside the replica loop; the
//       TAIL workgroups look the rate up per element.  Everything else is the
//       elastic text's: a replica that only joins is one stream, d comes from
//       the stepped w', no base momentum, no Phase D, no copy flag.
//
// This file is a shared object of its own (libcrossbow_sma_elastic_adaptive.so):
// no other object's device code is touched by it.
#include <hip/hip_ext.h>

#include "adaptive_steps_internal.h"
#include "task_elastic_launch.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) + 3 * sizeof(void *) + 8 <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

// The template parameters are task_elastic_kernel's.  chunks / bounds: the
// tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi);
// matrix: at least nvars rows of kMaxReplicas finished rates, 256-byte aligned.
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_adaptive_kernel(const TaskBarrierArgs a,
                                                                    const uint32_t *__restrict__ chunks,
                                                                    const uint32_t *__restrict__ bounds,
                                                                    const uint32_t nvars,
                                                                    const float *__restrict__ matrix) {
  const typename step_policy<AdaptiveStep, R>::type step{chunks, bounds, nvars, matrix};
#include "task_elastic_body.inc"
}

struct ElasticAdaptiveLauncher {
  typedef AdaptiveStep Step;
  const VarTables &vt;
  const float *matrix;
  template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_elastic_adaptive_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, b, lds, s, t.start,
                          t.stop, 0, a, vt.chunks, vt.bounds, vt.nvars, matrix);
  }
};

}  // namespace

hipError_t launch_task_elastic_adaptive(const TaskBarrierArgs &a, const VarTables &vt, const RateMatrix &m,
                                        bool keep_task_outputs, const LaunchConfig &cfg, hipStream_t stream,
                                        Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  // Every row a chunk entry or a boundary search can name is in the matrix, and
  // every column the widest scalar load reaches (kMaxReplicas floats a row).
  if (!m.dev || m.rows < vt.nvars || (reinterpret_cast<uintptr_t>(m.dev) & 255u) != 0 || a.step_mask == 0)
    return hipErrorInvalidValue;
  return task_elastic_launch(ElasticAdaptiveLauncher{vt, m.dev}, a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
