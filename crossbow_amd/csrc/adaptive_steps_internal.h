// adaptive_steps_internal.h -- the replicas' pending task steps with layer-wise
// adaptive rates (LARS, LARC) fused into the one-GPU SMA barrier
// (task_barrier_adaptive_kernels.hip; cbx_step_and_synchronise_adaptive,
// cbx_sma_plan_step_and_optimise_adaptive) and into the elastic-averaging one
// (task_elastic_adaptive_kernels.hip; cbx_step_and_synchronise_elastic_adaptive,
// cbx_ea_plan_step_and_optimise_adaptive).  Not part of the C-ABI; see
// include/crossbow_sma.h for the semantics and adaptive_internal.h for the
// tables, the scratch and the records, which are the replica step's.
#pragma once

#include "adaptive_internal.h"
#include "sma_internal.h"

namespace cbx {

// The finished rates of one launch, on the device: row v holds, at column k,
// (rate_k * mult[v]) * trust_k[v] of participating replica k.  Variable-major,
// rows of kMaxReplicas floats (256 bytes), the allocation 256-byte aligned.
// One row more than the variable list has: the pad of the context's buffers is
// a pseudo-variable of its own (build_padded_optimise_plan).  Zeroed when
// allocated; a column whose replica only joins is never used.
struct RateMatrix {
  float *dev = nullptr;
  uint32_t rows = 0;
};
// For the variable list of `t` (blocking), after freeing what `m` held.
hipError_t rate_matrix_alloc(RateMatrix &m, const AdaptiveTables &t);
void rate_matrix_free(RateMatrix &m);

// The stepping replicas of one call, in id order: stepping replica j is
// participating replica col[j], steps with rate[j] (-learning rate) and leaves
// its partials, records and trust table in scratch[j].
struct ReplicaSteps {
  int count = 0;
  const float *w[kMaxReplicas];
  const float *g[kMaxReplicas];
  const AdaptiveScratch *scratch[kMaxReplicas];
  float rate[kMaxReplicas];
  int col[kMaxReplicas];
};

// launch_variable_norms for every stepping replica at once, in two launches on
// `stream`: the two-buffer pass over w[j][0, n) and g[j][0, n) with grid
// (stats_grid(npieces), count), then one wave per (variable, stepping replica),
// which leaves the replica's records and trust table as launch_variable_norms
// leaves them, bit for bit, and row v, column col[j] of `m` besides.  mult:
// t.nvars multipliers (VarTables::mult, or AdaptiveTables::ones()).  rows:
// t.nvars, or t.nvars + 1 where the barrier's tables have the pad's
// pseudo-variable, whose row is (rate * 1.0f) * 1.0f.  Nothing past float n - 1
// is read.  policy: 0 plain, 1 nontemporal loads.
hipError_t launch_replica_norms(const ReplicaSteps &rs, const AdaptiveTables &t, const float *mult,
                                const AdaptiveParams &p, const RateMatrix &m, uint32_t rows, int policy,
                                hipStream_t stream, Timing pass = {}, Timing reduce = {});

// launch_task_barrier_variables with the rates of `m` in place of
// a.rate[k] * t.mult[v] (libcrossbow_sma_adaptive_steps.so): per stepping
// replica launch_sma_optimise_adaptive's bits, then the barrier's.  `t` as for
// launch_task_barrier_variables (t.mult is not read); m.rows >= t.nvars.  At
// least one replica steps.  The compiled forms are that launch's.
hipError_t launch_task_barrier_adaptive(const TaskBarrierArgs &a, const VarTables &t, const RateMatrix &m,
                                        bool keep_task_outputs, const LaunchConfig &cfg, hipStream_t stream,
                                        Timing tm = {});

// launch_task_elastic_variables with the rates of `m` in place of
// a.rate[k] * t.mult[v] (task_elastic_adaptive_kernels.hip,
// libcrossbow_sma_elastic_adaptive.so): per stepping replica
// launch_sma_optimise_adaptive's bits, then the elastic-averaging barrier's.
// `t`, `m` and the stepping replica as for launch_task_barrier_adaptive; `m` is
// what launch_replica_norms left on the same stream.  The compiled forms are
// launch_task_elastic's.
hipError_t launch_task_elastic_adaptive(const TaskBarrierArgs &a, const VarTables &t, const RateMatrix &m,
                                        bool keep_task_outputs, const LaunchConfig &cfg, hipStream_t stream,
                                        Timing tm = {});

}  // namespace cbx
