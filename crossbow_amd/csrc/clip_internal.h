// clip_internal.h -- gradient clipping by global L2 norm and the non-finite
// skip of the replica optimiser step (clip_kernels.hip; cbx_set_gradient_clip,
// cbx_sma_plan_optimise_clipped).  Not part of the C-ABI; see
// include/crossbow_sma.h for the semantics.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/crossbow_sma.h"
#include "sma_internal.h"
#include "stats_plan.h"

namespace cbx {

// Floats per tile of the norm pass: one wave, 16 float4 trips, one partial.
// Tiles, grid and summation tree are fixed functions of n alone.
constexpr uint32_t kClipTile = kStatsTile;

// One tile's partial: the sum of squares of its finite floats and the count
// of the others.  16 bytes; tile t of a replica at slab[t], in offset order,
// so a later per-operator accumulation can fill the same slab.
struct ClipPartial {
  double sum_sq;
  unsigned long long nonfinite;
};

// The record the reduce leaves and the CLIP step kernels read: cbx_clip_stats
// itself (scale at byte 16, flags at byte 20).
typedef cbx_clip_stats ClipRecord;
constexpr uint32_t kClipClipped = 1u, kClipSkipped = 2u;

// Per replica (context) or per slot (seam plan): [record | pad to 64 B | slab].
struct ClipScratch {
  char *dev = nullptr;
  uint32_t tiles = 0;
  ClipRecord *record() const { return reinterpret_cast<ClipRecord *>(dev); }
  ClipPartial *slab() const { return reinterpret_cast<ClipPartial *>(dev + 64); }
};

// The norm pass's loads of g: 1 nontemporal, 0 plain.  Plain: the step
// re-reads g right behind the pass and finds part of it on-die, which
// measured 2.4 % faster per clipped step (DESIGN.md 8e has both).
// $CBX_CLIP_NORM_LOADS = temporal | nontemporal overrides it for that
// measurement; it is read by cbx_set_gradient_clip and cbx_sma_plan_create.
constexpr int kClipNormPolicy = 0;
inline int clip_norm_policy() {
  const char *e = getenv("CBX_CLIP_NORM_LOADS");
  if (e && strcmp(e, "temporal") == 0) return 0;
  if (e && strcmp(e, "nontemporal") == 0) return 1;
  return kClipNormPolicy;
}

inline uint32_t clip_tiles(int64_t n) { return (uint32_t)((n + kClipTile - 1) / kClipTile); }

// One allocation for a model of n floats, the record zeroed (blocking).
hipError_t clip_scratch_alloc(ClipScratch &s, int64_t n);
void clip_scratch_free(ClipScratch &s);

// The norm pass over g[0, n) and, right behind it on the same stream, the
// one-wave reduce that leaves S, K, scale and the flags in the record and
// bumps its running counts.  g is 16-byte aligned; nothing past g[n - 1] is
// read.  policy: 0 plain, 1 nontemporal loads of g.  Each launch stamps its
// own optional timing pair.
hipError_t launch_gradient_norm(const float *g, int64_t n, const ClipScratch &s, float max_norm, bool skip_nonfinite,
                                int policy, hipStream_t stream, Timing pass = {}, Timing reduce = {});

// launch_sma_optimise / launch_sma_optimise_variables with the CLIP
// instantiations: g is multiplied by the record's scale before weight decay,
// and a step whose record carries the skip bit writes s = w and nothing else.
hipError_t launch_sma_optimise_clipped(const OptArgs &a, const ClipRecord *rec, const LaunchConfig &cfg,
                                       hipStream_t stream, Timing t = {});
hipError_t launch_sma_optimise_variables_clipped(const VarTables &t, VarOptArgs a, const ClipRecord *rec,
                                                 const LaunchConfig &cfg, hipStream_t stream, Timing tm = {});

// The records of a fused launch's participating replicas, in TaskBarrierArgs'
// order: a kernel parameter of its own (512 bytes) beside that block.
struct ClipRecordPtrs {
  const ClipRecord *__restrict__ p[kMaxReplicas];
};
// launch_task_barrier with the clipped step (task_barrier_clipped_kernels.hip,
// a shared object of its own: libcrossbow_sma_clipped.so): stepping replica k
// multiplies g by the scale of rec.p[k] before weight decay, writes a kept g
// always, and with the record's skip bit does s = w and nothing else before it
// joins the barrier.  rec.p[k] is the record launch_gradient_norm left earlier
// on the stream, non-null for every stepping replica; the other entries are not
// read.  At least one replica steps (without one there is nothing to clip:
// launch_task_barrier).  Compiled forms: no tail with unroll 1 or 2 and either
// policy; a tail with unroll 1 and policy 1.  Anything else is
// hipErrorInvalidValue, before the launch.
hipError_t launch_task_barrier_clipped(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                       const LaunchConfig &cfg, hipStream_t stream, Timing t = {});
// launch_task_barrier_clipped with a learning rate per variable
// (task_barrier_clipped_variables_kernels.hip, a shared object of its own:
// libcrossbow_sma_clipped_variables.so): stepping replica k clips as above and
// steps with a.rate[k] * t.mult[v], launch_sma_optimise_variables_clipped's
// bits per replica.  The tables as for launch_task_barrier_variables, the
// records and the compiled forms as for launch_task_barrier_clipped.
hipError_t launch_task_barrier_clipped_variables(const TaskBarrierArgs &a, const VarTables &t,
                                                 const ClipRecordPtrs &rec, bool keep_task_outputs,
                                                 const LaunchConfig &cfg, hipStream_t stream, Timing tm = {});

}  // namespace cbx
