// adaptive_internal.h -- layer-wise adaptive rate scaling (LARS, and LARC as
// its capped form) in the replica optimiser step (adaptive_rate_kernels.hip;
// cbx_set_adaptive_rate, cbx_sma_plan_optimise_adaptive).  Not part of the
// C-ABI; see include/crossbow_sma.h for the semantics.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/crossbow_sma.h"
#include "sma_internal.h"
#include "stats_plan.h"

namespace cbx {

// One piece's partial: the sums of squares of its finite floats of w and of
// g, and the count of the others in both.  32 bytes; piece p of a replica at
// slab[p], in offset order, so variable v's partials are
// slab[var_first[v] .. var_first[v + 1]).
struct AdaptivePartial {
  double w_sq, g_sq;
  unsigned long long nonfinite;
  unsigned long long reserved;
};

// The record the trust kernel leaves per variable: cbx_adaptive_stats itself.
typedef cbx_adaptive_stats AdaptiveRecord;
constexpr uint32_t kAdaptiveApplied = CBX_ADAPTIVE_APPLIED, kAdaptiveExcluded = CBX_ADAPTIVE_EXCLUDED,
                   kAdaptiveDegenerate = CBX_ADAPTIVE_DEGENERATE, kAdaptiveCapped = CBX_ADAPTIVE_CAPPED;

// What a device keeps per variable list, beside the tables of the per-variable
// step (VarTables): the piece table of the reduction (stats_plan.h), the
// variables' first pieces and their enable flags.  One allocation:
//   [pieces: npieces x 16 B][var_first: nvars + 1][enable: nvars words][ones: nvars floats]
// `ones` stands in for the multipliers of a step without
// cbx_set_variable_learning_rates (rate * 1.0f is exact).
struct AdaptiveTables {
  char *dev = nullptr;
  uint32_t npieces = 0;
  uint32_t nvars = 0;
  uint32_t elements = 0;
  const StatsPiece *pieces() const { return reinterpret_cast<const StatsPiece *>(dev); }
  uint32_t *var_first() const { return reinterpret_cast<uint32_t *>(dev + (size_t)npieces * sizeof(StatsPiece)); }
  uint32_t *enable() const { return var_first() + nvars + 1; }
  const float *ones() const { return reinterpret_cast<const float *>(enable() + nvars); }
};

// Per replica (context) or per slot (seam plan), one allocation:
//   [records: nvars x 32 B][trust: nvars floats, padded to 32 B][slab: npieces x 32 B]
struct AdaptiveScratch {
  char *dev = nullptr;
  uint32_t npieces = 0;
  uint32_t nvars = 0;
  size_t trust_bytes() const { return ((size_t)nvars * 4 + 31) / 32 * 32; }
  AdaptiveRecord *records() const { return reinterpret_cast<AdaptiveRecord *>(dev); }
  float *trust() const { return reinterpret_cast<float *>(dev + (size_t)nvars * sizeof(AdaptiveRecord)); }
  AdaptivePartial *slab() const {
    return reinterpret_cast<AdaptivePartial *>(dev + (size_t)nvars * sizeof(AdaptiveRecord) + trust_bytes());
  }
};

// The norm pass's loads of w and g: 1 nontemporal, 0 plain.  Plain, taken over
// from the clipped step's measurement: the step re-reads both
// buffers right behind the pass and finds part of them on-die.
// $CBX_ADAPTIVE_NORM_LOADS = temporal | nontemporal overrides it for a
// measurement of its own; it is read by cbx_set_adaptive_rate and
// cbx_sma_plan_set_adaptive.
constexpr int kAdaptiveNormPolicy = 0;
inline int adaptive_norm_policy() {
  const char *e = getenv("CBX_ADAPTIVE_NORM_LOADS");
  if (e && strcmp(e, "temporal") == 0) return 0;
  if (e && strcmp(e, "nontemporal") == 0) return 1;
  return kAdaptiveNormPolicy;
}

// trust (eta), epsilon, the stepping replica's weight decay (beta) and the mode
// (0 LARS, 1 LARC: the ratio capped at 1) of one call.
struct AdaptiveParams {
  float trust, epsilon, weight_decay;
  int mode;
};

// Uploads the piece table of `plan` (blocking) after freeing what `t` held.
// enable[0 .. nvars): 0 excludes a variable; nullptr: every variable is on.
hipError_t adaptive_tables_upload(AdaptiveTables &t, const StatsPlan &plan, const unsigned char *enable);
// One variable's flag (blocking; the caller has drained the device).
hipError_t adaptive_tables_set_enable(AdaptiveTables &t, uint32_t v, bool on);
void adaptive_tables_free(AdaptiveTables &t);

// One allocation for the variable list of `t`, zeroed (blocking).
hipError_t adaptive_scratch_alloc(AdaptiveScratch &s, const AdaptiveTables &t);
void adaptive_scratch_free(AdaptiveScratch &s);

// The two-buffer pass over w[0, n) and g[0, n) and, right behind it on the same
// stream, the one-wave-per-variable kernel that leaves W_v, G_v, K_v, the trust
// ratio and the flags in the records and the ratio in the dense trust table.
// w and g are 16-byte aligned; nothing past float n - 1 is read.  policy: 0
// plain, 1 nontemporal loads.  Each launch stamps its own optional timing pair.
hipError_t launch_variable_norms(const float *w, const float *g, const AdaptiveTables &t, const AdaptiveScratch &s,
                                 const AdaptiveParams &p, int policy, hipStream_t stream, Timing pass = {},
                                 Timing reduce = {});

// launch_sma_optimise_variables over [0, t.elements) with
// r_v = (a.rate * mult[v]) * trust[v]: two fp32 multiplies in that order.
// mult: t.mult, or AdaptiveTables::ones(); both and `trust` hold t.nvars
// floats.  a.lo and a.hi are set by the launcher.  Refuses what that launcher
// refuses.
hipError_t launch_sma_optimise_adaptive(const VarTables &t, VarOptArgs a, const float *mult, const float *trust,
                                        const LaunchConfig &cfg, hipStream_t stream, Timing tm = {});

}  // namespace cbx
