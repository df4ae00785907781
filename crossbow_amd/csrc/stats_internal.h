// stats_internal.h -- the model-statistics reduction (stats_kernels.hip) as the
// execution context (cbx_model_stats, the checkpoint guard) and the sma.c seam
// (cbx_sma_plan_buffer_stats) call it.  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/crossbow_sma.h"
#include "sma_internal.h"
#include "stats_plan.h"

namespace cbx {

// Kernel arguments of the one pass over memory.  Record (p, b) of the slab
// is piece p's partial result for buffer b: b = 0 the reference buffer,
// b = 1 + i buffer i.
struct StatsArgs {
  const float *bufs[kMaxReplicas];
  const float *ref;
  const StatsPiece *pieces;
  cbx_buffer_stats *slab;  // npieces * (nbufs + 1) records
  uint32_t npieces;
  int nbufs;
};

// What one device keeps between calls: the piece table of the last variable
// list (rebuilt only when the list changes) and the device scratch
//   [pieces][segments: var_first (nvars + 1), then {0, nvars}]
//   [totals: nb records][per variable: nvars * nb records][slab: npieces * nb]
// with nb = nbufs + 1.  Owned by a context's device or a plan's device; one
// call at a time, as for the step's own scratch.
struct StatsScratch {
  StatsPlan plan;
  std::vector<long long> key;  // the variable list the plan was built for
  bool uploaded = false;
  char *table = nullptr;  // pieces + segments
  size_t table_bytes = 0;
  char *records = nullptr;  // totals + per variable + slab
  size_t records_bytes = 0;
  std::vector<cbx_buffer_stats> host;  // totals + per variable, as copied back
  // Timestamps of the last call's dispatches themselves (no marker packets):
  // the pass starts `start` and stops `mid`, the second reduce stops `stop`.
  hipEvent_t start = nullptr, mid = nullptr, stop = nullptr;
  bool timed = false;
};

// One pass over `ref` and bufs[0 .. nbufs) (device pointers, `elements` floats
// each, 16-byte aligned) on `stream` of the current device, then the two
// launch-boundary reductions; blocks on `stream`.  totals: nbufs + 1 records
// (the reference first); vars: nvars * (nbufs + 1), [v * (nbufs + 1) + b], or
// nullptr.  Returns CBX_OK or a negative CBX_ERR_* with the message set.
int stats_run(StatsScratch &s, hipStream_t stream, const float *ref, const float *const *bufs, int nbufs,
              const long long *var_elements, int nvars, long long elements, cbx_buffer_stats *totals,
              cbx_buffer_stats *vars);
// Device milliseconds of the last stats_run on this scratch: the pass alone,
// and the pass with both reduces; -1 when there is none.
int stats_last_ms(StatsScratch &s, float *pass_ms, float *total_ms);
void stats_free(StatsScratch &s);

}  // namespace cbx
