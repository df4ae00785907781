// optimise_plan.h -- the chunk table of the per-variable replica step
// (variable_rate_kernels.hip, cbx_set_variable_learning_rates,
// cbx_replica_optimise_variables), and the kernels' lookup in it (variable_of).
// Plain C++ that needs no HIP: the builder and the lookup are tested on the
// CPU (tests/native/optimise_plan_test.cpp).
//
// A model buffer is a run of variables whose offsets are a running sum
// (ModelDef::offset, model.c:127-157), not multiples of 16 bytes.  The kernel
// moves it in chunks of kOptChunk floats, one wave's trip of 64 float4s, and
// needs every float's learning-rate multiplier.  For all but the few chunks
// that hold a variable boundary that is one value per chunk, so the table
// holds one 32-bit entry per chunk: the variable of the chunk's first float,
// shifted left by one, with bit 0 set iff a boundary lies strictly inside the
// chunk (a "mixed" chunk).  In a mixed chunk each lane finds the variable of
// each of its floats in the sorted boundary array `bounds` (nvars + 1 running
// offsets, bounds[0] = 0, bounds[nvars] = elements): the variable of float f
// is the one v with bounds[v] <= f < bounds[v + 1], which skips zero-length
// variables and copes with several boundaries inside one float4.  The table
// depends on the variables alone, not on the launch shape.
#pragma once

#include <cstdint>
#include <vector>

namespace cbx {

// Floats per chunk: 64 lanes x one float4.
constexpr uint32_t kOptChunk = 256;

struct OptimisePlan {
  std::vector<uint32_t> chunks;  // ceil(elements / kOptChunk) entries: (variable << 1) | mixed
  std::vector<uint32_t> bounds;  // nvars + 1 running offsets in floats
  int64_t elements = 0;
  int nvars = 0;
};

inline uint32_t opt_chunk_var(uint32_t entry) { return entry >> 1; }
inline bool opt_chunk_mixed(uint32_t entry) { return (entry & 1u) != 0; }

#ifdef __HIPCC__
#define CBX_OPT_INLINE __host__ __device__ __forceinline__
#else
#define CBX_OPT_INLINE inline
#endif
// The kernels' lookup in a mixed chunk: the variable of float f, at or after v0
// (the variable of the chunk's first float), i.e. the last v with
// bounds[v] <= f.  bounds[nvars] = elements > f.
CBX_OPT_INLINE uint32_t variable_of(const uint32_t *__restrict__ bounds, uint32_t nvars, uint32_t v0, uint32_t f) {
  uint32_t lo = v0, hi = nvars;
  while (hi - lo > 1u) {
    const uint32_t m = (lo + hi) >> 1;
    if (bounds[m] <= f) lo = m;
    else hi = m;
  }
  return lo;
}
#undef CBX_OPT_INLINE

// var_elements[0 .. nvars): floats per variable, in offset order; they must
// sum to `elements`.  False on no variables, negative counts, a wrong sum, or
// more than 2^32 - 1 bytes per buffer (the kernels use 32-bit byte offsets).
inline bool build_optimise_plan(const long long *var_elements, int nvars, long long elements, OptimisePlan *out) {
  out->chunks.clear();
  out->bounds.clear();
  out->elements = 0;
  out->nvars = 0;
  if (elements <= 0 || elements > (long long)(0xffffffffull / 4)) return false;
  if (nvars <= 0 || var_elements == nullptr) return false;
  long long sum = 0;
  for (int v = 0; v < nvars; ++v) {
    if (var_elements[v] < 0 || var_elements[v] > elements) return false;
    sum += var_elements[v];
    if (sum > elements) return false;
  }
  if (sum != elements) return false;
  out->bounds.reserve((size_t)nvars + 1);
  uint64_t at = 0;
  out->bounds.push_back(0);
  for (int v = 0; v < nvars; ++v) {
    at += (uint64_t)var_elements[v];
    out->bounds.push_back((uint32_t)at);
  }
  const uint64_t n = (uint64_t)elements;
  const uint64_t nchunks = (n + kOptChunk - 1) / kOptChunk;
  out->chunks.resize((size_t)nchunks);
  // `v` walks forward to the variable of each chunk's first float: the last
  // one that starts at or before it (zero-length variables are passed over).
  uint32_t v = 0;
  for (uint64_t c = 0; c < nchunks; ++c) {
    const uint64_t lo = c * kOptChunk, hi = lo + kOptChunk;
    while (out->bounds[v + 1] <= lo) ++v;  // bounds[nvars] = n > lo ends it
    // the first boundary past lo: it is inside the chunk iff it is below hi.
    // bounds[nvars] is the end of the model, not a boundary between variables.
    uint32_t b = v + 1;
    const bool mixed = b < (uint32_t)nvars && out->bounds[b] < hi;
    out->chunks[(size_t)c] = (v << 1) | (mixed ? 1u : 0u);
  }
  out->elements = elements;
  out->nvars = nvars;
  return true;
}

// The table of a buffer padded to `padded_elements` >= elements floats (the
// context's buffers, whole kPadFloat4s): the pad floats belong to a last
// pseudo-variable, index nvars, which the caller gives the multiplier 1, so a
// kernel that sweeps the padded length (task_barrier_variables_kernels.hip)
// reads no table past its end and steps a zero pad to zero.  The floats
// [0, elements) keep their own variables: a last partial chunk becomes a mixed
// chunk.  out->nvars is nvars + 1, out->elements the padded length; with no
// pad the pseudo-variable has no floats and no chunk names it.
inline bool build_padded_optimise_plan(const long long *var_elements, int nvars, long long elements,
                                       long long padded_elements, OptimisePlan *out) {
  OptimisePlan plain;
  if (padded_elements < elements || !build_optimise_plan(var_elements, nvars, elements, &plain)) {
    build_optimise_plan(nullptr, 0, 0, out);  // clears *out
    return false;
  }
  std::vector<long long> v(var_elements, var_elements + nvars);
  v.push_back(padded_elements - elements);
  return build_optimise_plan(v.data(), nvars + 1, padded_elements, out);
}

}  // namespace cbx
