// clip_kernels.hip -- the whole-model reduction behind gradient clipping by
// global L2 norm and the non-finite skip of the replica optimiser step, for
// CDNA4 (gfx950).  cbx_set_gradient_clip, cbx_sma_plan_optimise_clipped.
//
// The optimiser step is a streaming map; clipping needs S = sum g_i^2 over the
// whole model before the first element steps, with no host round trip (the
// step is enqueued on a task stream).  Two launches in front of the step, on
// the same stream:
//
//   pass      read-only over g: one one-wave workgroup per tile of kClipTile
//             floats.  Lane l takes float4s l, l + 64, ... of its tile in
//             order (every load of a group issued before the first add), then
//             a trailing float if the model ends inside a float4.  Each lane
//             accumulates in fp64 from the first add: (double)x * (double)x is
//             exact (48 significant bits), so only the adds round.  A
//             non-finite x adds nothing and counts.  The wave folds its lanes
//             with a fixed xor butterfly and lane 0 writes one 16-byte partial
//             (S_t, K_t) to the replica's slab.
//   reduce    one wave: lane l sums partials l, l + 64, ... in order, the same
//             butterfly, then one lane takes the decision
//               clipped = c > 0 && S > (double)c * (double)c   (exact product)
//               scale   = clipped ? (float)((double)c / sqrt(S)) : 1
//               skipped = skip_nonfinite && K > 0
//             and updates the replica's record in plain C++.
//
// No float atomics and no order that depends on arrival: tiles, grid and both
// trees are fixed functions of n alone (never of the CU count, a launch
// tunable or the stream), so context and seam return the same bits on the
// same data.  The CLIP instantiations of the two step kernels
// (sma_kernels.hip, variable_rate_kernels.hip) read the record behind them.
#include <hip/hip_ext.h>

#include "clip_internal.h"

namespace cbx {
namespace {

static_assert(sizeof(ClipRecord) == 48, "cbx_clip_stats is 48 bytes without padding");
static_assert(sizeof(ClipPartial) == 16, "one 16-byte partial per tile");

template <int P>
__device__ __forceinline__ v4f ldg4(const float *base, uint32_t off) {
  const v4f *p = reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

__device__ __forceinline__ void add_sq(double &q, uint32_t &nf, float x) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const double xd = fin ? (double)x : 0.0;
  q = fma(xd, xd, q);  // the product is exact: one rounding, the add's
  nf += fin ? 0u : 1u;
}

// float4 loads in flight per lane before the first add (16 per full tile).
constexpr int kClipDepth = 8;

template <int P>
__global__ __launch_bounds__(64) void gradient_norm_kernel(const float *__restrict__ g, uint32_t n,
                                                           ClipPartial *__restrict__ slab) {
  const uint32_t lane = threadIdx.x;
  const uint32_t lo = blockIdx.x * kClipTile;  // < n <= 2^30
  const uint32_t hi = n - lo < kClipTile ? n : lo + kClipTile;
  double q = 0.0;
  uint32_t nf = 0;
  if (hi - lo == kClipTile) {
#pragma unroll
    for (uint32_t j = 0; j < kClipTile / 256u; j += kClipDepth) {
      v4f x[kClipDepth];
#pragma unroll
      for (uint32_t u = 0; u < (uint32_t)kClipDepth; ++u) x[u] = ldg4<P>(g, ((lo >> 2) + (j + u) * 64u + lane) * 16u);
      __builtin_amdgcn_sched_barrier(0);  // every load of the group in flight first (see the fused SMA kernel)
#pragma unroll
      for (int u = 0; u < kClipDepth; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) add_sq(q, nf, x[u][k]);
      }
    }
  } else {
    // The model's last tile: whole float4s with a bound, then the floats
    // past the last one (an unpadded buffer ends there; a padded one's pad
    // is not part of the model).
    const uint32_t n4 = (hi - lo) >> 2;
    for (uint32_t i = lane; i < n4; i += 64u) {
      const v4f x = ldg4<P>(g, ((lo >> 2) + i) * 16u);
#pragma unroll
      for (int k = 0; k < 4; ++k) add_sq(q, nf, x[k]);
    }
    const uint32_t f = lo + n4 * 4u + lane;
    if (f < hi) add_sq(q, nf, g[f]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // fixed xor butterfly: every lane ends with the same bits
    q += __shfl_xor(q, o);
    nf += __shfl_xor(nf, o);
  }
  if (lane == 0) {
    slab[blockIdx.x].sum_sq = q;
    slab[blockIdx.x].nonfinite = nf;
  }
}

// Partials in flight per lane of the reduce.
constexpr int kReduceDepth = 16;

__global__ __launch_bounds__(64) void gradient_norm_reduce_kernel(const ClipPartial *__restrict__ slab, uint32_t tiles,
                                                                  float max_norm, int skip_nonfinite,
                                                                  ClipRecord *rec) {
  const uint32_t lane = threadIdx.x;
  double S = 0.0;
  unsigned long long K = 0;
  // Lane l adds partials l, l + 64, ... in that order; their loads go out
  // kReduceDepth at a time (one at a time the wave paid an HBM round trip per
  // partial: 25 us for ResNet-50's 6,240 tiles).  A slot past the end adds
  // +0, which leaves the non-negative sum's bits alone.
  for (uint32_t i0 = lane; i0 < tiles; i0 += 64u * kReduceDepth) {
    ClipPartial p[kReduceDepth];
#pragma unroll
    for (uint32_t u = 0; u < (uint32_t)kReduceDepth; ++u) {
      const uint32_t i = i0 + u * 64u;
      p[u] = i < tiles ? slab[i] : ClipPartial{0.0, 0ull};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kReduceDepth; ++u) {
      S += p[u].sum_sq;
      K += p[u].nonfinite;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    S += __shfl_xor(S, o);
    K += __shfl_xor(K, o);
  }
  if (lane == 0) {
    const double c = (double)max_norm;
    const bool clipped = max_norm > 0.0f && S > c * c;  // c * c is exact in fp64: no square root in the decision
    const bool skipped = skip_nonfinite != 0 && K > 0;
    rec->sum_sq = S;
    rec->nonfinite = K;
    rec->scale = clipped ? (float)(c / sqrt(S)) : 1.0f;
    rec->flags = (clipped ? kClipClipped : 0u) | (skipped ? kClipSkipped : 0u);
    rec->steps += 1;
    rec->clipped_steps += clipped ? 1 : 0;
    rec->skipped_steps += skipped ? 1 : 0;
  }
}

}  // namespace

hipError_t clip_scratch_alloc(ClipScratch &s, int64_t n) {
  clip_scratch_free(s);
  if (n <= 0 || n > (int64_t)(0xffffffffull / 4)) return hipErrorInvalidValue;
  const uint32_t tiles = clip_tiles(n);
  const size_t bytes = 64 + (size_t)tiles * sizeof(ClipPartial);
  char *dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), bytes);
  if (e != hipSuccess) return e;
  // hipMemset of device memory may return before it has run, and a caller's
  // non-blocking stream does not wait for the null stream: without the
  // synchronise a first step could have its fresh record zeroed under it.
  e = hipMemset(dev, 0, bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return e;
  }
  s.dev = dev;
  s.tiles = tiles;
  return hipSuccess;
}

void clip_scratch_free(ClipScratch &s) {
  if (s.dev) (void)hipFree(s.dev);
  s = ClipScratch();
}

hipError_t launch_gradient_norm(const float *g, int64_t n, const ClipScratch &s, float max_norm, bool skip_nonfinite,
                                int policy, hipStream_t stream, Timing pass, Timing reduce) {
  if (!g || !s.dev || n <= 0 || clip_tiles(n) != s.tiles || (reinterpret_cast<uintptr_t>(g) & 15u) != 0)
    return hipErrorInvalidValue;
  const dim3 grid(s.tiles), block(64);
  if (policy == 1)
    hipExtLaunchKernelGGL((gradient_norm_kernel<1>), grid, block, 0, stream, pass.start, pass.stop, 0, g, (uint32_t)n,
                          s.slab());
  else
    hipExtLaunchKernelGGL((gradient_norm_kernel<0>), grid, block, 0, stream, pass.start, pass.stop, 0, g, (uint32_t)n,
                          s.slab());
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipExtLaunchKernelGGL(gradient_norm_reduce_kernel, dim3(1), block, 0, stream, reduce.start, reduce.stop, 0,
                        (const ClipPartial *)s.slab(), s.tiles, max_norm, skip_nonfinite ? 1 : 0, s.record());
  return hipGetLastError();
}

}  // namespace cbx
