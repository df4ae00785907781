// averaging_kernels.hip -- HIP kernels of the elastic-averaging and
// Polyak-Ruppert barriers for CDNA4 (gfx950).
//
// The reference runs either step as 3-4 cuBLAS saxpy calls plus a device copy
// per replica (clib-multigpu/synch/synchronouseamsgd.c:42-90,
// synch/polyakruppert.c:42-137), moving the model about 5R times.  Here, as
// for SMA (sma_kernels.hip), one streaming pass reads every input once and
// writes every output once:
//
//   fused (1 GPU)     reads z, w_i (, s_i)   writes w_i, z (, last)
//   accumulate (A)    reads z, w_i (, s_i)   writes w_i, acc
//   apply (B)         reads D, z             writes z (, last) (, flagged w_i)
//
// Elastic averaging moves (2R+2)n floats at G = 1; Polyak-Ruppert the same,
// plus n when base->last exists.  Same shape as the SMA kernels: 16-byte
// float4s per lane, every load of a replica chunk issued before the first
// arithmetic, the running sum in registers, no LDS.
//
// Arithmetic is the reference's: one fp32 fma per cuBLAS saxpy element, in
// the reference's operation order (built with -ffp-contract=off).
#include <hip/hip_ext.h>

#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {
namespace {

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane, as in the SMA kernels (sma_tail_elem, sma_kernels.hip): the fma
// sequence per element, the chunked replica walk and the three Polyak-Ruppert
// rules are those of the float4 path below.
template <int MODEL, int PHASE, bool LAST>
__device__ __forceinline__ void averaging_tail_elem(const AvgArgs &a) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  float z0 = z[i];
  float acc;
  if constexpr (PHASE == 2) {
    acc = reinterpret_cast<const float *>(a.D)[i];
  } else {
    // polyakruppert.c:72: with alpha == 0 the replicas are read, never written
    const bool move = MODEL != kPolyak || a.alpha != 0.0f;
    acc = 0.0f;  // synchronouseamsgd.c:43, polyakruppert.c:43
    // every load of a chunk issued before its first store (sma_tail_elem)
    for (int c = 0; c < a.nrep; c += kChunk) {
      [[maybe_unused]] float sv[kChunk];
      float wv[kChunk];
#pragma unroll
      for (int r = 0; r < kChunk; ++r) {
        if (c + r < a.nrep) {
          if constexpr (MODEL == kElasticS) sv[r] = reinterpret_cast<const float *>(a.s[c + r])[i];
          wv[r] = reinterpret_cast<const float *>(a.w[c + r])[i];
        }
      }
#pragma unroll
      for (int r = 0; r < kChunk; ++r) {
        if (c + r < a.nrep) {
          float w1;
          if constexpr (MODEL == kPolyak) {
            acc = fmaf(a.scale, wv[r], acc);           // polyakruppert.c:51-56
            const float d = fmaf(-1.0f, z0, wv[r]);    // :63-69
            w1 = fmaf(-a.alpha, d, wv[r]);             // :72-79
          } else {
            const float d = fmaf(-1.0f, z0, MODEL == kElasticS ? sv[r] : wv[r]);  // synchronouseamsgd.c:55-61, :181-192
            w1 = fmaf(-a.alpha, d, wv[r]);             // :64-69
            acc = fmaf(a.alpha, d, acc);               // :72-77
          }
          // a flagged replica takes z below (fused) or in the apply phase
          if (move && !(MODEL == kPolyak && ((a.copy_mask >> (c + r)) & 1ull)))
            reinterpret_cast<float *>(a.w[c + r])[i] = w1;
        }
      }
    }
    if constexpr (PHASE == 1) {
      reinterpret_cast<float *>(a.acc)[i] = acc;
      return;
    }
  }
  if constexpr (MODEL == kPolyak) {
    const float L = fmaf(-1.0f, z0, acc);  // polyakruppert.c:98-104
    if constexpr (LAST) reinterpret_cast<float *>(a.last)[i] = L;
    z0 = fmaf(a.running, L, z0);  // :107-112
  } else {
    z0 = fmaf(1.0f, acc, z0);  // synchronouseamsgd.c:85-90
  }
  z[i] = z0;
  if constexpr (MODEL == kPolyak) {
    for (uint64_t m = a.copy_mask; m != 0; m &= m - 1)
      reinterpret_cast<float *>(a.w[__builtin_ctzll(m)])[i] = z0;  // polyakruppert.c:122-137
  }
}

// ---------------------------------------------------------------------------
// One kernel for {kElasticW, kElasticS, kPolyak} x PHASE {0 fused, 1
// accumulate-only, 2 apply}.  R >= 1 replicas fully unrolled (R <= kChunk);
// R == -1 takes a.nrep and walks the replicas in register-resident chunks of
// kChunk.  PHASE 2 touches no replica but kPolyak's flagged ones (R unused).
//
// Elastic averaging, per element (synchronouseamsgd.c; x_i is w_i on one
// device, :55-61, and the snapshot s_i on several, :181-192):
//   d   = fma(-1, z, x_i)              :55-61
//   w_i = fma(-alpha, d, w_i)          :64-69
//   acc = fma(+alpha, d, acc)          :72-77   (acc starts at +0, :43)
//   z   = fma(1, D, z)                 :85-90   (D = acc, all-reduced at G > 1)
// Polyak-Ruppert, per element (polyakruppert.c):
//   acc = fma(1/p, w_i, acc)           :51-56   (acc starts at +0, :43)
//   d   = fma(-1, z, w_i)              :63-69
//   w_i = fma(-alpha, d, w_i)          :72-79   (only if alpha != 0)
//   L   = fma(-1, z, D); last = L      :98-104  (D = acc, all-reduced at G > 1)
//   z   = fma(1/(clock+1), L, z)       :107-112
//   w_i = z                            :122-137 (only replicas whose copy flag is raised)
// ---------------------------------------------------------------------------
template <int MODEL, int PHASE, int R, bool LAST, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void averaging_kernel(const AvgArgs a) {
  constexpr int RR = (R > 0) ? R : kChunk;
  constexpr int RS = (MODEL == kElasticS) ? RR : 1;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      averaging_tail_elem<MODEL, PHASE, LAST>(a);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f al = a.alpha, nal = -a.alpha, sc = a.scale, ru = a.running, one = 1.0f, mone = -1.0f;
  // polyakruppert.c:72: with alpha == 0 the replicas are read, never written
  const bool move = MODEL != kPolyak || a.alpha != 0.0f;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    v4f zv[U], acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      zv[u] = ldo<P>(a.z, i);
      if constexpr (PHASE == 2) acc[u] = ldo<P>(a.D, i);
      else acc[u] = 0.0f;
    }
    if constexpr (PHASE != 2) {
      const int nrep = (R >= 0) ? R : a.nrep;
      for (int c = 0; c < nrep; c += RR) {
        [[maybe_unused]] v4f sv[U][RS];
        v4f wv[U][RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) {
          if (R < 0 && c + r >= nrep) break;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint32_t i = (base + u * 64u) * 16u;
            if constexpr (MODEL == kElasticS) sv[u][r] = ldo<P>(a.s[c + r], i);
            wv[u][r] = ldo<P>(a.w[c + r], i);
          }
        }
        // every load of the chunk in flight before the first use (sma_fused_kernel)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < RR; ++r) {
          if (R < 0 && c + r >= nrep) break;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if constexpr (MODEL == kPolyak) {
              acc[u] = vfma(sc, wv[u][r], acc[u]);
              const v4f d = vfma(mone, zv[u], wv[u][r]);
              if (move) wv[u][r] = vfma(nal, d, wv[u][r]);
            } else {
              const v4f d = vfma(mone, zv[u], MODEL == kElasticS ? sv[u][r] : wv[u][r]);
              wv[u][r] = vfma(nal, d, wv[u][r]);
              acc[u] = vfma(al, d, acc[u]);
            }
          }
        }
        if (move) {
#pragma unroll
          for (int r = 0; r < RR; ++r) {
            if (R < 0 && c + r >= nrep) break;
            // a flagged replica takes z below (fused) or in the apply phase
            if (MODEL == kPolyak && ((a.copy_mask >> (c + r)) & 1ull)) continue;
#pragma unroll
            for (int u = 0; u < U; ++u) sto<P>(a.w[c + r], (base + u * 64u) * 16u, wv[u][r]);
          }
        }
        if constexpr (R >= 0) break;
      }
    } else {
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (PHASE == 1) {
#pragma unroll
      for (int u = 0; u < U; ++u) sto<P>(a.acc, (base + u * 64u) * 16u, acc[u]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t i = (base + u * 64u) * 16u;
        if constexpr (MODEL == kPolyak) {
          const v4f L = vfma(mone, zv[u], acc[u]);
          if constexpr (LAST) sto<P>(a.last, i, L);
          zv[u] = vfma(ru, L, zv[u]);
        } else {
          zv[u] = vfma(one, acc[u], zv[u]);
        }
        sto<P>(a.z, i, zv[u]);
      }
      if constexpr (MODEL == kPolyak) {
        for (uint64_t m = a.copy_mask; m != 0; m &= m - 1) {
          const int r = __builtin_ctzll(m);
#pragma unroll
          for (int u = 0; u < U; ++u) sto<P>(a.w[r], (base + u * 64u) * 16u, zv[u]);
        }
      }
    }
  }
}

// Buffer streams per lane (reads, writes) of a launch, for the occupancy cap.
void stream_counts(int model, int phase, const AvgArgs &a, int *reads, int *writes) {
  const int flagged = __builtin_popcountll(a.copy_mask);
  if (phase == 2) {
    *reads = 2;
    *writes = 1 + (model == kPolyak ? (a.last ? 1 : 0) + flagged : 0);
    return;
  }
  const bool move = model != kPolyak || a.alpha != 0.0f;
  *reads = 1 + (model == kElasticS ? 2 : 1) * a.nrep;
  *writes = 1 + (move ? a.nrep : 0) + (phase == 0 && model == kPolyak && a.last ? 1 : 0);
}

template <int MODEL, int PHASE, int R, bool LAST, int P>
hipError_t avg_u(const AvgArgs &a0, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a0.n4);
  const bool tail = a0.tail_hi > a0.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop.  The context's padded buffers are
  // whole kPadFloat4s; the bulk of a caller-owned buffer is whole chunks only
  // (e.g. 1,280 float4s), and may be empty when a tail is all there is.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.unroll < 1 || a0.n4 < 0 || a0.n4 % (64ll * cfg.unroll) != 0 ||
      (a0.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a0.n4 > 0 ? grid_for(a0.n4, cfg) : dim3(0);
  const AvgArgs &a = a0;
  int reads = 0, writes = 0;
  stream_counts(MODEL, PHASE, a, &reads, &writes);
  // Auto occupancy: the apply phase as SMA's kernel B (kStreamsPerCU), the
  // replica phases from kAveragingStreamsPerCU; a launch too small to fill
  // the chip stays uncapped (lds_for_occupancy).
  LaunchConfig cap = cfg;
  if (PHASE != 2 && cfg.waves_per_cu < 0 && (int64_t)g.x * ((cfg.block + 63) / 64) >= 16ll * cfg.num_cus) {
    const int streams = reads + writes;
    const int w = (kAveragingStreamsPerCU + streams / 2) / streams;
    cap.waves_per_cu = w < 2 ? 2 : (w > 12 ? 12 : w);
  }
  const unsigned lds = lds_for_occupancy(cap, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    if constexpr (P != 1) {
      return hipErrorInvalidValue;
    } else {
      AvgArgs b = a0;
      b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
      g.x += (unsigned)b.tail_blocks;
      if (cfg.unroll == 2)
        hipExtLaunchKernelGGL((averaging_kernel<MODEL, PHASE, R, LAST, P, true, 2>), g, dim3(cfg.block), lds, s, t.start, t.stop, 0, b);
      else if (cfg.unroll == 1)
        hipExtLaunchKernelGGL((averaging_kernel<MODEL, PHASE, R, LAST, P, true, 1>), g, dim3(cfg.block), lds, s, t.start, t.stop, 0, b);
      else
        return hipErrorInvalidValue;
      return hipGetLastError();
    }
  }
  if (cfg.unroll == 4)
    hipExtLaunchKernelGGL((averaging_kernel<MODEL, PHASE, R, LAST, P, false, 4>), g, dim3(cfg.block), lds, s, t.start, t.stop, 0, a);
  else if (cfg.unroll == 2)
    hipExtLaunchKernelGGL((averaging_kernel<MODEL, PHASE, R, LAST, P, false, 2>), g, dim3(cfg.block), lds, s, t.start, t.stop, 0, a);
  else
    hipExtLaunchKernelGGL((averaging_kernel<MODEL, PHASE, R, LAST, P, false, 1>), g, dim3(cfg.block), lds, s, t.start, t.stop, 0, a);
  return hipGetLastError();
}

template <int MODEL, int PHASE, bool LAST, int P>
hipError_t avg_r(const AvgArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  switch (a.nrep) {
    case 1: return avg_u<MODEL, PHASE, 1, LAST, P>(a, cfg, s, t);
    case 2: return avg_u<MODEL, PHASE, 2, LAST, P>(a, cfg, s, t);
    case 3: return avg_u<MODEL, PHASE, 3, LAST, P>(a, cfg, s, t);
    case 4: return avg_u<MODEL, PHASE, 4, LAST, P>(a, cfg, s, t);
    case 5: return avg_u<MODEL, PHASE, 5, LAST, P>(a, cfg, s, t);
    case 6: return avg_u<MODEL, PHASE, 6, LAST, P>(a, cfg, s, t);
    case 7: return avg_u<MODEL, PHASE, 7, LAST, P>(a, cfg, s, t);
    case 8: return avg_u<MODEL, PHASE, 8, LAST, P>(a, cfg, s, t);
    default: return avg_u<MODEL, PHASE, -1, LAST, P>(a, cfg, s, t);  // 0 or more than kChunk
  }
}

template <int MODEL, int PHASE, bool LAST>
hipError_t avg_p(const AvgArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if constexpr (PHASE == 2)
    return cfg.policy == 1 ? avg_u<MODEL, 2, 0, LAST, 1>(a, cfg, s, t) : avg_u<MODEL, 2, 0, LAST, 0>(a, cfg, s, t);
  else
    return cfg.policy == 1 ? avg_r<MODEL, PHASE, LAST, 1>(a, cfg, s, t) : avg_r<MODEL, PHASE, LAST, 0>(a, cfg, s, t);
}

}  // namespace

// The snapshot form exists only where the step is split (G > 1).
hipError_t launch_averaging_fused(AvgModel m, const AvgArgs &a, const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (m == kElasticW) return avg_p<kElasticW, 0, false>(a, cfg, stream, t);
  if (m == kPolyak) return a.last ? avg_p<kPolyak, 0, true>(a, cfg, stream, t) : avg_p<kPolyak, 0, false>(a, cfg, stream, t);
  return hipErrorInvalidValue;
}

hipError_t launch_averaging_accumulate(AvgModel m, const AvgArgs &a, const LaunchConfig &cfg, hipStream_t stream,
                                       Timing t) {
  switch (m) {
    case kElasticW: return avg_p<kElasticW, 1, false>(a, cfg, stream, t);
    case kElasticS: return avg_p<kElasticS, 1, false>(a, cfg, stream, t);
    case kPolyak: return avg_p<kPolyak, 1, false>(a, cfg, stream, t);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_averaging_apply(AvgModel m, const AvgArgs &a, const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (m == kPolyak) return a.last ? avg_p<kPolyak, 2, true>(a, cfg, stream, t) : avg_p<kPolyak, 2, false>(a, cfg, stream, t);
  return avg_p<kElasticW, 2, false>(a, cfg, stream, t);  // both elastic forms apply alike
}

}  // namespace cbx
