// variable_rate_kernels.hip -- the replica optimiser step with a learning
// rate per variable, for CDNA4 (gfx950).
//
// crossbowKernelOptimiserSMA (kernels/optimisers/sma.cu:3-100) steps every
// variable with crossbowModelGetLearningRateForVariable's rate (model.c:159-177:
// rate *= multiplier when conf->irregular > 0), and the per-operator
// crossbowStreamSynchronousEamsgdModelUpdate (stream.c:422-479) steps only the
// variables of the operator whose gradient has just been produced.  Both are
// one kernel here: sma_optimise_kernel (sma_kernels.hip) plus a rate lookup
// and a float range [lo, hi).  Per element of variable v, with
// r_v = rate * mult[v] (rate = -lr, one fp32 multiply; the reference multiplies
// +lr and negates, which is exact):
//   g = fma(wd, w, g)                       (wd > 0)
//   g = r_v * g ; g = fma(mu, last, g) ; last = g ; s = w ; w = fma(1, g, w)
//   without momentum:  s = w ; w = fma(r_v, g, w)
// g and last keep sma.cu's sign (the negative-rate values); stream.c:455-467
// scales by +rate and subtracts, which gives the same w bits and g / last of
// the opposite sign.  s = w is taken per element in the ranged form as well.
//
// The lookup is per wave: a wave's trip of 64 float4s is one 256-float chunk
// and reads one entry of the host-built chunk table (optimise_plan.h) through
// a wave-uniform address, i.e. scalar loads; r_v then sits in a scalar
// register and the float4 path is sma_optimise_kernel's.  A chunk with a
// variable boundary inside it (142 of ResNet-50's 99,833) still moves
// float4s, but each lane finds the variable of each of its four floats in
// the sorted boundary array (a float4 may straddle several variables).  A
// chunk that is not wholly inside [lo, hi) takes the edge path: one float at
// a time, 4-byte loads and stores for the in-range floats only, so nothing
// outside the range is written, not even with its own value, and nothing past
// `hi` is read (caller-owned buffers hold exactly `elements` floats).  The
// kernels only read the tables; per task only the scalar rate travels, in the
// kernel arguments.
#include <hip/hip_ext.h>

#include <cstring>
#include <vector>

#include "clip_internal.h"
#include "optimise_plan.h"
#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {
namespace {

// CLIP: as sma_optimise_kernel's (sma_kernels.hip): g = scale * g before weight
// decay on all three paths, s = w alone when the record carries the skip bit.
template <bool MOM, bool WD, int P, int U, bool CLIP>
__global__ __launch_bounds__(512) void sma_optimise_variables_kernel(const VarOptArgs a,
                                                                           const uint32_t *__restrict__ chunks,
                                                                           const uint32_t *__restrict__ bounds,
                                                                           const float *__restrict__ mult,
                                                                           const ClipRecord *__restrict__ clip) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t wave =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const v4f mu = a.momentum, wd = a.wd, one = 1.0f;
  for (uint32_t c = a.chunk_lo + wave * U; c < a.chunk_hi; c += waves * U) {
    // wave-uniform: are all U chunks wholly inside [lo, hi)?
    if (c * kOptChunk >= a.lo && (c + U) * kOptChunk <= a.hi) {
      v4f w[U], g[U], l[U], r[U];
      uint32_t e[U];
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = chunks[c + u];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t i = ((c + u) * 64u + lane) * 16u;
        w[u] = ldo<P>(a.w, i);
        g[u] = ldo<P>(a.g, i);
        if constexpr (MOM) l[u] = ldo<P>(a.last, i);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (CLIP) {
        if ((clip->flags & kClipSkipped) != 0u) {  // wave-uniform
#pragma unroll
          for (int u = 0; u < U; ++u) sto<P>(a.s, ((c + u) * 64u + lane) * 16u, w[u]);
          continue;
        }
        const v4f scale = clip->scale;
#pragma unroll
        for (int u = 0; u < U; ++u) g[u] = scale * g[u];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t v0 = e[u] >> 1;
        if ((e[u] & 1u) == 0u) {
          r[u] = a.rate * mult[v0];  // uniform: a scalar load and a scalar register
        } else {
          const uint32_t f = (c + u) * kOptChunk + lane * 4u;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[u][k] = a.rate * mult[variable_of(bounds, a.nvars, v0, f + k)];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t i = ((c + u) * 64u + lane) * 16u;
        if constexpr (WD) g[u] = vfma(wd, w[u], g[u]);
        sto<P>(a.s, i, w[u]);
        if constexpr (MOM) {
          g[u] = r[u] * g[u];
          g[u] = vfma(mu, l[u], g[u]);
          sto<P>(a.last, i, g[u]);
          sto<P>(a.w, i, vfma(one, g[u], w[u]));
          sto<P>(a.g, i, g[u]);
        } else {
          sto<P>(a.w, i, vfma(r[u], g[u], w[u]));
          if constexpr (WD || CLIP) sto<P>(a.g, i, g[u]);
        }
      }
    } else {
      // Edge of the range (or of the buffer): the in-range floats one by one.
      float *wp = reinterpret_cast<float *>(a.w), *gp = reinterpret_cast<float *>(a.g);
      float *lp = reinterpret_cast<float *>(a.last), *sp = reinterpret_cast<float *>(a.s);
      for (int u = 0; u < U; ++u) {
        if (c + u >= a.chunk_hi) break;
        const uint32_t en = chunks[c + u];
        const uint32_t f0 = (c + u) * kOptChunk + lane * 4u;
        for (int k = 0; k < 4; ++k) {
          const uint32_t f = f0 + k;
          if (f < a.lo || f >= a.hi) continue;
          const uint32_t v = (en & 1u) ? variable_of(bounds, a.nvars, en >> 1, f) : (en >> 1);
          const float rv = a.rate * mult[v];
          const float wv = wp[f];
          float gv = gp[f];
          if constexpr (CLIP) {
            if ((clip->flags & kClipSkipped) != 0u) {
              sp[f] = wv;
              continue;
            }
            gv = clip->scale * gv;
          }
          if constexpr (WD) gv = fmaf(a.wd, wv, gv);
          sp[f] = wv;
          if constexpr (MOM) {
            gv = rv * gv;
            gv = fmaf(a.momentum, lp[f], gv);
            lp[f] = gv;
            wp[f] = fmaf(1.0f, gv, wv);
            gp[f] = gv;
          } else {
            wp[f] = fmaf(rv, gv, wv);
            if constexpr (WD || CLIP) gp[f] = gv;
          }
        }
      }
    }
  }
}

template <bool MOM, bool WD, int P, bool CLIP>
hipError_t variables_p(const VarTables &vt, const VarOptArgs &a, const ClipRecord *rec, const LaunchConfig &cfg,
                       hipStream_t stream, Timing t) {
  const int reads = 2 + (MOM ? 1 : 0), writes = MOM ? 4 : ((WD || CLIP) ? 3 : 2);
  const int64_t n4 = (int64_t)(a.chunk_hi - a.chunk_lo) * 64;
  const dim3 g = grid_for(n4, cfg);
  const unsigned l = lds_for_occupancy(cfg, reads, writes, g.x);
  if (cfg.unroll == 2)
    hipExtLaunchKernelGGL((sma_optimise_variables_kernel<MOM, WD, P, 2, CLIP>), g, dim3(cfg.block), l, stream,
                          t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, rec);
  else if (cfg.unroll == 1)
    hipExtLaunchKernelGGL((sma_optimise_variables_kernel<MOM, WD, P, 1, CLIP>), g, dim3(cfg.block), l, stream,
                          t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, rec);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

template <bool CLIP>
hipError_t variables_c(const VarTables &t, VarOptArgs a, const ClipRecord *rec, const LaunchConfig &cfg,
                       hipStream_t stream, Timing tm) {
  if (!t.chunks || a.lo > a.hi || a.hi > t.elements || cfg.block < 64 || cfg.block % 64 != 0 || cfg.block > 512)
    return hipErrorInvalidValue;
  if (a.lo == a.hi) return hipSuccess;
  a.nvars = t.nvars;
  a.chunk_lo = a.lo / kOptChunk;
  a.chunk_hi = (a.hi + kOptChunk - 1) / kOptChunk;
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (cfg.policy == 1) {
    if (mom)
      return wd ? variables_p<true, true, 1, CLIP>(t, a, rec, cfg, stream, tm)
                : variables_p<true, false, 1, CLIP>(t, a, rec, cfg, stream, tm);
    return wd ? variables_p<false, true, 1, CLIP>(t, a, rec, cfg, stream, tm)
              : variables_p<false, false, 1, CLIP>(t, a, rec, cfg, stream, tm);
  }
  if (mom)
    return wd ? variables_p<true, true, 0, CLIP>(t, a, rec, cfg, stream, tm)
              : variables_p<true, false, 0, CLIP>(t, a, rec, cfg, stream, tm);
  return wd ? variables_p<false, true, 0, CLIP>(t, a, rec, cfg, stream, tm)
            : variables_p<false, false, 0, CLIP>(t, a, rec, cfg, stream, tm);
}

}  // namespace

hipError_t launch_sma_optimise_variables(const VarTables &t, VarOptArgs a, const LaunchConfig &cfg,
                                         hipStream_t stream, Timing tm) {
  return variables_c<false>(t, a, nullptr, cfg, stream, tm);
}

hipError_t launch_sma_optimise_variables_clipped(const VarTables &t, VarOptArgs a, const ClipRecord *rec,
                                                 const LaunchConfig &cfg, hipStream_t stream, Timing tm) {
  if (!rec) return hipErrorInvalidValue;
  return variables_c<true>(t, a, rec, cfg, stream, tm);
}

hipError_t var_tables_upload(VarTables &t, const uint32_t *chunks, size_t nchunks, const uint32_t *bounds,
                             const float *mult, uint32_t nvars) {
  var_tables_free(t);
  if (!chunks || !bounds || nchunks == 0 || nvars == 0) return hipErrorInvalidValue;
  const size_t words = nchunks + ((size_t)nvars + 1) + nvars;
  std::vector<uint32_t> host(words);
  std::copy(chunks, chunks + nchunks, host.begin());
  std::copy(bounds, bounds + nvars + 1, host.begin() + (ptrdiff_t)nchunks);
  for (uint32_t v = 0; v < nvars; ++v) {
    const float m = mult ? mult[v] : 1.0f;
    std::memcpy(&host[nchunks + nvars + 1 + v], &m, 4);
  }
  uint32_t *dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), words * 4);
  if (e != hipSuccess) return e;
  e = hipMemcpy(dev, host.data(), words * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return e;
  }
  t.chunks = dev;
  t.bounds = dev + nchunks;
  t.mult = reinterpret_cast<float *>(dev + nchunks + nvars + 1);
  t.nvars = nvars;
  t.elements = bounds[nvars];
  return hipSuccess;
}

void var_tables_free(VarTables &t) {
  if (t.chunks) (void)hipFree(t.chunks);
  t = VarTables();
}

}  // namespace cbx
