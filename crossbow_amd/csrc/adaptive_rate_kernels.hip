// adaptive_rate_kernels.hip -- layer-wise adaptive rate scaling (LARS, and
// LARC as its capped form) in the replica optimiser step, for CDNA4 (gfx950).
// cbx_set_adaptive_rate, cbx_sma_plan_optimise_adaptive.  An extension: the
// reference has one rate per model and a fixed multiplier per variable
// (model.c:159-177), nothing that follows the norms.
//
// Every variable v steps with r_v = (rate * m_v) * t_v, where the trust ratio
// t_v = eta * |w_v| / (|g_v| + beta * |w_v| + eps) needs both norms of every
// variable before the first element steps, with no host round trip (the step
// is enqueued on a task stream).  Three launches on the same stream:
//
//   pass      read-only over w and g: one wave per piece of the host-built
//             piece table (stats_plan.h: a piece lies in one variable and one
//             4096-float tile).  An aligned piece by 16-byte loads, lane l the
//             float4s l, l + 64, ... of both buffers, every load of a group of
//             at most 8 + 8 issued before the first add; any other piece one
//             float per lane.  Each lane accumulates W and G in fp64 from the
//             first add ((double)x * (double)x is exact, so only the adds
//             round); a non-finite x adds nothing and counts.  The wave folds
//             its lanes with a fixed xor butterfly and lane 0 writes one
//             32-byte partial (W, G, K) to slab[piece].
//   trust     one wave per variable: lane l sums the variable's partials
//             l, l + 64, ... in piece order, the same butterfly, then lane 0
//             takes the ratio in fp64 in plain C++ (IEEE sqrt and divide),
//             rounds it to float once, and writes the variable's record and
//             its entry of the dense trust table.
//   step      sma_optimise_variables_kernel's three paths (uniform chunk, mixed
//             chunk, edge chunk one float at a time) over [0, n), with one more
//             table read: r = (rate * mult[v]) * trust[v].  In a uniform chunk
//             both reads go through a wave-uniform address, so the rate sits in
//             a scalar register.
//
// No float atomics and no order that depends on arrival: piece table, grid and
// both trees are fixed functions of the variable list alone (never of the CU
// count, a launch tunable or the stream), so context and seam return the same
// bits on the same data.
//
// Traffic: the pass reads 8 n bytes, the step moves 28 n (3 reads and 4 writes
// with momentum), so the path moves 36 n against the per-variable step's 28 n,
// plus two small launches (the trust kernel reads 32 bytes per piece).
//
// With several devices per context every local device carries its own tables
// and every replica its own scratch, as for clipping; that loop has not run on
// several devices.
#include <hip/hip_ext.h>

#include <vector>

#include "adaptive_internal.h"
#include "optimise_plan.h"
#include "stream_helpers.h"

namespace cbx {
namespace {

static_assert(sizeof(AdaptiveRecord) == 32, "cbx_adaptive_stats is 32 bytes without padding");
static_assert(sizeof(AdaptivePartial) == 32, "one 32-byte partial per piece");
static_assert(sizeof(StatsPiece) == 16, "the piece table is read as 16-byte entries");

template <int P>
__device__ __forceinline__ v4f ldg4(const float *base, uint32_t off) {
  const v4f *p = reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <int P>
__device__ __forceinline__ float ldg1(const float *base, uint32_t off) {
  const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

// clip_kernels.hip's rule, per buffer.
__device__ __forceinline__ void add_sq(double &q, uint32_t &nf, float x) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const double xd = fin ? (double)x : 0.0;
  q = fma(xd, xd, q);  // the product is exact: one rounding, the add's
  nf += fin ? 0u : 1u;
}

// float4 loads in flight per lane and buffer before the first add (a full
// 4096-float piece is two groups).
constexpr int kNormDepth = 8;

// One-wave workgroups; workgroup b walks pieces b, b + grid, ...
template <int P>
__global__ __launch_bounds__(64) void variable_norm_kernel(const float *__restrict__ w, const float *__restrict__ g,
                                                           const StatsPiece *__restrict__ pieces, uint32_t npieces,
                                                           AdaptivePartial *__restrict__ slab) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < npieces; p += gridDim.x) {
    const StatsPiece pc = pieces[p];  // wave-uniform
    double qw = 0.0, qg = 0.0;
    uint32_t nf = 0;
    if (pc.aligned) {
      const uint32_t lo4 = pc.lo >> 2, hi4 = pc.hi >> 2;
      for (uint32_t j = lo4; j < hi4; j += 64u * kNormDepth) {
        v4f x[kNormDepth], y[kNormDepth];
        // A float4 past the piece's end is not loaded: it adds +0 and counts
        // nothing, which leaves the non-negative sums' bits alone.
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)kNormDepth; ++u) {
          const uint32_t i4 = j + u * 64u + lane;
          x[u] = i4 < hi4 ? ldg4<P>(w, i4 * 16u) : v4f(0.0f);
          y[u] = i4 < hi4 ? ldg4<P>(g, i4 * 16u) : v4f(0.0f);
        }
        __builtin_amdgcn_sched_barrier(0);  // every load of the group in flight first (see the fused SMA kernel)
#pragma unroll
        for (int u = 0; u < kNormDepth; ++u) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            add_sq(qw, nf, x[u][k]);
            add_sq(qg, nf, y[u][k]);
          }
        }
      }
    } else {
      // At most 3 floats, or a segment without a whole float4: one per lane.
      for (uint32_t i = pc.lo + lane; i < pc.hi; i += 64u) {
        const float x = ldg1<P>(w, i * 4u), y = ldg1<P>(g, i * 4u);
        add_sq(qw, nf, x);
        add_sq(qg, nf, y);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // fixed xor butterfly: every lane ends with the same bits
      qw += __shfl_xor(qw, o);
      qg += __shfl_xor(qg, o);
      nf += __shfl_xor(nf, o);
    }
    if (lane == 0) {
      slab[p].w_sq = qw;
      slab[p].g_sq = qg;
      slab[p].nonfinite = nf;
      slab[p].reserved = 0;
    }
  }
}

// Partials in flight per lane of the trust kernel.
constexpr int kTrustDepth = 16;

__global__ __launch_bounds__(64) void variable_trust_kernel(const AdaptivePartial *__restrict__ slab,
                                                            const uint32_t *__restrict__ var_first,
                                                            const uint32_t *__restrict__ enable,
                                                            const AdaptiveParams prm, AdaptiveRecord *__restrict__ rec,
                                                            float *__restrict__ trust) {
  const uint32_t lane = threadIdx.x, v = blockIdx.x;
  const uint32_t lo = var_first[v], hi = var_first[v + 1];
  double W = 0.0, G = 0.0;
  unsigned long long K = 0;
  // Lane l adds partials lo + l, lo + l + 64, ... in that order; their loads go
  // out kTrustDepth at a time (gradient_norm_reduce_kernel).  A slot past the
  // end adds +0.
  for (uint32_t i0 = lo + lane; i0 < hi; i0 += 64u * kTrustDepth) {
    AdaptivePartial p[kTrustDepth];
#pragma unroll
    for (uint32_t u = 0; u < (uint32_t)kTrustDepth; ++u) {
      const uint32_t i = i0 + u * 64u;
      p[u] = i < hi ? slab[i] : AdaptivePartial{0.0, 0.0, 0ull, 0ull};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kTrustDepth; ++u) {
      W += p[u].w_sq;
      G += p[u].g_sq;
      K += p[u].nonfinite;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    W += __shfl_xor(W, o);
    G += __shfl_xor(G, o);
    K += __shfl_xor(K, o);
  }
  if (lane == 0) {
    float t = 1.0f;
    uint32_t flags = 0;
    if (enable[v] == 0u) {
      flags = kAdaptiveExcluded;
    } else if (lo == hi) {
      // a variable without floats: nothing to apply
    } else if (W == 0.0 || G == 0.0 || K > 0) {
      flags = kAdaptiveDegenerate;
    } else {
      const double nw = sqrt(W), ng = sqrt(G);
      const double den = (ng + (double)prm.weight_decay * nw) + (double)prm.epsilon;
      // W and G are finite (at most 2^30 squares of floats, far below the fp64
      // range) and positive here, so den > 0 and t is a number: +inf at most,
      // where the cast overflows, which mode 1 caps like any ratio over 1.
      t = (float)(((double)prm.trust * nw) / den);
      flags = kAdaptiveApplied;
      if (prm.mode == 1 && t > 1.0f) {
        t = 1.0f;
        flags |= kAdaptiveCapped;
      }
    }
    rec[v].w_sq = W;
    rec[v].g_sq = G;
    rec[v].nonfinite = K;
    rec[v].trust = t;
    rec[v].flags = flags;
    trust[v] = t;
  }
}

// sma_optimise_variables_kernel (variable_rate_kernels.hip) without its CLIP
// policy and its lower range bound, with one more table read.  That kernel's
// code object is pinned, so this is its text a second time: a fix to either
// belongs in both.
template <bool MOM, bool WD, int P, int U>
__global__ __launch_bounds__(512) void sma_optimise_adaptive_kernel(const VarOptArgs a,
                                                                          const uint32_t *__restrict__ chunks,
                                                                          const uint32_t *__restrict__ bounds,
                                                                          const float *__restrict__ mult,
                                                                          const float *__restrict__ trust) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t wave =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const v4f mu = a.momentum, wd = a.wd, one = 1.0f;
  for (uint32_t c = wave * U; c < a.chunk_hi; c += waves * U) {
    // wave-uniform: are all U chunks wholly inside [0, n)?
    if ((c + U) * kOptChunk <= a.hi) {
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
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t v0 = e[u] >> 1;
        if ((e[u] & 1u) == 0u) {
          r[u] = (a.rate * mult[v0]) * trust[v0];  // uniform: two scalar loads and a scalar register
        } else {
          const uint32_t f = (c + u) * kOptChunk + lane * 4u;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t v = variable_of(bounds, a.nvars, v0, f + k);
            r[u][k] = (a.rate * mult[v]) * trust[v];
          }
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
          if constexpr (WD) sto<P>(a.g, i, g[u]);
        }
      }
    } else {
      // The end of the buffer: the floats below n one by one.
      float *wp = reinterpret_cast<float *>(a.w), *gp = reinterpret_cast<float *>(a.g);
      float *lp = reinterpret_cast<float *>(a.last), *sp = reinterpret_cast<float *>(a.s);
      for (int u = 0; u < U; ++u) {
        if (c + u >= a.chunk_hi) break;
        const uint32_t en = chunks[c + u];
        const uint32_t f0 = (c + u) * kOptChunk + lane * 4u;
        for (int k = 0; k < 4; ++k) {
          const uint32_t f = f0 + k;
          if (f >= a.hi) continue;
          const uint32_t v = (en & 1u) ? variable_of(bounds, a.nvars, en >> 1, f) : (en >> 1);
          const float rv = (a.rate * mult[v]) * trust[v];
          const float wv = wp[f];
          float gv = gp[f];
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
            if constexpr (WD) gp[f] = gv;
          }
        }
      }
    }
  }
}

template <bool MOM, bool WD, int P>
hipError_t adaptive_p(const VarTables &vt, const VarOptArgs &a, const float *mult, const float *trust,
                      const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  const int reads = 2 + (MOM ? 1 : 0), writes = MOM ? 4 : (WD ? 3 : 2);
  const int64_t n4 = (int64_t)a.chunk_hi * 64;
  const dim3 g = grid_for(n4, cfg);
  const unsigned l = lds_for_occupancy(cfg, reads, writes, g.x);
  if (cfg.unroll == 2)
    hipExtLaunchKernelGGL((sma_optimise_adaptive_kernel<MOM, WD, P, 2>), g, dim3(cfg.block), l, stream, t.start,
                          t.stop, 0, a, vt.chunks, vt.bounds, mult, trust);
  else if (cfg.unroll == 1)
    hipExtLaunchKernelGGL((sma_optimise_adaptive_kernel<MOM, WD, P, 1>), g, dim3(cfg.block), l, stream, t.start,
                          t.stop, 0, a, vt.chunks, vt.bounds, mult, trust);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

template <int P>
hipError_t adaptive_c(const VarTables &t, const VarOptArgs &a, const float *mult, const float *trust,
                      const LaunchConfig &cfg, hipStream_t stream, Timing tm) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom)
    return wd ? adaptive_p<true, true, P>(t, a, mult, trust, cfg, stream, tm)
              : adaptive_p<true, false, P>(t, a, mult, trust, cfg, stream, tm);
  return wd ? adaptive_p<false, true, P>(t, a, mult, trust, cfg, stream, tm)
            : adaptive_p<false, false, P>(t, a, mult, trust, cfg, stream, tm);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_sma_optimise_adaptive(const VarTables &t, VarOptArgs a, const float *mult, const float *trust,
                                        const LaunchConfig &cfg, hipStream_t stream, Timing tm) {
  if (!t.chunks || !mult || !trust || t.elements == 0 || cfg.block < 64 || cfg.block % 64 != 0 || cfg.block > 512)
    return hipErrorInvalidValue;
  if (!a.w || !a.g || !a.s || (a.momentum > 0.0f && !a.last)) return hipErrorInvalidValue;
  a.nvars = t.nvars;
  a.lo = 0;
  a.hi = t.elements;
  a.chunk_lo = 0;
  a.chunk_hi = (a.hi + kOptChunk - 1) / kOptChunk;
  return cfg.policy == 1 ? adaptive_c<1>(t, a, mult, trust, cfg, stream, tm)
                         : adaptive_c<0>(t, a, mult, trust, cfg, stream, tm);
}

hipError_t launch_variable_norms(const float *w, const float *g, const AdaptiveTables &t, const AdaptiveScratch &s,
                                 const AdaptiveParams &p, int policy, hipStream_t stream, Timing pass,
                                 Timing reduce) {
  if (!w || !g || !t.dev || !s.dev || t.npieces == 0 || t.nvars == 0 || s.npieces != t.npieces ||
      s.nvars != t.nvars || !aligned16(w) || !aligned16(g))
    return hipErrorInvalidValue;
  const dim3 grid(stats_grid(t.npieces)), block(64);
  if (policy == 1)
    hipExtLaunchKernelGGL((variable_norm_kernel<1>), grid, block, 0, stream, pass.start, pass.stop, 0, w, g,
                          t.pieces(), t.npieces, s.slab());
  else
    hipExtLaunchKernelGGL((variable_norm_kernel<0>), grid, block, 0, stream, pass.start, pass.stop, 0, w, g,
                          t.pieces(), t.npieces, s.slab());
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipExtLaunchKernelGGL(variable_trust_kernel, dim3(t.nvars), block, 0, stream, reduce.start, reduce.stop, 0,
                        (const AdaptivePartial *)s.slab(), (const uint32_t *)t.var_first(),
                        (const uint32_t *)t.enable(), p, s.records(), s.trust());
  return hipGetLastError();
}

hipError_t adaptive_tables_upload(AdaptiveTables &t, const StatsPlan &plan, const unsigned char *enable) {
  adaptive_tables_free(t);
  const size_t np = plan.pieces.size();
  if (np == 0 || plan.var_first.size() < 2 || plan.var_first.back() != np) return hipErrorInvalidValue;
  const size_t V = plan.var_first.size() - 1;
  // pieces, var_first, enable, then V floats of 1: the multipliers of a step
  // without cbx_set_variable_learning_rates
  const size_t words = np * 4 + (V + 1) + V + V;
  std::vector<uint32_t> host(words);
  std::memcpy(host.data(), plan.pieces.data(), np * sizeof(StatsPiece));
  std::copy(plan.var_first.begin(), plan.var_first.end(), host.begin() + (ptrdiff_t)(np * 4));
  const float one = 1.0f;
  for (size_t v = 0; v < V; ++v) {
    host[np * 4 + V + 1 + v] = (!enable || enable[v]) ? 1u : 0u;
    std::memcpy(&host[np * 4 + V + 1 + V + v], &one, 4);
  }
  char *dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), words * 4);
  if (e != hipSuccess) return e;
  e = hipMemcpy(dev, host.data(), words * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return e;
  }
  t.dev = dev;
  t.npieces = (uint32_t)np;
  t.nvars = (uint32_t)V;
  t.elements = (uint32_t)plan.elements;
  return hipSuccess;
}

hipError_t adaptive_tables_set_enable(AdaptiveTables &t, uint32_t v, bool on) {
  if (!t.dev || v >= t.nvars) return hipErrorInvalidValue;
  const uint32_t word = on ? 1u : 0u;
  return hipMemcpy(t.enable() + v, &word, 4, hipMemcpyHostToDevice);
}

void adaptive_tables_free(AdaptiveTables &t) {
  if (t.dev) (void)hipFree(t.dev);
  t = AdaptiveTables();
}

hipError_t adaptive_scratch_alloc(AdaptiveScratch &s, const AdaptiveTables &t) {
  adaptive_scratch_free(s);
  if (!t.dev) return hipErrorInvalidValue;
  AdaptiveScratch n;
  n.npieces = t.npieces;
  n.nvars = t.nvars;
  const size_t bytes =
      (size_t)n.nvars * sizeof(AdaptiveRecord) + n.trust_bytes() + (size_t)n.npieces * sizeof(AdaptivePartial);
  char *dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), bytes);
  if (e != hipSuccess) return e;
  // As clip_scratch_alloc: hipMemset of device memory may return before it has
  // run, and a caller's non-blocking stream does not wait for the null stream.
  e = hipMemset(dev, 0, bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return e;
  }
  n.dev = dev;
  s = n;
  return hipSuccess;
}

void adaptive_scratch_free(AdaptiveScratch &s) {
  if (s.dev) (void)hipFree(s.dev);
  s = AdaptiveScratch();
}

}  // namespace cbx
