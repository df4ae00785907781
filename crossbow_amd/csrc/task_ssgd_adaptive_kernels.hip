// task_ssgd_adaptive_kernels.hip -- the replicas' pending task steps with
// layer-wise adaptive rates (LARS, and LARC as its capped form) fused into the
// one-GPU synchronous-SGD barrier (cbx_step_and_synchronise_ssgd_adaptive,
// cbx_ssgd_plan_step_and_optimise_adaptive), for CDNA4 (gfx950).  An extension:
// the reference has one rate per model (synch/synchronoussgd.c:13-106).
//
// Under update model WORKER the trust ratio belongs to the base model z and to
// the gradient summed over the replicas, so neither norm exists until every
// stepping replica's gradient has been accumulated: the ratio cannot ride the
// one streaming pass of task_ssgd_kernel.  Three launches on one stream:
//
//   pass    one-wave workgroups over the statistics piece table (stats_plan.h:
//           a piece lies in one variable and one 4096-float tile), workgroup b
//           the pieces b, b + grid, ...  An aligned piece by 16-byte loads, lane
//           l the float4s l, l + 64, ... in groups of kPassDepth (one in the
//           chunked walk); any other
//           piece one float per lane.  Per group a lane holds acc, z and Gs and
//           walks the stepping replicas in register-resident chunks of kChunk,
//           every load of a chunk issued before its first arithmetic.  It
//           writes acc back (and g_i with weight decay and kept outputs) and
//           folds z^2 and gbar^2 into per-lane fp64 sums ((double)x * (double)x
//           is exact, only the adds round; a non-finite float adds nothing and
//           counts), which the fixed xor butterfly folds into one 32-byte
//           partial per piece.  No LDS, no atomics.
//   trust   one wave per variable: the partials in piece order, the same
//           butterfly, then lane 0 takes the ratio in fp64, rounds it to float
//           once and writes the variable's record and the dense trust table.
//   apply   task_ssgd_kernel's streaming shape (float4 per lane behind an SGPR
//           base, unroll 1 or 2, acc, z and last loaded before the first
//           arithmetic, a runtime loop of broadcast stores) with one more read:
//           the chunk's t_v through the host-built chunk table
//           (optimise_plan.h).  A uniform chunk takes it by one wave-uniform
//           load into a scalar register, a chunk with a variable boundary
//           gathers per lane (variable_of).  The pad of the context's buffers
//           is a pseudo-variable past the trust table and steps at 1.
//
// Per element of variable v (one fp32 operation per line; -ffp-contract=off):
//   acc = the base gradient as found
//   Gs  = +0
//   per stepping replica i, list order (ascending id):
//     Gs  = Gs + g_i                                     raw, before weight decay
//     gv  = g_i ; gv = fma(wd, w_i, gv) ; g_i = gv       task_ssgd_kernel's sequence
//     acc = fma(rate_i, gv, acc)
//   gbar = ratio * Gs
//   Z_v = sum z^2, G_v = sum gbar^2, K_v = the non-finite floats of both
//   t_v = variable_trust_kernel's rule on (Z_v, G_v, K_v)
//   a = t_v * acc
//   D = ratio * a ; D = fma(mu, last, D) ; last = D ; z = fma(1, D, z) ; base gradient = +0
//   w_j = z for every receiving replica j
// The norm is over the mean of the stepping replicas' raw gradients: what the
// base gradient held on entry joins the update and not the norm.  With t_v == 1
// everywhere the buffers are launch_task_ssgd's bit for bit.
//
// Traffic without weight decay: (8R + 36) n bytes against the plain fused
// call's (8R + 24) n: acc written and read again, z read twice.  The pass loads
// and stores acc and z plainly whatever the policy, since the apply kernel reads
// both right behind it; the policy governs the replicas' g and w.
//
// Piece table, grids of the first two launches and both trees are fixed
// functions of the variable list alone, so context and seam return the same
// records on the same data.
//
// This file is a shared object of its own (libcrossbow_sma_ssgd_adaptive.so):
// the device code of the other objects is not touched by it.
#include <hip/hip_ext.h>

#include "optimise_plan.h"
#include "stream_helpers.h"
#include "task_ssgd_adaptive_internal.h"

namespace cbx {

namespace {

static_assert(sizeof(AdaptiveRecord) == 32, "cbx_adaptive_stats is 32 bytes without padding");
static_assert(sizeof(AdaptivePartial) == 32, "one 32-byte partial per piece");
static_assert(sizeof(StatsPiece) == 16, "the piece table is read as 16-byte entries");

template <int P>
__device__ __forceinline__ float ldf(const void *base, uint32_t off) {
  const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <int P>
__device__ __forceinline__ void stf(void *base, uint32_t off, float v) {
  float *p = reinterpret_cast<float *>(reinterpret_cast<char *>(base) + off);
  if constexpr (P == 1) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// adaptive_rate_kernels.hip's rule (clip_kernels.hip's), per buffer.
__device__ __forceinline__ void add_sq(double &q, uint32_t &nf, float x) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const double xd = fin ? (double)x : 0.0;
  q = fma(xd, xd, q);  // the product is exact: one rounding, the add's
  nf += fin ? 0u : 1u;
}

// float4s per lane in one group of the pass.  Two, the footprint of
// task_ssgd_kernel at unroll 2: with weight decay a chunk of kChunk replicas
// is 2 x 8 x 2 float4s = 128 VGPRs in flight beside acc, z and Gs (24) and the
// fp64 sums: 169 VGPRs at most, two waves per SIMD; a full tile is 8 groups.
// The chunked walk (S == -1), whose guarded loads keep more alive, takes one:
// at two its weight-decay forms fill all 256 VGPRs and move 32 more through
// AGPRs, at one they hold 154 and none.  No instantiation uses scratch.
// Nothing has measured which depth is fastest.
constexpr int kPassDepth = 2;
constexpr int kPassDepthChunked = 1;

// One piece's floats [lo, hi) one per lane: at most 3 floats, or a segment
// without a whole float4.  The fp32 sequence per element and the chunked walk
// are those of the float4 path.
template <int S, bool WD, bool KEEP, int P>
__device__ __forceinline__ void pass_scalar_piece(const TaskSsgdArgs &a, uint32_t lo, uint32_t hi, double &qz,
                                                  double &qg, uint32_t &nf) {
  constexpr int SS = (S > 0) ? S : kChunk;
  const int nstep = (S > 0) ? S : a.nstep;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 64u) {
    const uint32_t off = i * 4u;
    float acc = ldf<0>(a.acc, off);
    const float z = ldf<0>(a.z, off);
    float gs = 0.0f;
#pragma nounroll
    for (int c = 0; c < nstep; c += SS) {
      float y[SS];
      [[maybe_unused]] float x[SS];
#pragma unroll
      for (int r = 0; r < SS; ++r) {
        if (S < 0 && c + r >= nstep) continue;
        y[r] = ldf<P>(a.g[c + r], off);
        if constexpr (WD) x[r] = ldf<P>(a.sw[c + r], off);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < SS; ++r) {
        if (S < 0 && c + r >= nstep) continue;
        float gv = y[r];
        gs = gs + gv;
        if constexpr (WD) {
          gv = fmaf(a.wd, x[r], gv);
          if constexpr (KEEP) stf<P>(a.g[c + r], off, gv);
        }
        acc = fmaf(a.rate[c + r], gv, acc);
      }
      if constexpr (S > 0) break;
    }
    stf<0>(a.acc, off, acc);
    add_sq(qz, nf, z);
    add_sq(qg, nf, a.ratio * gs);
  }
}

// S > 0: that many stepping replicas, fully unrolled (S <= kChunk); S == -1
// takes a.nstep and walks them in register-resident chunks of kChunk.  WD: the
// stepping replicas' weight decay (their w is read).  KEEP (with WD only): g_i
// is written as the plain step writes it.  P: the loads of g and w and the
// stores of g (1 nontemporal).  One-wave workgroups; workgroup b walks pieces
// b, b + grid, ... as variable_norm_kernel does.  Only floats inside a piece
// are read or written: the table ends at the model's last float.
template <int S, bool WD, bool KEEP, int P>
__global__ __launch_bounds__(64) void ssgd_accumulate_norm_kernel(const TaskSsgdArgs a,
                                                                  const StatsPiece *__restrict__ pieces,
                                                                  uint32_t npieces,
                                                                  AdaptivePartial *__restrict__ slab) {
  static_assert(S == -1 || (S >= 1 && S <= kChunk), "the unrolled forms hold one chunk");
  static_assert(WD || !KEEP, "without weight decay the step writes no g: one form");
  constexpr int SS = (S > 0) ? S : kChunk;
  constexpr int D = (S > 0) ? kPassDepth : kPassDepthChunked;
  const int nstep = (S > 0) ? S : a.nstep;
  const uint32_t lane = threadIdx.x;
  const v4f ratio = a.ratio;
  [[maybe_unused]] const v4f wd = a.wd;
  for (uint32_t p = blockIdx.x; p < npieces; p += gridDim.x) {
    const StatsPiece pc = pieces[p];  // wave-uniform
    double qz = 0.0, qg = 0.0;
    uint32_t nf = 0;
    if (pc.aligned) {
      const uint32_t lo4 = pc.lo >> 2, hi4 = pc.hi >> 2;
      for (uint32_t j = lo4; j < hi4; j += 64u * D) {
        v4f acc[D], zv[D], gs[D];
        uint32_t off[D];
        bool in[D];
        // A float4 past the piece's end is neither loaded nor stored: it adds
        // +0 and counts nothing, which leaves the non-negative sums' bits alone.
#pragma unroll
        for (int u = 0; u < D; ++u) {
          const uint32_t i4 = j + (uint32_t)u * 64u + lane;
          in[u] = i4 < hi4;
          off[u] = i4 * 16u;
          acc[u] = in[u] ? ldo<0>(a.acc, off[u]) : v4f(0.0f);
          zv[u] = in[u] ? ldo<0>(a.z, off[u]) : v4f(0.0f);
          gs[u] = 0.0f;
        }
        // one chunk's registers at a time
#pragma nounroll
        for (int c = 0; c < nstep; c += SS) {
          v4f y[D][SS];
          [[maybe_unused]] v4f x[D][SS];
#pragma unroll
          for (int r = 0; r < SS; ++r) {
            if (S < 0 && c + r >= nstep) continue;  // a guard, not a break: the unrolled body keeps its registers
#pragma unroll
            for (int u = 0; u < D; ++u) {
              y[u][r] = in[u] ? ldo<P>(a.g[c + r], off[u]) : v4f(0.0f);
              if constexpr (WD) x[u][r] = in[u] ? ldo<P>(a.sw[c + r], off[u]) : v4f(0.0f);
            }
          }
          // every load of the chunk, and acc and z, in flight before the first use
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int r = 0; r < SS; ++r) {
            if (S < 0 && c + r >= nstep) continue;
            const v4f rate = a.rate[c + r];
#pragma unroll
            for (int u = 0; u < D; ++u) {
              v4f gv = y[u][r];
              gs[u] = gs[u] + gv;
              if constexpr (WD) {
                gv = vfma(wd, x[u][r], gv);
                if constexpr (KEEP) {
                  if (in[u]) sto<P>(a.g[c + r], off[u], gv);
                }
              }
              acc[u] = vfma(rate, gv, acc[u]);
            }
          }
          if constexpr (S > 0) break;
        }
#pragma unroll
        for (int u = 0; u < D; ++u) {
          if (in[u]) sto<0>(a.acc, off[u], acc[u]);
          const v4f gbar = ratio * gs[u];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            add_sq(qz, nf, zv[u][k]);
            add_sq(qg, nf, gbar[k]);
          }
        }
      }
    } else {
      pass_scalar_piece<S, WD, KEEP, P>(a, pc.lo, pc.hi, qz, qg, nf);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // fixed xor butterfly: every lane ends with the same bits
      qz += __shfl_xor(qz, o);
      qg += __shfl_xor(qg, o);
      nf += __shfl_xor(nf, o);
    }
    if (lane == 0) {
      slab[p].w_sq = qz;
      slab[p].g_sq = qg;
      slab[p].nonfinite = nf;
      slab[p].reserved = 0;
    }
  }
}

// Partials in flight per lane of the trust kernel.
constexpr int kTrustDepth = 16;

// variable_trust_kernel (adaptive_rate_kernels.hip) written once more: the
// original sits in an anonymous namespace of an object whose code is pinned.  A
// fix to either belongs in both.
__global__ __launch_bounds__(64) void ssgd_variable_trust_kernel(const AdaptivePartial *__restrict__ slab,
                                                                 const uint32_t *__restrict__ var_first,
                                                                 const uint32_t *__restrict__ enable,
                                                                 const AdaptiveParams prm,
                                                                 AdaptiveRecord *__restrict__ rec,
                                                                 float *__restrict__ trust) {
  const uint32_t lane = threadIdx.x, v = blockIdx.x;
  const uint32_t lo = var_first[v], hi = var_first[v + 1];
  double W = 0.0, G = 0.0;
  unsigned long long K = 0;
  // Lane l adds partials lo + l, lo + l + 64, ... in that order; their loads go
  // out kTrustDepth at a time.  A slot past the end adds +0.
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
      // W and G are finite and positive here, so den > 0 and t is a number:
      // +inf at most, where the cast overflows, which mode 1 caps like any
      // ratio over 1.
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

// The tables the apply kernel reads beside TaskSsgdArgs.
struct TrustTables {
  const uint32_t *chunks;  // one entry per 256-float chunk of the swept length: (variable << 1) | mixed
  const uint32_t *bounds;  // nvars + 1 running offsets, floats
  const float *trust;      // ntrust ratios, the trust kernel's
  uint32_t nvars;          // of the chunk table (the context's: the pad's pseudo-variable included)
  uint32_t ntrust;         // a variable at or past it steps at 1
};

__device__ __forceinline__ float trust_of(const TrustTables &tt, uint32_t v) {
  return v < tt.ntrust ? tt.trust[v] : 1.0f;
}

// Buffers the caller owns hold exactly n floats: their last elements
// [a.tail_lo, a.tail_hi) go to the first a.tail_blocks workgroups of the same
// launch, one float per lane (task_ssgd_tail_elem).  Nothing at or past
// a.tail_hi is read, nothing outside the range is written.
template <bool MOM>
__device__ __forceinline__ void apply_tail_elem(const TaskSsgdArgs &a, const TrustTables &tt) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  float *accp = reinterpret_cast<float *>(a.acc);
  const float acc = accp[i];
  const float z0 = z[i];
  [[maybe_unused]] float l0 = 0.0f;
  if constexpr (MOM) l0 = reinterpret_cast<const float *>(a.last)[i];
  const uint32_t f = (uint32_t)i, en = tt.chunks[f / kOptChunk];
  const uint32_t v = (en & 1u) ? variable_of(tt.bounds, tt.nvars, en >> 1, f) : (en >> 1);
  const float av = trust_of(tt, v) * acc;
  float D = a.ratio * av;  // synchronoussgd.c:55-62
  if constexpr (MOM) {
    D = fmaf(a.momentum, l0, D);  // :64-76
    reinterpret_cast<float *>(a.last)[i] = D;
  }
  const float zv = fmaf(1.0f, D, z0);  // :79-84
  z[i] = zv;
  accp[i] = 0.0f;  // :103
  for (int r = 0; r < a.nrecv; ++r) reinterpret_cast<float *>(a.w[r])[i] = zv;  // common.c:198-220
}

// task_ssgd_kernel's apply and broadcast (its S == 0 form) on a = t_v * acc.
// MOM: the base model's momentum.  TAIL: the launch's first a.tail_blocks
// workgroups do the caller's last elements.  A wave's trip is U whole chunks of
// the chunk table (64 float4s each), so a chunk's entry and, in a uniform
// chunk, its ratio are wave-uniform: scalar loads and a scalar register.
template <bool MOM, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void ssgd_apply_trust_kernel(const TaskSsgdArgs a, const TrustTables tt) {
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      apply_tail_elem<MOM>(a, tt);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const uint32_t lane = threadIdx.x & 63u;
  const v4f ratio = a.ratio, one = 1.0f, zero = 0.0f;
  [[maybe_unused]] const v4f mu = a.momentum;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 6));  // the wave's first chunk
    v4f acc[U], zv[U], t[U];
    [[maybe_unused]] v4f l[U];
    uint32_t e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = tt.chunks[c0 + (uint32_t)u];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      acc[u] = ldo<P>(a.acc, i);
      zv[u] = ldo<P>(a.z, i);
      if constexpr (MOM) l[u] = ldo<P>(a.last, i);
    }
    // acc, z and last in flight before the first use
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t v0 = e[u] >> 1;
      if ((e[u] & 1u) == 0u) {
        t[u] = trust_of(tt, v0);  // uniform: one scalar load
      } else {
        const uint32_t f = (c0 + (uint32_t)u) * kOptChunk + lane * 4u;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[u][k] = trust_of(tt, variable_of(tt.bounds, tt.nvars, v0, f + k));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      const v4f av = t[u] * acc[u];
      v4f D = ratio * av;
      if constexpr (MOM) {
        D = vfma(mu, l[u], D);
        sto<P>(a.last, i, D);
      }
      zv[u] = vfma(one, D, zv[u]);
      sto<P>(a.z, i, zv[u]);
      sto<P>(a.acc, i, zero);
    }
    for (int r = 0; r < a.nrecv; ++r) {
#pragma unroll
      for (int u = 0; u < U; ++u) sto<P>(a.w[r], (base + u * 64u) * 16u, zv[u]);
    }
  }
}

// ---- the pass's ladder -----------------------------------------------------

template <int S, bool WD, bool KEEP, int P>
hipError_t pass_go(const TaskSsgdArgs &a, const AdaptiveTables &t, const AdaptiveScratch &s, hipStream_t st,
                   hipEvent_t start) {
  hipExtLaunchKernelGGL((ssgd_accumulate_norm_kernel<S, WD, KEEP, P>), dim3(stats_grid(t.npieces)), dim3(64), 0, st,
                        start, nullptr, 0, a, t.pieces(), t.npieces, s.slab());
  return hipGetLastError();
}

// The stepping replicas unrolled up to one chunk, chunked beyond it.
template <bool WD, bool KEEP, int P>
hipError_t pass_form(const TaskSsgdArgs &a, const AdaptiveTables &t, const AdaptiveScratch &s, hipStream_t st,
                     hipEvent_t start) {
  switch (a.nstep) {
    case 1: return pass_go<1, WD, KEEP, P>(a, t, s, st, start);
    case 2: return pass_go<2, WD, KEEP, P>(a, t, s, st, start);
    case 3: return pass_go<3, WD, KEEP, P>(a, t, s, st, start);
    case 4: return pass_go<4, WD, KEEP, P>(a, t, s, st, start);
    case 5: return pass_go<5, WD, KEEP, P>(a, t, s, st, start);
    case 6: return pass_go<6, WD, KEEP, P>(a, t, s, st, start);
    case 7: return pass_go<7, WD, KEEP, P>(a, t, s, st, start);
    case 8: return pass_go<8, WD, KEEP, P>(a, t, s, st, start);
    default: return pass_go<-1, WD, KEEP, P>(a, t, s, st, start);
  }
}

template <int P>
hipError_t pass_conf(const TaskSsgdArgs &a, bool keep, const AdaptiveTables &t, const AdaptiveScratch &s,
                     hipStream_t st, hipEvent_t start) {
  // without weight decay the step writes no g: kept and discarded are one kernel
  if (!(a.wd > 0.0f)) return pass_form<false, false, P>(a, t, s, st, start);
  return keep ? pass_form<true, true, P>(a, t, s, st, start) : pass_form<true, false, P>(a, t, s, st, start);
}

// ---- the apply kernel's ladder ---------------------------------------------

// Only what a door reaches is compiled: the tail rides the nontemporal policy
// at unroll 1, the seam's shape; without one, unroll 1 or 2 at either policy.
template <bool MOM, int P, bool TAIL, int U>
hipError_t apply_go(const TaskSsgdArgs &a, const TrustTables &tt, dim3 g, int block, unsigned lds, hipStream_t s,
                    hipEvent_t stop) {
  if constexpr (TAIL ? (P == 1 && U == 1) : true) {
    hipExtLaunchKernelGGL((ssgd_apply_trust_kernel<MOM, P, TAIL, U>), g, dim3(block), lds, s, nullptr, stop, 0, a, tt);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <bool MOM, int P>
hipError_t apply_u(const TaskSsgdArgs &a, const TrustTables &tt, const LaunchConfig &cfg0, hipStream_t s,
                   hipEvent_t stop) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's trip is whole chunks (ts_u, task_ssgd_kernels.hip): no bounds
  // check sits in the kernel's loop, and no chunk past the table is looked up.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane: the base model reads acc, z (, last) and writes
  // them, a receiving replica is one write.  The cap is ts_u's.
  const int m = MOM ? 1 : 0;
  const int reads = 2 + m, writes = a.nrecv + 2 + m;
  LaunchConfig cap = cfg;
  if (cfg.waves_per_cu < 0 && (int64_t)g.x * ((cfg.block + 63) / 64) >= 16ll * cfg.num_cus) {
    const int streams = reads + writes;
    const int w = (kAveragingStreamsPerCU + streams / 2) / streams;
    cap.waves_per_cu = w < 2 ? 2 : (w > 12 ? 12 : w);
  }
  const unsigned lds = lds_for_occupancy(cap, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    TaskSsgdArgs b = a;
    b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
    g.x += (unsigned)b.tail_blocks;
    if (cfg.unroll == 1) return apply_go<MOM, P, true, 1>(b, tt, g, cfg.block, lds, s, stop);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return apply_go<MOM, P, false, 2>(a, tt, g, cfg.block, lds, s, stop);
  if (cfg.unroll == 1) return apply_go<MOM, P, false, 1>(a, tt, g, cfg.block, lds, s, stop);
  return hipErrorInvalidValue;
}

// What apply_u and apply_go refuse, asked before the pass has changed anything.
bool apply_shape_compiled(const TaskSsgdArgs &a, const LaunchConfig &cfg0) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || a.n4 < 0 || (a.n4 == 0 && !tail)) return false;
  if (cfg.unroll != 1 && cfg.unroll != 2) return false;
  if (a.n4 % (64ll * cfg.unroll) != 0) return false;
  return !tail || (cfg.unroll == 1 && cfg.policy == 1);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_task_ssgd_adaptive(const TaskSsgdArgs &a, const AdaptiveTables &t, const AdaptiveScratch &s,
                                     const AdaptiveParams &p, const VarTables &vt, bool keep_task_outputs,
                                     const LaunchConfig &cfg, hipStream_t stream, Timing tm) {
  if (a.nstep < 1 || a.nstep > kMaxReplicas || a.nrecv < 0 || a.nrecv > kMaxReplicas) return hipErrorInvalidValue;
  const bool mom = a.momentum > 0.0f;  // synchronoussgd.c:64
  if (!a.z || !a.acc || (mom && !a.last)) return hipErrorInvalidValue;
  if (!t.dev || !s.dev || t.npieces == 0 || t.nvars == 0 || s.npieces != t.npieces || s.nvars != t.nvars)
    return hipErrorInvalidValue;
  if (!vt.chunks || !vt.bounds || vt.nvars < t.nvars) return hipErrorInvalidValue;
  // The pieces end at the model's last float, the sweep of the apply kernel at
  // the chunk table's: the first inside the second.
  const bool tail = a.tail_hi > a.tail_lo;
  const int64_t swept = tail ? a.tail_hi : a.n4 * 4;
  if (tail && a.tail_lo != a.n4 * 4) return hipErrorInvalidValue;
  if ((int64_t)t.elements > swept || swept > (int64_t)vt.elements) return hipErrorInvalidValue;
  if (!aligned16(a.z) || !aligned16(a.acc) || !apply_shape_compiled(a, cfg)) return hipErrorInvalidValue;
  for (int k = 0; k < a.nstep; ++k)
    if (!a.g[k] || !aligned16(a.g[k]) || (a.wd > 0.0f && (!a.sw[k] || !aligned16(a.sw[k])))) return hipErrorInvalidValue;

  hipError_t e = cfg.policy == 1 ? pass_conf<1>(a, keep_task_outputs, t, s, stream, tm.start)
                                 : pass_conf<0>(a, keep_task_outputs, t, s, stream, tm.start);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ssgd_variable_trust_kernel, dim3(t.nvars), dim3(64), 0, stream,
                     (const AdaptivePartial *)s.slab(), (const uint32_t *)t.var_first(), (const uint32_t *)t.enable(),
                     p, s.records(), s.trust());
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const TrustTables tt = {vt.chunks, vt.bounds, s.trust(), vt.nvars, s.nvars};
  if (cfg.policy == 1)
    return mom ? apply_u<true, 1>(a, tt, cfg, stream, tm.stop) : apply_u<false, 1>(a, tt, cfg, stream, tm.stop);
  return mom ? apply_u<true, 0>(a, tt, cfg, stream, tm.stop) : apply_u<false, 0>(a, tt, cfg, stream, tm.stop);
}

}  // namespace cbx
