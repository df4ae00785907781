// task_barrier_variables_kernels.hip -- the replicas' pending task steps with a
// learning rate per variable, fused into the one-GPU SMA barrier
// (cbx_step_and_synchronise_variables, cbx_sma_plan_step_and_optimise_variables),
// for CDNA4 (gfx950).
//
// task_barrier_kernel (task_barrier_kernels.hip) plus the rate lookup of
// sma_optimise_variables_kernel (variable_rate_kernels.hip): the same single
// streaming pass, float4s behind an SGPR base and a 32-bit offset, every load
// of a replica chunk issued before the first arithmetic, acc in registers, no
// LDS, R <= kChunk unrolled and larger R in chunks of kChunk, the mixed form
// chosen by pointer.  Per element of variable v and per stepping replica i
//   r_iv = rate_i * mult[v]                        one fp32 multiply (model.c:159-177)
// and then task_barrier_kernel's sequence with r_iv in place of rate_i
// (built with -ffp-contract=off):
//   g = fma(wd, w, g)                              sma.cu:24-31 (wd > 0)
//   s = w                                          :71 / :87
//   g = r_iv * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)     :52-74
//   or, without momentum, w' = fma(r_iv, g, w)     :90
// for a replica that only joins the barrier s = s_i, w' = w_i; then for both
//   d = fma(-1, z, s) ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)    sma.c:79-107
// and D = acc ; D = fma(0.9, last, D), last = D ; z = fma(1, D, z)             sma.c:148-174
// With a copy request (Phase D, sma.c:185-227) every w_i becomes the new z.
//
// The lookup is per wave: a wave's 64 float4s are one 256-float chunk of the
// host-built table (optimise_plan.h), at unroll 2 two chunks.  The tables are
// kernel parameters of their own, `const __restrict__`, so the entry and the
// multiplier of a uniform chunk arrive through scalar loads; the entry's load
// is issued with the trip's first float4 loads and used after the last.  In a
// chunk with a boundary inside, each lane finds the variable of each of its
// four floats in the sorted boundary array.  r_iv is a vector multiply of the
// (scalar) rate_i by the lane's four multipliers on both paths: the same bits
// as a scalar multiply, and no branch in the replica loop.
//
// The context's buffers are padded to kPadFloat4: its table is built over the
// padded length, the pad floats a last pseudo-variable of multiplier 1
// (build_padded_optimise_plan), so the kernel knows nothing of the pad and a
// zero pad stays zero.  Buffers the caller owns take the TAIL instantiations:
// the last elements one per lane, each float's variable from the same tables.
//
// This file is a shared object of its own (libcrossbow_sma_variables.so): the
// device code of libcrossbow_sma.so is not touched by it.
#include <hip/hip_ext.h>

#include "optimise_plan.h"
#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {
namespace {

// The variable of float f, at or after v0 (the variable of the chunk's first
// float): the last v with bounds[v] <= f.  bounds[nvars] = elements > f.
// (variable_rate_kernels.hip's, which this object does not link.)
__device__ __forceinline__ uint32_t variable_of(const uint32_t *__restrict__ bounds, uint32_t nvars, uint32_t v0,
                                                uint32_t f) {
  uint32_t lo = v0, hi = nvars;
  while (hi - lo > 1u) {
    const uint32_t m = (lo + hi) >> 1;
    if (bounds[m] <= f) lo = m;
    else hi = m;
  }
  return lo;
}

// task_barrier_tail_elem with the float's own multiplier: elements
// [a.tail_lo, a.tail_hi), one per lane.  Nothing at or past a.tail_hi is read
// (the chunk entry of float i < elements exists), nothing outside is written.
template <bool MOM, bool BMOM, bool WD, bool KEEP>
__device__ __forceinline__ void task_barrier_variables_tail_elem(const TaskBarrierArgs &a,
                                                                 const uint32_t *__restrict__ chunks,
                                                                 const uint32_t *__restrict__ bounds,
                                                                 const float *__restrict__ mult, uint32_t nvars) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  const uint32_t en = chunks[(uint32_t)i / kOptChunk];
  const float m = mult[(en & 1u) ? variable_of(bounds, nvars, en >> 1, (uint32_t)i) : (en >> 1)];
  float *z = reinterpret_cast<float *>(a.z);
  float z0 = z[i];
  float l0 = 0.0f;
  if constexpr (BMOM) l0 = reinterpret_cast<const float *>(a.blast)[i];
  float acc = 0.0f;  // sma.c:66
  for (int c = 0; c < a.nrep; c += kChunk) {
    // a stepping replica: x = w, y = g, l = last_i; one that only joins: x = s, y = w
    float x[kChunk], y[kChunk];
    [[maybe_unused]] float l[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool step = ((a.step_mask >> (c + r)) & 1ull) != 0;
        x[r] = reinterpret_cast<const float *>(step ? a.w[c + r] : a.s[c + r])[i];
        y[r] = reinterpret_cast<const float *>(step ? a.g[c + r] : a.w[c + r])[i];
        if constexpr (MOM) {
          if (step) l[r] = reinterpret_cast<const float *>(a.last[c + r])[i];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool step = ((a.step_mask >> (c + r)) & 1ull) != 0;
        const float sv = x[r];
        float wn;
        if (step) {
          const float rate = a.rate[c + r] * m;  // model.c:159-177
          float gv = y[r];
          if constexpr (WD) gv = fmaf(a.wd, sv, gv);  // sma.cu:24-31
          if constexpr (MOM) {
            gv = rate * gv;                    // :52-56
            gv = fmaf(a.momentum, l[r], gv);   // :59-64
            reinterpret_cast<float *>(a.last[c + r])[i] = gv;  // :68
            wn = fmaf(1.0f, gv, sv);           // :74
          } else {
            wn = fmaf(rate, gv, sv);  // :90
          }
          if constexpr (KEEP) {
            reinterpret_cast<float *>(a.s[c + r])[i] = sv;  // :71 / :87
            if constexpr (MOM || WD) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
          }
        } else {
          wn = y[r];
        }
        const float d = fmaf(-1.0f, z0, sv);                             // sma.c:79-90
        acc = fmaf(a.alpha, d, acc);                                     // :102-107
        reinterpret_cast<float *>(a.w[c + r])[i] = fmaf(-a.alpha, d, wn);  // :93-99
      }
    }
  }
  float D = acc;
  if constexpr (BMOM) {
    D = fmaf(kBaseMomentum, l0, D);  // sma.c:155-164
    reinterpret_cast<float *>(a.blast)[i] = D;
  }
  z0 = fmaf(1.0f, D, z0);  // sma.c:169-174
  z[i] = z0;
  if (a.copy != 0)
    for (int r = 0; r < a.nrep; ++r) reinterpret_cast<float *>(a.w[r])[i] = z0;  // sma.c:185-227
}

// The template parameters are task_barrier_kernel's.  chunks / bounds / mult:
// the tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi).
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_variables_kernel(const TaskBarrierArgs a,
                                                                     const uint32_t *__restrict__ chunks,
                                                                     const uint32_t *__restrict__ bounds,
                                                                     const float *__restrict__ mult,
                                                                     const uint32_t nvars) {
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_barrier_variables_tail_elem<MOM, BMOM, WD, KEEP>(a, chunks, bounds, mult, nvars);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const uint32_t lane = threadIdx.x & 63u;
  const v4f al = a.alpha, nal = -a.alpha, mb = kBaseMomentum, one = 1.0f, mone = -1.0f;
  const v4f mu = a.momentum, wd = a.wd;
  const bool copy = a.copy != 0;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    // the wave's first chunk: wave-uniform, so the entries come through scalar loads
    const uint32_t ch = (uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 6));
    uint32_t e[U];
    v4f zv[U], lv[U], acc[U], mv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = chunks[ch + u];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      zv[u] = ldo<P>(a.z, i);
      if constexpr (BMOM) lv[u] = ldo<P>(a.blast, i);
      acc[u] = 0.0f;  // sma.c:66
    }
    const int nrep = (R > 0) ? R : a.nrep;
    // one chunk's registers at a time: unrolled further, the mixed form spills
#pragma nounroll
    for (int c = 0; c < nrep; c += RR) {
      // a stepping replica: x = w, y = g, l = last_i; one that only joins: x = s, y = w
      v4f x[U][RR], y[U][RR], l[U][RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;  // a guard, not a break: the unrolled body keeps its registers
        const bool step = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          // the stream is chosen by its (scalar) base, not by a branch around the loads
          x[u][r] = ldo<P>(step ? a.w[c + r] : a.s[c + r], i);
          y[u][r] = ldo<P>(step ? a.g[c + r] : a.w[c + r], i);
          if constexpr (MOM) {
            if (step) l[u][r] = ldo<P>(a.last[c + r], i);
          }
        }
      }
      // every load of the chunk in flight before the first use (task_barrier_kernel)
      __builtin_amdgcn_sched_barrier(0);
      // The multipliers, once per trip and behind the first replica chunk's
      // loads: the table entry is not waited for ahead of them.
      if (R > 0 || c == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t v0 = e[u] >> 1;
          if ((e[u] & 1u) == 0u) {  // wave-uniform
            mv[u] = mult[v0];       // a scalar load
          } else {
            const uint32_t f = (ch + u) * kOptChunk + lane * 4u;
#pragma unroll
            for (int k = 0; k < 4; ++k) mv[u][k] = mult[variable_of(bounds, nvars, v0, f + k)];
          }
        }
      }
      // The stores' byte offsets, made opaque here: the lookup's branches end
      // the loads' basic block, and an address carried over from it reaches the
      // stores as a 64-bit VGPR pair per stream; computed anew in this block
      // it folds into the "saddr + voffset" form again, as in task_barrier_kernel.
      uint32_t so[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        so[u] = (base + u * 64u) * 16u;
        asm volatile("" : "+v"(so[u]));
      }
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        const bool step = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
        const v4f rate = a.rate[c + r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = so[u];
          v4f sv = x[u][r], wn;
          if (step) {
            const v4f rv = rate * mv[u];  // r_iv, model.c:159-177
            v4f gv = y[u][r];
            if constexpr (WD) gv = vfma(wd, sv, gv);
            if constexpr (MOM) {
              gv = rv * gv;
              gv = vfma(mu, l[u][r], gv);
              sto<P>(a.last[c + r], i, gv);
              wn = vfma(one, gv, sv);
            } else {
              wn = vfma(rv, gv, sv);
            }
            if constexpr (KEEP) {
              sto<P>(a.s[c + r], i, sv);
              if constexpr (MOM || WD) sto<P>(a.g[c + r], i, gv);
            }
          } else {
            wn = y[u][r];
          }
          const v4f d = vfma(mone, zv[u], sv);
          acc[u] = vfma(al, d, acc[u]);
          sto<P>(a.w[c + r], i, vfma(nal, d, wn));
        }
      }
      if constexpr (R > 0) break;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (base + u * 64u) * 16u;
      asm volatile("" : "+v"(i));  // as `so` above
      v4f D = acc[u];
      if constexpr (BMOM) {
        D = vfma(mb, lv[u], D);
        sto<P>(a.blast, i, D);
      }
      zv[u] = vfma(one, D, zv[u]);
      sto<P>(a.z, i, zv[u]);
    }
    // Phase D is rare (a learning-rate boundary): the lane's own later store
    // to the same address wins.
    if (copy) {
      for (int r = 0; r < nrep; ++r) {
#pragma unroll
        for (int u = 0; u < U; ++u) sto<P>(a.w[r], (base + u * 64u) * 16u, zv[u]);
      }
    }
  }
}

// Only what a door reaches is compiled: the context's forms (no tail, unroll 1
// or 2, either policy) and the seam's (a tail, unroll 1, nontemporal).  Any
// other shape is hipErrorInvalidValue, before the launch.
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P>
hipError_t tbv_u(const TaskBarrierArgs &a, const VarTables &vt, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // whole chunks only, as launch_task_barrier; the bulk may be empty when a tail is all there is
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  int steps = 0;
  for (int r = 0; r < a.nrep; ++r) steps += (int)((a.step_mask >> r) & 1ull);
  const int joins = a.nrep - steps;
  const int reads = 1 + (BMOM ? 1 : 0) + steps * (2 + (MOM ? 1 : 0)) + joins * 2;
  const int writes = 1 + (BMOM ? 1 : 0) + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 1 + ((MOM || WD) ? 1 : 0) : 0)) + joins;
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {
    if constexpr (P != 1) {
      return hipErrorInvalidValue;
    } else {
      if (cfg.unroll != 1) return hipErrorInvalidValue;
      TaskBarrierArgs b = a;
      b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
      g.x += (unsigned)b.tail_blocks;
      hipExtLaunchKernelGGL((task_barrier_variables_kernel<R, MIXED, MOM, BMOM, WD, KEEP, 1, true, 1>), g,
                            dim3(cfg.block), lds, s, t.start, t.stop, 0, b, vt.chunks, vt.bounds, vt.mult, vt.nvars);
      return hipGetLastError();
    }
  }
  // Base momentum beside stepping replicas that have none, weight decay on: a
  // context has base->last iff its replicas were made with momentum, so only
  // the seam reaches this form, at policy 1 and unroll 1 (a caller-owned buffer
  // of whole chunks has no tail).
  constexpr bool kSeamOnly = MIXED && !MOM && BMOM && WD;
  if constexpr (kSeamOnly && P != 1) {
    return hipErrorInvalidValue;
  } else {
    if (cfg.unroll == 2) {
      if constexpr (kSeamOnly) return hipErrorInvalidValue;
      else
        hipExtLaunchKernelGGL((task_barrier_variables_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 2>), g,
                              dim3(cfg.block), lds, s, t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars);
    } else if (cfg.unroll == 1) {
      hipExtLaunchKernelGGL((task_barrier_variables_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 1>), g,
                            dim3(cfg.block), lds, s, t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.mult, vt.nvars);
    } else {
      return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
}

// The ladders below are launch_task_barrier's (task_barrier_kernels.hip).
template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tbv_all(const TaskBarrierArgs &a, const VarTables &vt, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  switch (a.nrep) {
    case 1: return tbv_u<1, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 2: return tbv_u<2, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 3: return tbv_u<3, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 4: return tbv_u<4, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 5: return tbv_u<5, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 6: return tbv_u<6, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 7: return tbv_u<7, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    case 8: return tbv_u<8, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
    default: return tbv_u<-1, false, MOM, MOM, WD, KEEP, P>(a, vt, cfg, s, t);
  }
}

template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tbv_form(const TaskBarrierArgs &a, const VarTables &vt, bool bmom, const LaunchConfig &cfg, hipStream_t s,
                    Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  if (a.nrep > 0 && a.step_mask == all && bmom == MOM) return tbv_all<MOM, WD, KEEP, P>(a, vt, cfg, s, t);
  return bmom ? tbv_u<-1, true, MOM, true, WD, KEEP, P>(a, vt, cfg, s, t)
              : tbv_u<-1, true, MOM, false, WD, KEEP, P>(a, vt, cfg, s, t);
}

template <bool KEEP, int P>
hipError_t tbv_conf(const TaskBarrierArgs &a, const VarTables &vt, bool bmom, const LaunchConfig &cfg, hipStream_t s,
                    Timing t) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom)
    return wd ? tbv_form<true, true, KEEP, P>(a, vt, bmom, cfg, s, t) : tbv_form<true, false, KEEP, P>(a, vt, bmom, cfg, s, t);
  return wd ? tbv_form<false, true, KEEP, P>(a, vt, bmom, cfg, s, t) : tbv_form<false, false, KEEP, P>(a, vt, bmom, cfg, s, t);
}

}  // namespace

hipError_t launch_task_barrier_variables(const TaskBarrierArgs &a, const VarTables &vt, bool keep_task_outputs,
                                         const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  // No table is read past its end: one entry per 256-float chunk of the bulk,
  // and every tail float has a variable.
  if (!vt.chunks || !vt.bounds || !vt.mult || vt.nvars == 0 || a.n4 < 0 || a.tail_lo < 0) return hipErrorInvalidValue;
  const uint64_t nchunks = ((uint64_t)vt.elements + kOptChunk - 1) / kOptChunk;
  if ((uint64_t)a.n4 * 4u > nchunks * kOptChunk) return hipErrorInvalidValue;
  if (a.tail_hi > a.tail_lo && a.tail_hi > (int64_t)vt.elements) return hipErrorInvalidValue;
  const bool bmom = a.blast != nullptr;
  if (cfg.policy == 1)
    return keep_task_outputs ? tbv_conf<true, 1>(a, vt, bmom, cfg, stream, t)
                             : tbv_conf<false, 1>(a, vt, bmom, cfg, stream, t);
  return keep_task_outputs ? tbv_conf<true, 0>(a, vt, bmom, cfg, stream, t)
                           : tbv_conf<false, 0>(a, vt, bmom, cfg, stream, t);
}

}  // namespace cbx
