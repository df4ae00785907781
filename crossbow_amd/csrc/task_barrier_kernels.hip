// task_barrier_kernels.hip -- the replicas' pending task steps fused into the
// one-GPU SMA barrier (cbx_step_and_synchronise), for CDNA4 (gfx950).
//
// With tau = 1 every task step (sma_optimise_kernel) is followed by a barrier
// (sma_fused_kernel) before the replica is read again.  The two passes read
// and write w_i twice, and the barrier reads back an s_i the step wrote only
// for it.  Per element, with R replicas and momentum on:
//
//   R x step, then the barrier      (28R + 12R + 16) n B = (40R + 16) n
//   this kernel, s and g kept       (28R + 16) n
//   this kernel, s and g discarded  (20R + 16) n
//
// One streaming pass in the shape of the kernels it fuses: 16-byte float4s per
// lane behind an SGPR base and a 32-bit offset, every load of a replica chunk
// issued before the first arithmetic, acc in registers, no LDS.  The context's
// buffers are padded to kPadFloat4 and need no tail; buffers the caller owns
// (cbx_sma_plan_step_and_optimise) take the TAIL instantiations.
//
// Arithmetic is the two kernels', one fp32 operation per reference call, in
// their order (built with -ffp-contract=off): for a stepping replica i
//   g = fma(wd, w, g)                              sma.cu:24-31 (wd > 0)
//   s = w                                          :71 / :87
//   g = rate_i * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)   :52-74
//   or, without momentum, w' = fma(rate_i, g, w)   :90
// for a replica that only joins the barrier s = s_i, w' = w_i; then for both
//   d = fma(-1, z, s) ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)    sma.c:79-107
// and D = acc ; D = fma(0.9, last, D), last = D ; z = fma(1, D, z)             sma.c:148-174
// With a copy request (Phase D, sma.c:185-227) every w_i becomes the new z;
// last_i (and s_i, g_i) are written all the same.
#include <hip/hip_ext.h>

#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {

static_assert(sizeof(TaskBarrierArgs) <= 4096, "the kernel argument block must stay under HIP's 4 KB");
static_assert(kMaxReplicas <= 64, "step_mask holds one bit per replica");

namespace {

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane, as in the SMA kernels (sma_tail_elem, sma_kernels.hip): the fp32
// sequence per element, the per-replica choice by a.step_mask (set for every
// replica in the all-step forms too), the chunked replica walk and Phase D are
// those of the float4 path below.
template <bool MOM, bool BMOM, bool WD, bool KEEP>
__device__ __forceinline__ void task_barrier_tail_elem(const TaskBarrierArgs &a) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  float z0 = z[i];
  float l0 = 0.0f;
  if constexpr (BMOM) l0 = reinterpret_cast<const float *>(a.blast)[i];
  float acc = 0.0f;  // sma.c:66
  for (int c = 0; c < a.nrep; c += kChunk) {
    // a stepping replica: x = w, y = g, l = last_i; one that only joins: x = s, y = w
    float x[kChunk], y[kChunk];
    [[maybe_unused]] float l[kChunk];
    // every load of a chunk issued before its first store (sma_tail_elem)
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
          const float rate = a.rate[c + r];
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

// R > 0: that many replicas, fully unrolled (R <= kChunk); R == -1 takes
// a.nrep and walks the replicas in register-resident chunks of kChunk.
// MIXED: a.step_mask says which replicas step (a wave-uniform branch per
// replica); otherwise all of them do.  MOM / WD: the stepping replicas'
// momentum and weight decay; BMOM: the base model's momentum (a.blast).
// KEEP: s_i and g_i of the stepping replicas are written as the plain step
// writes them; otherwise they are not touched.  a.copy is wave-uniform too.
// TAIL: the launch's first a.tail_blocks workgroups do the caller's last
// elements (task_barrier_tail_elem); without it the kernel is the context's.
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_kernel(const TaskBarrierArgs a) {
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_barrier_tail_elem<MOM, BMOM, WD, KEEP>(a);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f al = a.alpha, nal = -a.alpha, mb = kBaseMomentum, one = 1.0f, mone = -1.0f;
  const v4f mu = a.momentum, wd = a.wd;
  const bool copy = a.copy != 0;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    v4f zv[U], lv[U], acc[U];
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
          // the stream is chosen by its (scalar) base, not by a branch around the
          // loads: branches here cost the mixed form its unrolled registers
          x[u][r] = ldo<P>(step ? a.w[c + r] : a.s[c + r], i);
          y[u][r] = ldo<P>(step ? a.g[c + r] : a.w[c + r], i);
          if constexpr (MOM) {
            if (step) l[u][r] = ldo<P>(a.last[c + r], i);
          }
        }
      }
      // every load of the chunk in flight before the first use (sma_fused_kernel)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        const bool step = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
        const v4f rate = a.rate[c + r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          v4f sv = x[u][r], wn;
          if (step) {
            v4f gv = y[u][r];
            if constexpr (WD) gv = vfma(wd, sv, gv);
            if constexpr (MOM) {
              gv = rate * gv;
              gv = vfma(mu, l[u][r], gv);
              sto<P>(a.last[c + r], i, gv);
              wn = vfma(one, gv, sv);
            } else {
              wn = vfma(rate, gv, sv);
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
      const uint32_t i = (base + u * 64u) * 16u;
      v4f D = acc[u];
      if constexpr (BMOM) {
        D = vfma(mb, lv[u], D);
        sto<P>(a.blast, i, D);
      }
      zv[u] = vfma(one, D, zv[u]);
      sto<P>(a.z, i, zv[u]);
    }
    // Phase D is rare (a learning-rate boundary): the loop above stays free of
    // branches, and the lane's own later store to the same address wins.
    if (copy) {
      for (int r = 0; r < nrep; ++r) {
#pragma unroll
        for (int u = 0; u < U; ++u) sto<P>(a.w[r], (base + u * 64u) * 16u, zv[u]);
      }
    }
  }
}

template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P>
hipError_t tb_u(const TaskBarrierArgs &a, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop.  The context's padded buffers are
  // whole kPadFloat4s; the bulk of a caller-owned buffer is whole chunks only
  // (e.g. 1,280 float4s), and may be empty when a tail is all there is.  The
  // check stands in front of the context's launches too, which had none: the
  // arena's whole kPadFloat4s and the setter's shapes always pass it.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.unroll < 1 || a.n4 < 0 || a.n4 % (64ll * cfg.unroll) != 0 ||
      (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane: a stepping replica reads w, g (, last_i) and
  // writes w (, last_i) (, s, g); one that only joins reads s, w and writes w.
  int steps = 0;
  for (int r = 0; r < a.nrep; ++r) steps += (int)((a.step_mask >> r) & 1ull);
  const int joins = a.nrep - steps;
  const int reads = 1 + (BMOM ? 1 : 0) + steps * (2 + (MOM ? 1 : 0)) + joins * 2;
  const int writes = 1 + (BMOM ? 1 : 0) + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 1 + ((MOM || WD) ? 1 : 0) : 0)) + joins;
  // the cap is sized by the bulk's grid: the few tail workgroups are not counted
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front (nontemporal policy only)
    if constexpr (P != 1) {
      return hipErrorInvalidValue;
    } else {
      TaskBarrierArgs b = a;
      b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
      g.x += (unsigned)b.tail_blocks;
      if (cfg.unroll == 2)
        hipExtLaunchKernelGGL((task_barrier_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, true, 2>), g, dim3(cfg.block), lds, s,
                              t.start, t.stop, 0, b);
      else if (cfg.unroll == 1)
        hipExtLaunchKernelGGL((task_barrier_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, true, 1>), g, dim3(cfg.block), lds, s,
                              t.start, t.stop, 0, b);
      else
        return hipErrorInvalidValue;
      return hipGetLastError();
    }
  }
  if (cfg.unroll == 2)
    hipExtLaunchKernelGGL((task_barrier_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 2>), g, dim3(cfg.block), lds, s,
                          t.start, t.stop, 0, a);
  else if (cfg.unroll == 1)
    hipExtLaunchKernelGGL((task_barrier_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 1>), g, dim3(cfg.block), lds, s,
                          t.start, t.stop, 0, a);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// Every participating replica steps, with the base model's momentum on iff
// theirs is (what the setters produce): the BSP case, unrolled for R <= kChunk.
template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tb_all(const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  switch (a.nrep) {
    case 1: return tb_u<1, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 2: return tb_u<2, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 3: return tb_u<3, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 4: return tb_u<4, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 5: return tb_u<5, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 6: return tb_u<6, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 7: return tb_u<7, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    case 8: return tb_u<8, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
    default: return tb_u<-1, false, MOM, MOM, WD, KEEP, P>(a, cfg, s, t);
  }
}

// Anything else (some replicas only join, no replica at all, base and replica
// momentum that differ): the runtime-chunked form with a branch per replica.
template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tb_mixed(const TaskBarrierArgs &a, bool bmom, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  return bmom ? tb_u<-1, true, MOM, true, WD, KEEP, P>(a, cfg, s, t) : tb_u<-1, true, MOM, false, WD, KEEP, P>(a, cfg, s, t);
}

template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tb_form(const TaskBarrierArgs &a, bool bmom, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  if (a.nrep > 0 && a.step_mask == all && bmom == MOM) return tb_all<MOM, WD, KEEP, P>(a, cfg, s, t);
  return tb_mixed<MOM, WD, KEEP, P>(a, bmom, cfg, s, t);
}

template <bool KEEP, int P>
hipError_t tb_conf(const TaskBarrierArgs &a, bool bmom, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom) return wd ? tb_form<true, true, KEEP, P>(a, bmom, cfg, s, t) : tb_form<true, false, KEEP, P>(a, bmom, cfg, s, t);
  return wd ? tb_form<false, true, KEEP, P>(a, bmom, cfg, s, t) : tb_form<false, false, KEEP, P>(a, bmom, cfg, s, t);
}

}  // namespace

hipError_t launch_task_barrier(const TaskBarrierArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                               hipStream_t stream, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  const bool bmom = a.blast != nullptr;
  if (cfg.policy == 1)
    return keep_task_outputs ? tb_conf<true, 1>(a, bmom, cfg, stream, t) : tb_conf<false, 1>(a, bmom, cfg, stream, t);
  return keep_task_outputs ? tb_conf<true, 0>(a, bmom, cfg, stream, t) : tb_conf<false, 0>(a, bmom, cfg, stream, t);
}

}  // namespace cbx
