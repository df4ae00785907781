// task_elastic_kernels.hip -- the replicas' pending task steps fused into the
// one-GPU elastic-averaging barrier (cbx_step_and_synchronise_elastic,
// cbx_ea_plan_step_and_optimise), for CDNA4 (gfx950).
//
// EA-SGD (update model 3 with cbx_set_elastic_average): with tau = 1 every
// task step (kernels/optimisers/synchronouseamsgd.cu, whose call sequence is
// sma.cu's: sma_optimise_kernel) is followed by the elastic barrier
// (synch/synchronouseamsgd.c:42-90: averaging_kernel<kElasticW>), which on one
// device reads the replica's data AFTER the step and no snapshot.  Per
// element, with R replicas and momentum on:
//
//   R x step, then the barrier      (28R + 8R + 8) n B = (36R + 8) n
//   this kernel, s and g kept       (28R + 8) n
//   this kernel, s and g discarded  (20R + 8) n
//
// One streaming pass in the shape of the kernels it fuses (task_barrier_body.inc,
// averaging_kernels.hip): 16-byte float4s per lane behind an SGPR base and a
// 32-bit offset, every load of a replica chunk issued before the first
// arithmetic, acc in registers, no LDS.  The context's buffers are padded to
// kPadFloat4 and need no tail; buffers the caller owns take the TAIL
// instantiations.
//
// Per participating replica i (one fp32 operation per reference call, in their
// order; built with -ffp-contract=off):
//   stepping:
//     g = fma(wd, w, g)                               sma.cu:24-31 (wd > 0)
//     s = w                                           :71 / :87 (kept outputs only)
//     g = rate_i * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)   :52-74
//     or, without momentum, w' = fma(rate_i, g, w)    :90
//   only joining: w' = w_i
//   all: d = fma(-1, z, w') ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)   synchronouseamsgd.c:55-77
// then z = fma(1, acc, z) (:85-90), acc from +0 (:43).
//
// Unlike the SMA fused kernel (task_barrier_body.inc): d comes from the stepped
// w', not from a snapshot; a replica that only joins is one stream, not two;
// there is no base momentum and no Phase D, and no copy flag is looked at.
//
// This file is a shared object of its own (libcrossbow_sma_elastic_steps.so):
// the device code of libcrossbow_sma.so is not touched by it.  Only what a door
// reaches is compiled: the context's forms (no tail, unroll 1 or 2, either
// policy) and the seam's (a tail, unroll 1, nontemporal).
#include <hip/hip_ext.h>

#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {

static_assert(kMaxReplicas <= 64, "step_mask holds one bit per replica");

namespace {

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane, as in task_barrier_tail_elem: the fp32 sequence per element, the
// per-replica choice by a.step_mask (set for every replica in the all-step
// forms too) and the chunked replica walk are those of the float4 path below.
// Nothing at or past a.tail_hi is read, nothing outside the range is written.
template <bool MOM, bool WD, bool KEEP>
__device__ __forceinline__ void task_elastic_tail_elem(const TaskBarrierArgs &a) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  const float z0 = z[i];
  float acc = 0.0f;  // synchronouseamsgd.c:43
  for (int c = 0; c < a.nrep; c += kChunk) {
    float x[kChunk];
    [[maybe_unused]] float y[kChunk], l[kChunk];
    // every load of a chunk issued before its first store (sma_tail_elem)
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool stepping = ((a.step_mask >> (c + r)) & 1ull) != 0;
        x[r] = reinterpret_cast<const float *>(a.w[c + r])[i];
        if (stepping) {
          y[r] = reinterpret_cast<const float *>(a.g[c + r])[i];
          if constexpr (MOM) l[r] = reinterpret_cast<const float *>(a.last[c + r])[i];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool stepping = ((a.step_mask >> (c + r)) & 1ull) != 0;
        float wn = x[r];
        if (stepping) {
          const float rate = a.rate[c + r];
          float gv = y[r];
          if constexpr (WD) gv = fmaf(a.wd, x[r], gv);  // sma.cu:24-31
          if constexpr (MOM) {
            gv = rate * gv;                   // :52-56
            gv = fmaf(a.momentum, l[r], gv);  // :59-64
            reinterpret_cast<float *>(a.last[c + r])[i] = gv;  // :68
            wn = fmaf(1.0f, gv, x[r]);        // :74
          } else {
            wn = fmaf(rate, gv, x[r]);  // :90
          }
          if constexpr (KEEP) {
            reinterpret_cast<float *>(a.s[c + r])[i] = x[r];  // :71 / :87
            if constexpr (MOM || WD) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
          }
        }
        const float d = fmaf(-1.0f, z0, wn);                               // synchronouseamsgd.c:55-61
        reinterpret_cast<float *>(a.w[c + r])[i] = fmaf(-a.alpha, d, wn);  // :64-69
        acc = fmaf(a.alpha, d, acc);                                       // :72-77
      }
    }
  }
  z[i] = fmaf(1.0f, acc, z0);  // :85-90
}

// R > 0: that many replicas, fully unrolled (R <= kChunk), all of them
// stepping; R == -1 takes a.nrep and walks the replicas in register-resident
// chunks of kChunk.  MIXED: a.step_mask says which replicas step (a
// wave-uniform choice per replica); otherwise all of them do.  MOM / WD: the
// stepping replicas' momentum and weight decay.  KEEP: s_i and g_i of the
// stepping replicas are written as the plain step writes them; otherwise they
// are not touched.  TAIL: the launch's first a.tail_blocks workgroups do the
// caller's last elements (task_elastic_tail_elem); without it the kernel is the
// context's.  a.s of a replica that only joins, a.blast and a.copy are not read.
template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_elastic_kernel(const TaskBarrierArgs a) {
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_elastic_tail_elem<MOM, WD, KEEP>(a);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f al = a.alpha, nal = -a.alpha, one = 1.0f, mone = -1.0f;
  const v4f mu = a.momentum, wd = a.wd;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    v4f zv[U], acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      zv[u] = ldo<P>(a.z, (base + u * 64u) * 16u);
      acc[u] = 0.0f;  // synchronouseamsgd.c:43
    }
    const int nrep = (R > 0) ? R : a.nrep;
    // one chunk's registers at a time: unrolled further, the mixed form spills
#pragma nounroll
    for (int c = 0; c < nrep; c += RR) {
      // x = w_i; of a stepping replica also y = g_i and l = last_i
      v4f x[U][RR], y[U][RR], l[U][RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;  // a guard, not a break: the unrolled body keeps its registers
        const bool stepping = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          x[u][r] = ldo<P>(a.w[c + r], i);
          // a replica that only joins is this one stream: its g and last_i may not exist
          if (stepping) {
            y[u][r] = ldo<P>(a.g[c + r], i);
            if constexpr (MOM) l[u][r] = ldo<P>(a.last[c + r], i);
          }
        }
      }
      // every load of the chunk in flight before the first use (sma_fused_kernel)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        const bool stepping = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
        const v4f rate = a.rate[c + r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          const v4f wv = x[u][r];
          v4f wn = wv;
          if (stepping) {
            v4f gv = y[u][r];
            if constexpr (WD) gv = vfma(wd, wv, gv);
            if constexpr (MOM) {
              gv = rate * gv;
              gv = vfma(mu, l[u][r], gv);
              sto<P>(a.last[c + r], i, gv);
              wn = vfma(one, gv, wv);
            } else {
              wn = vfma(rate, gv, wv);
            }
            if constexpr (KEEP) {
              sto<P>(a.s[c + r], i, wv);
              if constexpr (MOM || WD) sto<P>(a.g[c + r], i, gv);
            }
          }
          const v4f d = vfma(mone, zv[u], wn);
          sto<P>(a.w[c + r], i, vfma(nal, d, wn));
          acc[u] = vfma(al, d, acc[u]);
        }
      }
      if constexpr (R > 0) break;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) sto<P>(a.z, (base + u * 64u) * 16u, vfma(one, acc[u], zv[u]));
  }
}

// Only what a door reaches is compiled (hipErrorInvalidValue otherwise, before
// the launch): the tail rides the nontemporal policy at unroll 1, the seam's
// shape; without one, unroll 1 or 2 at either policy.
template <int P, bool TAIL, int U>
constexpr bool task_elastic_compiled() {
  return TAIL ? (P == 1 && U == 1) : true;
}

template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
hipError_t te_go(const TaskBarrierArgs &a, dim3 g, int block, unsigned lds, hipStream_t s, Timing t) {
  if constexpr (task_elastic_compiled<P, TAIL, U>()) {
    hipExtLaunchKernelGGL((task_elastic_kernel<R, MIXED, MOM, WD, KEEP, P, TAIL, U>), g, dim3(block), lds, s, t.start,
                          t.stop, 0, a);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P>
hipError_t te_u(const TaskBarrierArgs &a, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop (tb_u, task_barrier_launch.h): the
  // context's padded buffers are whole kPadFloat4s, the bulk of a caller-owned
  // buffer is whole chunks only and may be empty when a tail is all there is.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane: z is read and written; a stepping replica reads w,
  // g (, last_i) and writes w (, last_i) (, s, and g where the step changes
  // it); one that only joins reads w and writes w.
  int steps = 0;
  for (int r = 0; r < a.nrep; ++r) steps += (int)((a.step_mask >> r) & 1ull);
  const int joins = a.nrep - steps;
  const int reads = 1 + steps * (2 + (MOM ? 1 : 0)) + joins;
  const int writes = 1 + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 1 + (MOM || WD ? 1 : 0) : 0)) + joins;
  // The cap is sized by the bulk's grid: the few tail workgroups are not
  // counted.  Its stream target is the SMA fused kernels' (kStreamsPerCU): at
  // R = 8 with momentum that and the averaging kernels' 76 both give 2 waves
  // per CU, kept or discarded (profiles/task_barrier_elastic/sweep.jsonl).
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    TaskBarrierArgs b = a;
    b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
    g.x += (unsigned)b.tail_blocks;
    if (cfg.unroll == 1) return te_go<R, MIXED, MOM, WD, KEEP, P, true, 1>(b, g, cfg.block, lds, s, t);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return te_go<R, MIXED, MOM, WD, KEEP, P, false, 2>(a, g, cfg.block, lds, s, t);
  if (cfg.unroll == 1) return te_go<R, MIXED, MOM, WD, KEEP, P, false, 1>(a, g, cfg.block, lds, s, t);
  return hipErrorInvalidValue;
}

// The form ladder.  task_barrier_launch.h's picks its unrolled path on the base
// model's momentum being the replicas'; this barrier has no base momentum, so
// the unrolled path is taken whenever every participating replica steps.
template <bool MOM, bool WD, bool KEEP, int P>
hipError_t te_form(const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  if (a.nrep > 0 && a.step_mask == all) {
    switch (a.nrep) {
      case 1: return te_u<1, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 2: return te_u<2, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 3: return te_u<3, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 4: return te_u<4, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 5: return te_u<5, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 6: return te_u<6, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 7: return te_u<7, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      case 8: return te_u<8, false, MOM, WD, KEEP, P>(a, cfg, s, t);
      default: return te_u<-1, false, MOM, WD, KEEP, P>(a, cfg, s, t);
    }
  }
  // Some replicas only join, nobody steps, or nobody is there at all: the
  // runtime-chunked form with a choice per replica.
  return te_u<-1, true, MOM, WD, KEEP, P>(a, cfg, s, t);
}

template <bool KEEP, int P>
hipError_t te_conf(const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom) return wd ? te_form<true, true, KEEP, P>(a, cfg, s, t) : te_form<true, false, KEEP, P>(a, cfg, s, t);
  return wd ? te_form<false, true, KEEP, P>(a, cfg, s, t) : te_form<false, false, KEEP, P>(a, cfg, s, t);
}

}  // namespace

hipError_t launch_task_elastic(const TaskBarrierArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                               hipStream_t stream, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  if (a.step_mask == 0 && (a.momentum > 0.0f || a.wd > 0.0f)) return hipErrorInvalidValue;  // nobody's to be
  if (cfg.policy == 1)
    return keep_task_outputs ? te_conf<true, 1>(a, cfg, stream, t) : te_conf<false, 1>(a, cfg, stream, t);
  return keep_task_outputs ? te_conf<true, 0>(a, cfg, stream, t) : te_conf<false, 0>(a, cfg, stream, t);
}

}  // namespace cbx
