// task_ssgd_kernels.hip -- the replicas' pending task steps fused into the
// one-GPU synchronous-SGD barrier (cbx_step_and_synchronise_ssgd,
// cbx_ssgd_plan_step_and_optimise), for CDNA4 (gfx950).
//
// S-SGD (update model WORKER): with tau = 1 every task step
// (kernels/optimisers/synchronoussgd.cu:3-56: ssgd_accumulate_kernel, a pass
// over the device's base gradient per replica) is followed by the barrier
// (synch/synchronoussgd.c:13-106 with common.c:198-220: ssgd_apply_kernel).  Per
// element, with R replicas stepping and receiving and base momentum on:
//
//   R x step, then the barrier            (12R + 4R + 24) n B = (16R + 24) n
//   the same with weight decay            (20R + 4R + 24) n   = (24R + 24) n
//   this kernel, no weight decay          (4R + 4R + 24) n    = (8R + 24) n
//   this kernel, weight decay, g kept     (16R + 24) n
//   this kernel, weight decay, g dropped  (12R + 24) n
//
// One streaming pass in the shape of the kernels it fuses: 16-byte float4s per
// lane behind an SGPR base and a 32-bit offset, acc, z, last and every load of
// a stepping chunk issued before the first arithmetic, acc in registers, no LDS.
// The context's buffers are padded to kPadFloat4 and need no tail; buffers the
// caller owns take the TAIL instantiations.
//
// Per element (one fp32 operation per reference call, in their order; built
// with -ffp-contract=off):
//   acc = the base gradient as found                              (not assumed zero)
//   per stepping replica i, list order (ascending id):
//     gv = g_i ; gv = fma(wd, w_i, gv) ; g_i = gv                 synchronoussgd.cu:20-26 (wd > 0; kept outputs only)
//     acc = fma(rate_i, gv, acc)                                  :46-52
//   D = ratio * acc                                               synchronoussgd.c:55-62
//   D = fma(mu, last, D) ; last = D                               :64-76 (base momentum, not forced to 0.9)
//   z = fma(1, D, z)                                              :79-84
//   base gradient = +0                                            :103
//   w_j = z for every receiving replica j                         common.c:198-220
//
// Unlike the SMA and the elastic fused kernels: the stepping replicas feed one
// accumulator that starts from memory, their w is an input of the weight decay
// only, and the result is a broadcast, so the stepping and the receiving
// replicas are two lists (a replica that only joins is one write stream).  A
// stepping replica's w_i is read before the same lane writes z into it: every
// element belongs to one lane of one trip, and the broadcast is that trip's
// last act.
//
// This file is a shared object of its own (libcrossbow_sma_ssgd_steps.so): the
// device code of the other objects is not touched by it.  Only what a door
// reaches is compiled: the context's forms (no tail, unroll 1 or 2, either
// policy) and the seam's (a tail, unroll 1, nontemporal).
#include <hip/hip_ext.h>

#include "stream_helpers.h"
#include "task_ssgd_internal.h"

namespace cbx {

namespace {

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane: the fp32 sequence per element and the chunked walk of the stepping
// replicas are those of the float4 path below.  Nothing at or past a.tail_hi
// is read, nothing outside the range is written.
template <bool WD, bool KEEP, bool MOM>
__device__ __forceinline__ void task_ssgd_tail_elem(const TaskSsgdArgs &a) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  float *accp = reinterpret_cast<float *>(a.acc);
  float acc = accp[i];
  const float z0 = z[i];
  [[maybe_unused]] float l0 = 0.0f;
  if constexpr (MOM) l0 = reinterpret_cast<const float *>(a.last)[i];
  for (int c = 0; c < a.nstep; c += kChunk) {
    float y[kChunk];
    [[maybe_unused]] float x[kChunk];
    // every load of a chunk issued before its first store (sma_tail_elem)
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nstep) {
        y[r] = reinterpret_cast<const float *>(a.g[c + r])[i];
        if constexpr (WD) x[r] = reinterpret_cast<const float *>(a.sw[c + r])[i];
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nstep) {
        float gv = y[r];
        if constexpr (WD) {
          gv = fmaf(a.wd, x[r], gv);  // synchronoussgd.cu:20-26
          if constexpr (KEEP) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
        }
        acc = fmaf(a.rate[c + r], gv, acc);  // :46-52
      }
    }
  }
  float D = a.ratio * acc;  // synchronoussgd.c:55-62
  if constexpr (MOM) {
    D = fmaf(a.momentum, l0, D);  // :64-76
    reinterpret_cast<float *>(a.last)[i] = D;
  }
  const float zv = fmaf(1.0f, D, z0);  // :79-84
  z[i] = zv;
  accp[i] = 0.0f;  // :103
  for (int r = 0; r < a.nrecv; ++r) reinterpret_cast<float *>(a.w[r])[i] = zv;  // common.c:198-220
}

// S >= 0: that many stepping replicas, fully unrolled (S <= kChunk; 0: the
// barrier alone, nobody steps); S == -1 takes a.nstep and walks them in
// register-resident chunks of kChunk.  WD: the stepping replicas' weight decay
// (their w is read).  KEEP (with WD only): g_i is written as the plain step
// writes it; otherwise it is not touched.  MOM: the base model's momentum.
// TAIL: the launch's first a.tail_blocks workgroups do the caller's last
// elements (task_ssgd_tail_elem); without it the kernel is the context's.  The
// receiving replicas are a runtime loop of stores, as in ssgd_apply_kernel.
template <int S, bool WD, bool KEEP, bool MOM, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_ssgd_kernel(const TaskSsgdArgs a) {
  static_assert(S >= -1 && S <= kChunk, "the unrolled forms hold one chunk");
  static_assert(WD || !KEEP, "without weight decay the step writes no g: one form");
  static_assert(S != 0 || !WD, "nobody steps: nobody's weight decay");
  constexpr int SS = (S > 0) ? S : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_ssgd_tail_elem<WD, KEEP, MOM>(a);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f ratio = a.ratio, one = 1.0f, zero = 0.0f;
  [[maybe_unused]] const v4f mu = a.momentum, wd = a.wd;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    v4f acc[U], zv[U];
    [[maybe_unused]] v4f l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      acc[u] = ldo<P>(a.acc, i);  // as the call finds it: earlier task steps may have added into it
      zv[u] = ldo<P>(a.z, i);
      if constexpr (MOM) l[u] = ldo<P>(a.last, i);
    }
    if constexpr (S != 0) {
      const int nstep = (S > 0) ? S : a.nstep;
      // one chunk's registers at a time
#pragma nounroll
      for (int c = 0; c < nstep; c += SS) {
        // y = g_i; with weight decay also x = w_i
        v4f y[U][SS];
        [[maybe_unused]] v4f x[U][SS];
#pragma unroll
        for (int r = 0; r < SS; ++r) {
          if (S < 0 && c + r >= nstep) continue;  // a guard, not a break: the unrolled body keeps its registers
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint32_t i = (base + u * 64u) * 16u;
            y[u][r] = ldo<P>(a.g[c + r], i);
            if constexpr (WD) x[u][r] = ldo<P>(a.sw[c + r], i);
          }
        }
        // every load of the chunk, and acc, z and last, in flight before the first use
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < SS; ++r) {
          if (S < 0 && c + r >= nstep) continue;
          const v4f rate = a.rate[c + r];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            v4f gv = y[u][r];
            if constexpr (WD) {
              gv = vfma(wd, x[u][r], gv);
              if constexpr (KEEP) sto<P>(a.g[c + r], (base + u * 64u) * 16u, gv);
            }
            acc[u] = vfma(rate, gv, acc[u]);
          }
        }
        if constexpr (S > 0) break;
      }
    } else {
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      v4f D = ratio * acc[u];
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

// Only what a door reaches is compiled (hipErrorInvalidValue otherwise, before
// the launch): the tail rides the nontemporal policy at unroll 1, the seam's
// shape; without one, unroll 1 or 2 at either policy.
template <int P, bool TAIL, int U>
constexpr bool task_ssgd_compiled() {
  return TAIL ? (P == 1 && U == 1) : true;
}

template <int S, bool WD, bool KEEP, bool MOM, int P, bool TAIL, int U>
hipError_t ts_go(const TaskSsgdArgs &a, dim3 g, int block, unsigned lds, hipStream_t s, Timing t) {
  if constexpr (task_ssgd_compiled<P, TAIL, U>()) {
    hipExtLaunchKernelGGL((task_ssgd_kernel<S, WD, KEEP, MOM, P, TAIL, U>), g, dim3(block), lds, s, t.start, t.stop, 0,
                          a);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int S, bool WD, bool KEEP, bool MOM, int P>
hipError_t ts_u(const TaskSsgdArgs &a, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop: the context's padded buffers are
  // whole kPadFloat4s, the bulk of a caller-owned buffer is whole chunks only
  // and may be empty when a tail is all there is.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane, the kernel's own count: a stepping replica is one
  // read (g), one more with weight decay (w) and then one write where g is
  // kept; a receiving replica is one write; the base model reads acc, z
  // (, last) and writes them.
  const int m = MOM ? 1 : 0;
  const int reads = a.nstep * (1 + (WD ? 1 : 0)) + 2 + m;
  const int writes = a.nstep * (WD && KEEP ? 1 : 0) + a.nrecv + 2 + m;
  // The cap is sized by the bulk's grid: the few tail workgroups are not
  // counted.  Its stream target is the averaging kernels'
  // (kAveragingStreamsPerCU), which like this one hold one float4 per stream
  // and lane: at R = 8 it gives 3 waves per CU without weight decay (22
  // streams), 2 with it (38) and 3 with it and the outputs discarded (30), the
  // fastest row of each in profiles/task_barrier_ssgd/sweep.jsonl; the SMA
  // kernels' 56 differs in the last only, 2 waves, 6 % slower there.  A launch
  // too small to fill the chip stays uncapped (lds_for_occupancy).
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
    if (cfg.unroll == 1) return ts_go<S, WD, KEEP, MOM, P, true, 1>(b, g, cfg.block, lds, s, t);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return ts_go<S, WD, KEEP, MOM, P, false, 2>(a, g, cfg.block, lds, s, t);
  if (cfg.unroll == 1) return ts_go<S, WD, KEEP, MOM, P, false, 1>(a, g, cfg.block, lds, s, t);
  return hipErrorInvalidValue;
}

// The form ladder: the stepping replicas unrolled up to one chunk, chunked
// beyond it.  The receiving list is a runtime loop in every form.
template <bool WD, bool KEEP, bool MOM, int P>
hipError_t ts_form(const TaskSsgdArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  switch (a.nstep) {
    case 1: return ts_u<1, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 2: return ts_u<2, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 3: return ts_u<3, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 4: return ts_u<4, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 5: return ts_u<5, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 6: return ts_u<6, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 7: return ts_u<7, WD, KEEP, MOM, P>(a, cfg, s, t);
    case 8: return ts_u<8, WD, KEEP, MOM, P>(a, cfg, s, t);
    default: return ts_u<-1, WD, KEEP, MOM, P>(a, cfg, s, t);
  }
}

template <bool MOM, int P>
hipError_t ts_conf(const TaskSsgdArgs &a, bool keep, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  if (a.nstep == 0) return ts_u<0, false, false, MOM, P>(a, cfg, s, t);  // the barrier alone
  // without weight decay the step writes no g: kept and discarded are one kernel
  if (!(a.wd > 0.0f)) return ts_form<false, false, MOM, P>(a, cfg, s, t);
  return keep ? ts_form<true, true, MOM, P>(a, cfg, s, t) : ts_form<true, false, MOM, P>(a, cfg, s, t);
}

}  // namespace

hipError_t launch_task_ssgd(const TaskSsgdArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                            hipStream_t stream, Timing t) {
  if (a.nstep < 0 || a.nstep > kMaxReplicas || a.nrecv < 0 || a.nrecv > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nstep == 0 && a.wd > 0.0f) return hipErrorInvalidValue;  // nobody's to be
  const bool mom = a.momentum > 0.0f;                            // synchronoussgd.c:64
  if (mom && !a.last) return hipErrorInvalidValue;
  if (cfg.policy == 1)
    return mom ? ts_conf<true, 1>(a, keep_task_outputs, cfg, stream, t)
               : ts_conf<false, 1>(a, keep_task_outputs, cfg, stream, t);
  return mom ? ts_conf<true, 0>(a, keep_task_outputs, cfg, stream, t)
             : ts_conf<false, 0>(a, keep_task_outputs, cfg, stream, t);
}

}  // namespace cbx
