// task_ssgd_clipped_kernels.hip -- synchronous SGD (update model WORKER) with
// gradient clipping by global L2 norm and the skip of a non-finite gradient
// (cbx_set_gradient_clip), for CDNA4 (gfx950): the clipped task step
// (cbx_replica_accumulate_clipped, cbx_ssgd_plan_accumulate_clipped) and the
// replicas' clipped task steps fused into the one-GPU barrier
// (cbx_step_and_synchronise_ssgd_clipped,
// cbx_ssgd_plan_step_and_optimise_clipped).
//
// Clipping is per replica, by the norm of that replica's own g: the norm pass
// and its one-wave reduce (launch_gradient_norm, clip_kernels.hip) leave each
// stepping replica's record (S, K, scale, flags) earlier on the stream.  Under
// S-SGD every replica's gradient goes into one accumulator whose result is
// broadcast to all of them, so one NaN would reach the base model and every
// replica in one barrier; a skipped replica therefore contributes NOTHING:
//
//   acc = the base gradient as found                              (not assumed zero)
//   per stepping replica i, list order (ascending id), record (scale_i, flags_i):
//     skip bit set:  nothing.  g_i, w_i and the rate are not loaded, acc takes no
//                    fma (not one with 0: 0 * NaN is NaN), g_i is not written
//     otherwise:     gv = scale_i * g_i                           one multiply, before the weight decay
//                    gv = fma(wd, w_i, gv)                        synchronoussgd.cu:20-26 (wd > 0)
//                    g_i = gv                                     kept outputs: always, as the SMA clipped step
//                    acc = fma(rate_i, gv, acc)                   :46-52
//   D = ratio * acc ; D = fma(mu, last, D) ; last = D ; z = fma(1, D, z)
//   base gradient = +0 ; w_j = z for every receiving replica j    as task_ssgd_kernels.hip
//
// ratio stays 1 / wpc whatever was skipped: a skipped replica is a zero in the
// mean.  Built with -ffp-contract=off, one fp32 operation per line above.
//
// The design is task_ssgd_kernel's with a clip policy: 16-byte float4s per lane
// behind an SGPR base and a 32-bit offset, acc in registers, no LDS, the
// stepping replicas unrolled up to one chunk and chunked beyond it.  Each
// record's {scale, flags} is one 8-byte load through a wave-uniform address
// from the constant address space (a scalar load; nothing is written through
// the scalar path): ahead of the trip loop in the unrolled forms, at the head of
// each chunk in the chunked one.  The skip is a wave-uniform branch around the
// replica's loads and another around its arithmetic and stores, so a skipped
// replica moves no byte: 4n to 12n fewer per skipped replica.  Every load of the
// replicas that are not skipped, and acc, z and last, is issued before the first
// use (sched_barrier).
//
// Bytes per element, R stepping and receiving, base momentum on, none skipped,
// beside the norm passes' 4R n:
//   no weight decay, g kept (12R + 24) n      discarded (8R + 24) n
//   weight decay,    g kept (16R + 24) n      discarded (12R + 24) n
// KEEP without WD is a form of its own here: the clipped step writes a kept g.
//
// A shared object of its own (libcrossbow_sma_ssgd_clipped.so): the device code
// of the other objects is not touched by it.  Only what a door reaches is
// compiled.
#include <hip/hip_ext.h>

#include "stream_helpers.h"
#include "task_ssgd_clipped_internal.h"

namespace cbx {

namespace {

static_assert(offsetof(ClipRecord, scale) == 16 && offsetof(ClipRecord, flags) == 20,
              "scale and flags are fetched by one 8-byte load at byte 16");

typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// {scale's bits, flags} of one record.  The record was written by an earlier
// kernel on the stream and is not written here, and its address is uniform: a
// load from the constant address space is a scalar load.
__device__ __forceinline__ v2u record_words(const ClipRecord *rec) {
  typedef const v2u __attribute__((address_space(4))) * cptr;
  return *(cptr)(reinterpret_cast<uintptr_t>(rec) + 16u);
}

// A chunk's entry past the last stepping replica: nothing to do, like a skip.
__device__ __forceinline__ v2u no_replica() {
  v2u w;
  w.x = 0u;
  w.y = kClipSkipped;
  return w;
}

__device__ __forceinline__ bool skipped(v2u w) { return (w.y & kClipSkipped) != 0u; }
__device__ __forceinline__ float scale_of(v2u w) { return __builtin_bit_cast(float, w.x); }

// ---------------------------------------------------------------------------
// (b) The clipped task step of one replica: ssgd_accumulate_kernel
// (sma_kernels.hip) with the record.  Reads g, acc (, w), writes g, acc:
// 16n B (+4n with weight decay); nothing on the skip bit.
// ---------------------------------------------------------------------------
template <bool WD, int P, bool TAIL, int U>
__global__ __launch_bounds__(512) void ssgd_accumulate_clipped_kernel(const SsgdArgs a,
                                                                      const ClipRecord *__restrict__ clip) {
  const v2u sf = record_words(clip);
  if (skipped(sf)) return;  // wave-uniform, before the first load: nothing is touched
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {  // the caller's last elements, one float per lane
      const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
      if (i >= a.tail_hi) return;
      float *g = reinterpret_cast<float *>(a.g), *acc = reinterpret_cast<float *>(a.acc);
      float gv = scale_of(sf) * g[i];
      if constexpr (WD) gv = fmaf(a.wd, reinterpret_cast<const float *>(a.wsrc)[i], gv);  // synchronoussgd.cu:20-26
      g[i] = gv;
      acc[i] = fmaf(a.rate, gv, acc[i]);  // :46-52
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f rate = a.rate, scale = scale_of(sf);
  [[maybe_unused]] const v4f wd = a.wd;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    v4f g[U], acc[U];
    [[maybe_unused]] v4f w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      g[u] = ldo<P>(a.g, i);
      acc[u] = ldo<P>(a.acc, i);
      if constexpr (WD) w[u] = ldo<P>(a.wsrc, i);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      g[u] = scale * g[u];
      if constexpr (WD) g[u] = vfma(wd, w[u], g[u]);
      sto<P>(a.g, i, g[u]);
      sto<P>(a.acc, i, vfma(rate, g[u], acc[u]));
    }
  }
}

// ---------------------------------------------------------------------------
// (a) The fused clipped barrier.
// ---------------------------------------------------------------------------

// The caller's last elements [a.tail_lo, a.tail_hi), one float per lane, by the
// launch's first a.tail_blocks workgroups (TAIL instantiations): the fp32
// sequence per element, the chunked walk and the skip are those of the float4
// path below.  Nothing at or past a.tail_hi is read, nothing outside the range
// is written.
template <bool WD, bool KEEP, bool MOM>
__device__ __forceinline__ void task_ssgd_clipped_tail_elem(const TaskSsgdArgs &a, const ClipRecordPtrs &rec) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  float *z = reinterpret_cast<float *>(a.z);
  float *accp = reinterpret_cast<float *>(a.acc);
  float acc = accp[i];
  const float z0 = z[i];
  [[maybe_unused]] float l0 = 0.0f;
  if constexpr (MOM) l0 = reinterpret_cast<const float *>(a.last)[i];
  for (int c = 0; c < a.nstep; c += kChunk) {
    v2u sf[kChunk];
    float y[kChunk];
    [[maybe_unused]] float x[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) sf[r] = c + r < a.nstep ? record_words(rec.p[c + r]) : no_replica();
    // every load of a chunk issued before its first store
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (skipped(sf[r])) continue;
      y[r] = reinterpret_cast<const float *>(a.g[c + r])[i];
      if constexpr (WD) x[r] = reinterpret_cast<const float *>(a.sw[c + r])[i];
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (skipped(sf[r])) continue;
      float gv = scale_of(sf[r]) * y[r];
      if constexpr (WD) gv = fmaf(a.wd, x[r], gv);  // synchronoussgd.cu:20-26
      if constexpr (KEEP) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
      acc = fmaf(a.rate[c + r], gv, acc);  // :46-52
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

// S in 1..kChunk: that many stepping replicas, fully unrolled, their records
// read once ahead of the trip loop; S == -1 takes a.nstep, walks them in
// register-resident chunks of kChunk and reads a chunk's records at its head
// (an entry past a.nstep counts as skipped).  WD: the weight decay (w_i is
// read).  KEEP: g_i is written, with or without weight decay.  MOM, P, TAIL and
// U as in task_ssgd_kernel.
template <int S, bool WD, bool KEEP, bool MOM, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_ssgd_clipped_kernel(const TaskSsgdArgs a, const ClipRecordPtrs rec) {
  static_assert(S == -1 || (S >= 1 && S <= kChunk), "the unrolled forms hold one chunk; somebody steps");
  constexpr int SS = (S > 0) ? S : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_ssgd_clipped_tail_elem<WD, KEEP, MOM>(a, rec);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  const v4f ratio = a.ratio, one = 1.0f, zero = 0.0f;
  [[maybe_unused]] const v4f mu = a.momentum, wd = a.wd;
  v2u sf[SS];
  if constexpr (S > 0) {
#pragma unroll
    for (int r = 0; r < SS; ++r) sf[r] = record_words(rec.p[r]);
  }
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
    const int nstep = (S > 0) ? S : a.nstep;
    // one chunk's registers at a time
#pragma nounroll
    for (int c = 0; c < nstep; c += SS) {
      if constexpr (S < 0) {
#pragma unroll
        for (int r = 0; r < SS; ++r) sf[r] = c + r < nstep ? record_words(rec.p[c + r]) : no_replica();
      }
      // y = g_i; with weight decay also x = w_i
      v4f y[U][SS];
      [[maybe_unused]] v4f x[U][SS];
#pragma unroll
      for (int r = 0; r < SS; ++r) {
        if (skipped(sf[r])) continue;  // wave-uniform: none of the replica's loads is issued
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
        if (skipped(sf[r])) continue;  // no arithmetic, no store: acc is not touched
        const v4f scale = scale_of(sf[r]), rate = a.rate[c + r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          v4f gv = scale * y[u][r];
          if constexpr (WD) gv = vfma(wd, x[u][r], gv);
          if constexpr (KEEP) sto<P>(a.g[c + r], (base + u * 64u) * 16u, gv);
          acc[u] = vfma(rate, gv, acc[u]);
        }
      }
      if constexpr (S > 0) break;
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
constexpr bool task_ssgd_clipped_compiled() {
  return TAIL ? (P == 1 && U == 1) : true;
}

template <int S, bool WD, bool KEEP, bool MOM, int P, bool TAIL, int U>
hipError_t tsc_go(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, dim3 g, int block, unsigned lds, hipStream_t s,
                  Timing t) {
  if constexpr (task_ssgd_clipped_compiled<P, TAIL, U>()) {
    hipExtLaunchKernelGGL((task_ssgd_clipped_kernel<S, WD, KEEP, MOM, P, TAIL, U>), g, dim3(block), lds, s, t.start,
                          t.stop, 0, a, rec);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <int S, bool WD, bool KEEP, bool MOM, int P>
hipError_t tsc_u(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop (launch_task_ssgd).
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane, this kernel's own count: a stepping replica is one
  // read (g), one more with weight decay (w), and one write where g is kept,
  // with or without weight decay; a receiving replica is one write; the base
  // model reads acc, z (, last) and writes them.  A skipped replica still
  // counts: the host does not know the flags.
  const int m = MOM ? 1 : 0;
  const int reads = a.nstep * (1 + (WD ? 1 : 0)) + 2 + m;
  const int writes = a.nstep * (KEEP ? 1 : 0) + a.nrecv + 2 + m;
  // The cap is launch_task_ssgd's rule, the averaging kernels' stream target
  // (kAveragingStreamsPerCU), with the counts above: at R = 8, 3 waves per CU
  // with 22 or 30 streams, 2 with 38 or 46.  A launch too small to fill the chip
  // stays uncapped (lds_for_occupancy).
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
    if (cfg.unroll == 1) return tsc_go<S, WD, KEEP, MOM, P, true, 1>(b, rec, g, cfg.block, lds, s, t);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return tsc_go<S, WD, KEEP, MOM, P, false, 2>(a, rec, g, cfg.block, lds, s, t);
  if (cfg.unroll == 1) return tsc_go<S, WD, KEEP, MOM, P, false, 1>(a, rec, g, cfg.block, lds, s, t);
  return hipErrorInvalidValue;
}

// The form ladder: the stepping replicas unrolled up to one chunk, chunked
// beyond it.  The receiving list is a runtime loop in every form.
template <bool WD, bool KEEP, bool MOM, int P>
hipError_t tsc_form(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, const LaunchConfig &cfg, hipStream_t s,
                    Timing t) {
  switch (a.nstep) {
    case 1: return tsc_u<1, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 2: return tsc_u<2, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 3: return tsc_u<3, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 4: return tsc_u<4, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 5: return tsc_u<5, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 6: return tsc_u<6, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 7: return tsc_u<7, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    case 8: return tsc_u<8, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
    default: return tsc_u<-1, WD, KEEP, MOM, P>(a, rec, cfg, s, t);
  }
}

template <bool MOM, int P>
hipError_t tsc_conf(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, bool keep, const LaunchConfig &cfg,
                    hipStream_t s, Timing t) {
  if (a.wd > 0.0f)
    return keep ? tsc_form<true, true, MOM, P>(a, rec, cfg, s, t) : tsc_form<true, false, MOM, P>(a, rec, cfg, s, t);
  return keep ? tsc_form<false, true, MOM, P>(a, rec, cfg, s, t) : tsc_form<false, false, MOM, P>(a, rec, cfg, s, t);
}

template <bool WD, int P>
hipError_t acc_clipped_p(const SsgdArgs &a0, const ClipRecord *rec, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const bool tail = a0.tail_hi > a0.tail_lo;
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 512 || (cfg.unroll != 1 && cfg.unroll != 2) || a0.n4 < 0 ||
      a0.n4 % (64ll * cfg.unroll) != 0 || (a0.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  SsgdArgs a = a0;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  const int reads = 2 + (WD ? 1 : 0), writes = 2;  // g, acc (, w) in; g, acc out
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  const dim3 b(cfg.block);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    if constexpr (P != 1) {
      return hipErrorInvalidValue;
    } else {
      a.tail_blocks = (int)((a.tail_hi - a.tail_lo + cfg.block - 1) / cfg.block);
      g.x += (unsigned)a.tail_blocks;
      if (cfg.unroll == 2)
        hipExtLaunchKernelGGL((ssgd_accumulate_clipped_kernel<WD, P, true, 2>), g, b, lds, s, t.start, t.stop, 0, a, rec);
      else
        hipExtLaunchKernelGGL((ssgd_accumulate_clipped_kernel<WD, P, true, 1>), g, b, lds, s, t.start, t.stop, 0, a, rec);
      return hipGetLastError();
    }
  }
  if (cfg.unroll == 2)
    hipExtLaunchKernelGGL((ssgd_accumulate_clipped_kernel<WD, P, false, 2>), g, b, lds, s, t.start, t.stop, 0, a, rec);
  else
    hipExtLaunchKernelGGL((ssgd_accumulate_clipped_kernel<WD, P, false, 1>), g, b, lds, s, t.start, t.stop, 0, a, rec);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_task_ssgd_clipped(const TaskSsgdArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                    const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (a.nstep < 1 || a.nstep > kMaxReplicas || a.nrecv < 0 || a.nrecv > kMaxReplicas) return hipErrorInvalidValue;
  for (int k = 0; k < a.nstep; ++k)
    if (!rec.p[k]) return hipErrorInvalidValue;
  const bool mom = a.momentum > 0.0f;  // synchronoussgd.c:64
  if (mom && !a.last) return hipErrorInvalidValue;
  if (cfg.policy == 1)
    return mom ? tsc_conf<true, 1>(a, rec, keep_task_outputs, cfg, stream, t)
               : tsc_conf<false, 1>(a, rec, keep_task_outputs, cfg, stream, t);
  return mom ? tsc_conf<true, 0>(a, rec, keep_task_outputs, cfg, stream, t)
             : tsc_conf<false, 0>(a, rec, keep_task_outputs, cfg, stream, t);
}

hipError_t launch_ssgd_accumulate_clipped(const SsgdArgs &a, const ClipRecord *rec, const LaunchConfig &cfg,
                                          hipStream_t stream, Timing t) {
  if (!rec) return hipErrorInvalidValue;
  const bool wd = a.wd > 0.0f;
  if (cfg.policy == 1)
    return wd ? acc_clipped_p<true, 1>(a, rec, cfg, stream, t) : acc_clipped_p<false, 1>(a, rec, cfg, stream, t);
  return wd ? acc_clipped_p<true, 0>(a, rec, cfg, stream, t) : acc_clipped_p<false, 0>(a, rec, cfg, stream, t);
}

}  // namespace cbx
