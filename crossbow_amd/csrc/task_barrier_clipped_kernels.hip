// task_barrier_clipped_kernels.hip -- the replicas' pending task steps, clipped
// by global L2 norm, fused into the one-GPU SMA barrier
// (cbx_step_and_synchronise_clipped, cbx_sma_plan_step_and_optimise_clipped),
// for CDNA4 (gfx950).
//
// task_barrier_kernel (task_barrier_kernels.hip) plus the CLIP arithmetic of
// sma_optimise_kernel (sma_kernels.hip): the same single streaming pass,
// float4s behind an SGPR base and a 32-bit offset, every load of a replica
// chunk issued before the first arithmetic, acc in registers, no LDS,
// R <= kChunk unrolled and larger R in chunks of kChunk, the mixed form chosen
// by pointer.  Stepping replica i has a record of its own (cbx_clip_stats),
// left by the norm reduce (clip_kernels.hip) in front of this launch:
//   g = scale_i * g                                one fp32 multiply, before weight decay
// and then task_barrier_kernel's sequence (built with -ffp-contract=off):
//   g = fma(wd, w, g)                              sma.cu:24-31 (wd > 0)
//   s = w                                          :71 / :87
//   g = rate_i * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)   :52-74
//   or, without momentum, w' = fma(rate_i, g, w)   :90
// A kept g_i is always written, as the clipped step writes it.  When the
// record carries the skip bit the step is s = w and nothing else: last_i and
// g_i are stored with the bits that were loaded, w' = w.  For a replica that
// only joins the barrier s = s_i, w' = w_i; then for all of them
//   d = fma(-1, z, s) ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)    sma.c:79-107
// and D = acc ; D = fma(0.9, last, D), last = D ; z = fma(1, D, z)             sma.c:148-174
// With a copy request (Phase D, sma.c:185-227) every w_i becomes the new z.
//
// The skip is known only on the device, and a branch around a replica's
// loads or stores costs the unrolled chunk its registers: it is
// a select per stored word between what was loaded and what was computed, on
// integer views, so no arithmetic instruction touches a value that has to stay
// a bit copy (a signalling NaN keeps its payload).  Every store is issued
// either way.
//
// The record pointers are a kernel parameter of their own beside
// TaskBarrierArgs.  scale and flags are neighbours in the record (bytes 16 and
// 20): one 8-byte scalar load per replica, a chunk's issued together behind
// the chunk's float4 loads and first used after the last of them.
//
// This file is a shared object of its own (libcrossbow_sma_clipped.so): the
// device code of libcrossbow_sma.so is not touched by it.
#include <hip/hip_ext.h>

#include <cstddef>

#include "clip_internal.h"
#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {

static_assert(offsetof(ClipRecord, scale) == 16 && offsetof(ClipRecord, flags) == 20,
              "scale and flags are fetched by one 8-byte load at byte 16");
static_assert(sizeof(TaskBarrierArgs) + sizeof(ClipRecordPtrs) <= 4096,
              "the kernel argument block must stay under HIP's 4 KB");

namespace {

typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// {scale's bits, flags} of one record.  The record was written by an earlier
// kernel on the stream and is not written here, and its address is uniform:
// a load from the constant address space is a scalar load.
__device__ __forceinline__ v2u record_words(const ClipRecord *rec) {
  typedef const v2u __attribute__((address_space(4))) * cptr;
  return *(cptr)(reinterpret_cast<uintptr_t>(rec) + 16u);
}

// skip ? kept : made, word by word (v_cndmask): never an arithmetic instruction
__device__ __forceinline__ v4f pick(bool skip, v4f kept, v4f made) {
  const v4u k = __builtin_bit_cast(v4u, kept), m = __builtin_bit_cast(v4u, made);
  v4u o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = skip ? k[j] : m[j];
  return __builtin_bit_cast(v4f, o);
}

__device__ __forceinline__ float pick(bool skip, float kept, float made) {
  return __uint_as_float(skip ? __float_as_uint(kept) : __float_as_uint(made));
}

// task_barrier_tail_elem with the records: elements [a.tail_lo, a.tail_hi),
// one per lane.  Nothing at or past a.tail_hi is read or written.
template <bool MOM, bool BMOM, bool WD, bool KEEP>
__device__ __forceinline__ void task_barrier_clipped_tail_elem(const TaskBarrierArgs &a, const ClipRecordPtrs &rec) {
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
    v2u sf[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool step = ((a.step_mask >> (c + r)) & 1ull) != 0;
        x[r] = reinterpret_cast<const float *>(step ? a.w[c + r] : a.s[c + r])[i];
        y[r] = reinterpret_cast<const float *>(step ? a.g[c + r] : a.w[c + r])[i];
        if constexpr (MOM) {
          if (step) l[r] = reinterpret_cast<const float *>(a.last[c + r])[i];
        }
        sf[r] = record_words(rec.p[c + r]);  // a joining replica's entry is a valid record too
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool step = ((a.step_mask >> (c + r)) & 1ull) != 0;
        const float sv = x[r];
        float wn;
        if (step) {
          const bool skip = (sf[r][1] & kClipSkipped) != 0u;
          const float rate = a.rate[c + r];
          float gv = __uint_as_float(sf[r][0]) * y[r];
          if constexpr (WD) gv = fmaf(a.wd, sv, gv);  // sma.cu:24-31
          if constexpr (MOM) {
            gv = rate * gv;                    // :52-56
            gv = fmaf(a.momentum, l[r], gv);   // :59-64
            reinterpret_cast<float *>(a.last[c + r])[i] = pick(skip, l[r], gv);  // :68
            wn = fmaf(1.0f, gv, sv);           // :74
          } else {
            wn = fmaf(rate, gv, sv);  // :90
          }
          wn = pick(skip, sv, wn);
          if constexpr (KEEP) {
            reinterpret_cast<float *>(a.s[c + r])[i] = sv;  // :71 / :87
            reinterpret_cast<float *>(a.g[c + r])[i] = pick(skip, y[r], gv);
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

// The template parameters are task_barrier_kernel's.  rec.p[k]: the record of
// participating replica k; an entry whose replica only joins is loaded and not
// used, so it holds some valid record as well (launch_task_barrier_clipped).
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_clipped_kernel(const TaskBarrierArgs a, const ClipRecordPtrs rec) {
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_barrier_clipped_tail_elem<MOM, BMOM, WD, KEEP>(a, rec);
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
      v2u sf[RR];
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
      // The chunk's records, together and behind its float4 loads: no load waits
      // for another, and none is waited for ahead of the streams.
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        sf[r] = record_words(rec.p[c + r]);
      }
      // every load of the chunk in flight before the first use (task_barrier_kernel)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        const bool step = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
        const v4f rate = a.rate[c + r];
        const v4f scale = __uint_as_float(sf[r][0]);
        const bool skip = (sf[r][1] & kClipSkipped) != 0u;  // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          v4f sv = x[u][r], wn;
          if (step) {
            v4f gv = scale * y[u][r];
            if constexpr (WD) gv = vfma(wd, sv, gv);
            if constexpr (MOM) {
              gv = rate * gv;
              gv = vfma(mu, l[u][r], gv);
              sto<P>(a.last[c + r], i, pick(skip, l[u][r], gv));
              wn = vfma(one, gv, sv);
            } else {
              wn = vfma(rate, gv, sv);
            }
            wn = pick(skip, sv, wn);
            if constexpr (KEEP) {
              sto<P>(a.s[c + r], i, sv);
              sto<P>(a.g[c + r], i, pick(skip, y[u][r], gv));
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
hipError_t tbc_u(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, const LaunchConfig &cfg0, hipStream_t s,
                 Timing t) {
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
  const int writes = 1 + (BMOM ? 1 : 0) + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 2 : 0)) + joins;
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {
    if constexpr (P != 1) {
      return hipErrorInvalidValue;
    } else {
      if (cfg.unroll != 1) return hipErrorInvalidValue;
      TaskBarrierArgs b = a;
      b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
      g.x += (unsigned)b.tail_blocks;
      hipExtLaunchKernelGGL((task_barrier_clipped_kernel<R, MIXED, MOM, BMOM, WD, KEEP, 1, true, 1>), g,
                            dim3(cfg.block), lds, s, t.start, t.stop, 0, b, rec);
      return hipGetLastError();
    }
  }
  // Base momentum beside stepping replicas that have none: a context has
  // base->last iff its replicas were made with momentum, so only the seam
  // reaches this form, at policy 1 and unroll 1 (a caller-owned buffer of whole
  // chunks has no tail).
  constexpr bool kSeamOnly = MIXED && !MOM && BMOM;
  if constexpr (kSeamOnly && P != 1) {
    return hipErrorInvalidValue;
  } else {
    if (cfg.unroll == 2) {
      if constexpr (kSeamOnly) return hipErrorInvalidValue;
      else
        hipExtLaunchKernelGGL((task_barrier_clipped_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 2>), g,
                              dim3(cfg.block), lds, s, t.start, t.stop, 0, a, rec);
    } else if (cfg.unroll == 1) {
      hipExtLaunchKernelGGL((task_barrier_clipped_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, false, 1>), g,
                            dim3(cfg.block), lds, s, t.start, t.stop, 0, a, rec);
    } else {
      return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
}

// The ladders below are launch_task_barrier's (task_barrier_kernels.hip).
template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tbc_all(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, const LaunchConfig &cfg, hipStream_t s,
                   Timing t) {
  switch (a.nrep) {
    case 1: return tbc_u<1, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 2: return tbc_u<2, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 3: return tbc_u<3, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 4: return tbc_u<4, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 5: return tbc_u<5, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 6: return tbc_u<6, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 7: return tbc_u<7, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    case 8: return tbc_u<8, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
    default: return tbc_u<-1, false, MOM, MOM, WD, KEEP, P>(a, rec, cfg, s, t);
  }
}

template <bool MOM, bool WD, bool KEEP, int P>
hipError_t tbc_form(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool bmom, const LaunchConfig &cfg,
                    hipStream_t s, Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  if (a.step_mask == all && bmom == MOM) return tbc_all<MOM, WD, KEEP, P>(a, rec, cfg, s, t);
  return bmom ? tbc_u<-1, true, MOM, true, WD, KEEP, P>(a, rec, cfg, s, t)
              : tbc_u<-1, true, MOM, false, WD, KEEP, P>(a, rec, cfg, s, t);
}

template <bool KEEP, int P>
hipError_t tbc_conf(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool bmom, const LaunchConfig &cfg,
                    hipStream_t s, Timing t) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom)
    return wd ? tbc_form<true, true, KEEP, P>(a, rec, bmom, cfg, s, t)
              : tbc_form<true, false, KEEP, P>(a, rec, bmom, cfg, s, t);
  return wd ? tbc_form<false, true, KEEP, P>(a, rec, bmom, cfg, s, t)
            : tbc_form<false, false, KEEP, P>(a, rec, bmom, cfg, s, t);
}

}  // namespace

hipError_t launch_task_barrier_clipped(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, bool keep_task_outputs,
                                       const LaunchConfig &cfg, hipStream_t stream, Timing t) {
  if (a.nrep < 1 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  // No record pointer is followed that the caller did not give: every stepping
  // replica has one, and a launch without a stepping replica has nothing to
  // clip (launch_task_barrier runs it).  The entries of the replicas that only
  // join are loaded and not used: they take the first stepping replica's.
  if (a.step_mask == 0) return hipErrorInvalidValue;
  ClipRecordPtrs full;
  const ClipRecord *any = nullptr;
  for (int k = 0; k < a.nrep; ++k) {
    if (((a.step_mask >> k) & 1ull) == 0) continue;
    if (!rec.p[k] || (reinterpret_cast<uintptr_t>(rec.p[k]) & 7u) != 0) return hipErrorInvalidValue;
    if (!any) any = rec.p[k];
  }
  for (int k = 0; k < kMaxReplicas; ++k)
    full.p[k] = (k < a.nrep && ((a.step_mask >> k) & 1ull) != 0) ? rec.p[k] : any;
  const bool bmom = a.blast != nullptr;
  if (cfg.policy == 1)
    return keep_task_outputs ? tbc_conf<true, 1>(a, full, bmom, cfg, stream, t)
                             : tbc_conf<false, 1>(a, full, bmom, cfg, stream, t);
  return keep_task_outputs ? tbc_conf<true, 0>(a, full, bmom, cfg, stream, t)
                           : tbc_conf<false, 0>(a, full, bmom, cfg, stream, t);
}

}  // namespace cbx
