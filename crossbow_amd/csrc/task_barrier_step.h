// task_barrier_step.h -- what the four fused task-step barrier kernels differ
// in (task_barrier_kernels.hip, task_barrier_variables_kernels.hip,
// task_barrier_clipped_kernels.hip, task_barrier_clipped_variables_kernels.hip),
// and the element-wise tail they share.  Device code only; the bulk of the
// kernels is task_barrier_body.inc.
//
// A step policy is a mode's two constants and the kernel parameters it has
// beside TaskBarrierArgs.  The shared text reads a policy's members only under
// `if constexpr` on its constants, so an instantiation holds nothing of a mode
// it is not.  The kernel that is both (a learning rate per variable and
// clipped) is the fourth policy, with both constants set and both sets of
// members.
#pragma once

#include <cstddef>

#include "clip_internal.h"
#include "optimise_plan.h"
#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {

// Plain: replica i steps with a.rate[i] (sma.cu:3-100).
struct PlainStep {
  static constexpr bool kPerVariable = false, kClips = false;
};

// A learning rate per variable: r_iv = a.rate[i] * mult[v], one fp32 multiply
// (model.c:159-177).  The tables of optimise_plan.h over at least a.n4 * 4
// floats (and a.tail_hi); they are kernel parameters of their own,
// `const __restrict__`, so the entry and the multiplier of a uniform chunk
// arrive through scalar loads.
struct VariablesStep {
  static constexpr bool kPerVariable = true, kClips = false;
  const uint32_t *__restrict__ chunks;
  const uint32_t *__restrict__ bounds;
  const float *__restrict__ mult;
  uint32_t nvars;
};

// Clipped by global L2 norm: g = scale_i * g, one fp32 multiply before weight
// decay; a kept g_i is always written; with the record's skip bit the step is
// s = w and nothing else.  rec.p[k]: the record of participating replica k; an
// entry whose replica only joins is loaded and not used, so it holds some valid
// record as well (launch_task_barrier_clipped).
struct ClippedStep {
  static constexpr bool kPerVariable = false, kClips = true;
  const ClipRecordPtrs &rec;
};

// Both: g = scale_i * g before weight decay, then the step with r_iv = a.rate[i]
// * mult[v]; the skip and the kept g are ClippedStep's
// (launch_sma_optimise_variables_clipped per replica, clip_internal.h).
struct ClippedVariablesStep {
  static constexpr bool kPerVariable = true, kClips = true;
  const uint32_t *__restrict__ chunks;
  const uint32_t *__restrict__ bounds;
  const float *__restrict__ mult;
  uint32_t nvars;
  const ClipRecordPtrs &rec;
};

// The policy S, named through a template parameter of the kernel: `if
// constexpr` discards a statement unchecked only where its condition depends
// on one.
template <class S, int>
struct step_policy {
  typedef S type;
};

static_assert(offsetof(ClipRecord, scale) == 16 && offsetof(ClipRecord, flags) == 20,
              "scale and flags are fetched by one 8-byte load at byte 16");

typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// {scale's bits, flags} of one record.  The record was written by an earlier
// kernel on the stream and is not written here, and its address is uniform:
// a load from the constant address space is a scalar load.
__device__ __forceinline__ v2u record_words(const ClipRecord *rec) {
  typedef const v2u __attribute__((address_space(4))) * cptr;
  return *(cptr)(reinterpret_cast<uintptr_t>(rec) + 16u);
}

// skip ? kept : made, word by word (v_cndmask) on integer views: no arithmetic
// instruction touches a value that has to stay a bit copy (a signalling NaN
// keeps its payload).  The skip is known only on the device, and a branch
// around a replica's loads or stores costs the unrolled chunk its registers
// (DESIGN.md 8f), so every store is issued either way.
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

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane, as in the SMA kernels (sma_tail_elem, sma_kernels.hip): the fp32
// sequence per element, the per-replica choice by a.step_mask (set for every
// replica in the all-step forms too), the chunked replica walk and Phase D are
// those of the float4 path (task_barrier_body.inc).  Nothing at or past
// a.tail_hi is read (the chunk entry of float i < elements exists), nothing
// outside the range is written.
template <bool MOM, bool BMOM, bool WD, bool KEEP, class STEP>
__device__ __forceinline__ void task_barrier_tail_elem(const TaskBarrierArgs &a, const STEP &step) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  [[maybe_unused]] float m;  // the float's own multiplier
  if constexpr (STEP::kPerVariable) {
    const uint32_t en = step.chunks[(uint32_t)i / kOptChunk];
    m = step.mult[(en & 1u) ? variable_of(step.bounds, step.nvars, en >> 1, (uint32_t)i) : (en >> 1)];
  }
  float *z = reinterpret_cast<float *>(a.z);
  float z0 = z[i];
  float l0 = 0.0f;
  if constexpr (BMOM) l0 = reinterpret_cast<const float *>(a.blast)[i];
  float acc = 0.0f;  // sma.c:66
  for (int c = 0; c < a.nrep; c += kChunk) {
    // a stepping replica: x = w, y = g, l = last_i; one that only joins: x = s, y = w
    float x[kChunk], y[kChunk];
    [[maybe_unused]] float l[kChunk];
    [[maybe_unused]] v2u sf[kChunk];
    // every load of a chunk issued before its first store (sma_tail_elem)
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool stepping = ((a.step_mask >> (c + r)) & 1ull) != 0;
        x[r] = reinterpret_cast<const float *>(stepping ? a.w[c + r] : a.s[c + r])[i];
        y[r] = reinterpret_cast<const float *>(stepping ? a.g[c + r] : a.w[c + r])[i];
        if constexpr (MOM) {
          if (stepping) l[r] = reinterpret_cast<const float *>(a.last[c + r])[i];
        }
        if constexpr (STEP::kClips) sf[r] = record_words(step.rec.p[c + r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool stepping = ((a.step_mask >> (c + r)) & 1ull) != 0;
        const float sv = x[r];
        float wn;
        if (stepping) {
          [[maybe_unused]] bool skip = false;
          if constexpr (STEP::kClips) skip = (sf[r][1] & kClipSkipped) != 0u;
          float rate = a.rate[c + r];
          if constexpr (STEP::kPerVariable) rate = a.rate[c + r] * m;  // model.c:159-177
          float gv = y[r];
          if constexpr (STEP::kClips) gv = __uint_as_float(sf[r][0]) * y[r];
          if constexpr (WD) gv = fmaf(a.wd, sv, gv);  // sma.cu:24-31
          if constexpr (MOM) {
            gv = rate * gv;                   // :52-56
            gv = fmaf(a.momentum, l[r], gv);  // :59-64
            float ln = gv;                    // :68
            if constexpr (STEP::kClips) ln = pick(skip, l[r], gv);
            reinterpret_cast<float *>(a.last[c + r])[i] = ln;
            wn = fmaf(1.0f, gv, sv);  // :74
          } else {
            wn = fmaf(rate, gv, sv);  // :90
          }
          if constexpr (STEP::kClips) wn = pick(skip, sv, wn);
          if constexpr (KEEP) {
            reinterpret_cast<float *>(a.s[c + r])[i] = sv;  // :71 / :87
            if constexpr (STEP::kClips) reinterpret_cast<float *>(a.g[c + r])[i] = pick(skip, y[r], gv);
            else if constexpr (MOM || WD) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
          }
        } else {
          wn = y[r];
        }
        const float d = fmaf(-1.0f, z0, sv);                               // sma.c:79-90
        acc = fmaf(a.alpha, d, acc);                                       // :102-107
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

}  // namespace cbx
