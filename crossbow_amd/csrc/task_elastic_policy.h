// task_elastic_policy.h -- what the three fused task-step elastic-averaging
// kernels with a step policy share beside their body
// (task_elastic_policy_body.inc): the element-wise tail, and the host side from
// the run-time arguments to one kernel instantiation
// (launch_task_elastic_variables, launch_task_elastic_clipped,
// launch_task_elastic_clipped_variables).  The policies are
// task_barrier_step.h's VariablesStep, ClippedStep and ClippedVariablesStep; the
// plain step is task_elastic_kernels.hip, an object of its own that this text
// does not touch.
//
// Each compilation unit gives a launcher L:
//   L::Step                         its step policy
//   l.launch<R, ..., TAIL, U>(grid, block, lds, stream, timing, args)
//                                   hipExtLaunchKernelGGL of its kernel, with its own parameters beside `args`
// Only what a door reaches is compiled (hipErrorInvalidValue otherwise, before
// the launch): the tail rides the nontemporal policy at unroll 1, the seam's
// shape; without one, unroll 1 or 2 at either policy.
#pragma once

#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {

// Buffers the caller owns (the sma.c seam, sma_seam.hip) hold exactly n
// floats.  Their last elements [a.tail_lo, a.tail_hi) go to the first
// a.tail_blocks workgroups of the same launch (TAIL instantiations), one float
// per lane with its own multiplier, as in task_elastic_tail_elem and
// task_barrier_tail_elem: the fp32 sequence per element, the per-replica choice
// by a.step_mask (set for every replica in the all-step forms too) and the
// chunked replica walk are those of the float4 path.  Nothing at or past
// a.tail_hi is read (the chunk entry of float i < elements exists), nothing
// outside the range is written.
template <bool MOM, bool WD, bool KEEP, class STEP>
__device__ __forceinline__ void task_elastic_policy_tail_elem(const TaskBarrierArgs &a, const STEP &step) {
  const int64_t i = a.tail_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.tail_hi) return;
  [[maybe_unused]] float m;  // the float's own multiplier
  if constexpr (STEP::kPerVariable) {
    const uint32_t en = step.chunks[(uint32_t)i / kOptChunk];
    m = step.mult[(en & 1u) ? variable_of(step.bounds, step.nvars, en >> 1, (uint32_t)i) : (en >> 1)];
  }
  float *z = reinterpret_cast<float *>(a.z);
  const float z0 = z[i];
  float acc = 0.0f;  // synchronouseamsgd.c:43
  for (int c = 0; c < a.nrep; c += kChunk) {
    float x[kChunk];
    [[maybe_unused]] float y[kChunk], l[kChunk];
    [[maybe_unused]] v2u sf[kChunk];
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
        if constexpr (STEP::kClips) sf[r] = record_words(step.rec.p[c + r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      if (c + r < a.nrep) {
        const bool stepping = ((a.step_mask >> (c + r)) & 1ull) != 0;
        float wn = x[r];
        if (stepping) {
          [[maybe_unused]] bool skip = false;
          if constexpr (STEP::kClips) skip = (sf[r][1] & kClipSkipped) != 0u;
          float rate = a.rate[c + r];
          if constexpr (STEP::kPerVariable) rate = a.rate[c + r] * m;  // model.c:159-177
          float gv = y[r];
          if constexpr (STEP::kClips) gv = __uint_as_float(sf[r][0]) * y[r];
          if constexpr (WD) gv = fmaf(a.wd, x[r], gv);  // sma.cu:24-31
          if constexpr (MOM) {
            gv = rate * gv;                   // :52-56
            gv = fmaf(a.momentum, l[r], gv);  // :59-64
            float ln = gv;                    // :68
            if constexpr (STEP::kClips) ln = pick(skip, l[r], gv);
            reinterpret_cast<float *>(a.last[c + r])[i] = ln;
            wn = fmaf(1.0f, gv, x[r]);  // :74
          } else {
            wn = fmaf(rate, gv, x[r]);  // :90
          }
          if constexpr (STEP::kClips) wn = pick(skip, x[r], wn);
          if constexpr (KEEP) {
            reinterpret_cast<float *>(a.s[c + r])[i] = x[r];  // :71 / :87
            if constexpr (STEP::kClips) reinterpret_cast<float *>(a.g[c + r])[i] = pick(skip, y[r], gv);
            else if constexpr (MOM || WD) reinterpret_cast<float *>(a.g[c + r])[i] = gv;
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

template <int P, bool TAIL, int U>
constexpr bool task_elastic_policy_compiled() {
  return TAIL ? (P == 1 && U == 1) : true;
}

template <class L, int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P, bool TAIL, int U>
hipError_t tep_go(const L &l, const TaskBarrierArgs &a, dim3 g, int block, unsigned lds, hipStream_t s, Timing t) {
  if constexpr (task_elastic_policy_compiled<P, TAIL, U>()) {
    l.template launch<R, MIXED, MOM, WD, KEEP, P, TAIL, U>(g, dim3(block), lds, s, t, a);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <class L, int R, bool MIXED, bool MOM, bool WD, bool KEEP, int P>
hipError_t tep_u(const L &l, const TaskBarrierArgs &a, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop (te_u, task_elastic_kernels.hip).
  if (cfg.block <= 0 || cfg.block % 64 != 0 || cfg.block > 256 || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane: z is read and written; a stepping replica reads w,
  // g (, last_i) and writes w (, last_i) (, s, and g where the step changes it:
  // a clipped step keeps g always); one that only joins reads w and writes w.
  int steps = 0;
  for (int r = 0; r < a.nrep; ++r) steps += (int)((a.step_mask >> r) & 1ull);
  const int joins = a.nrep - steps;
  constexpr bool kKeepsG = MOM || WD || L::Step::kClips;
  const int reads = 1 + steps * (2 + (MOM ? 1 : 0)) + joins;
  const int writes = 1 + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 1 + (kKeepsG ? 1 : 0) : 0)) + joins;
  // the cap is sized by the bulk's grid: the few tail workgroups are not counted
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    TaskBarrierArgs b = a;
    b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
    g.x += (unsigned)b.tail_blocks;
    if (cfg.unroll == 1) return tep_go<L, R, MIXED, MOM, WD, KEEP, P, true, 1>(l, b, g, cfg.block, lds, s, t);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return tep_go<L, R, MIXED, MOM, WD, KEEP, P, false, 2>(l, a, g, cfg.block, lds, s, t);
  if (cfg.unroll == 1) return tep_go<L, R, MIXED, MOM, WD, KEEP, P, false, 1>(l, a, g, cfg.block, lds, s, t);
  return hipErrorInvalidValue;
}

// te_form's ladder (task_elastic_kernels.hip): the unrolled path whenever every
// participating replica steps.
template <class L, bool MOM, bool WD, bool KEEP, int P>
hipError_t tep_form(const L &l, const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  if (a.nrep > 0 && a.step_mask == all) {
    switch (a.nrep) {
      case 1: return tep_u<L, 1, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 2: return tep_u<L, 2, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 3: return tep_u<L, 3, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 4: return tep_u<L, 4, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 5: return tep_u<L, 5, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 6: return tep_u<L, 6, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 7: return tep_u<L, 7, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 8: return tep_u<L, 8, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      default: return tep_u<L, -1, false, MOM, WD, KEEP, P>(l, a, cfg, s, t);
    }
  }
  // Some replicas only join, nobody steps, or nobody is there at all: the
  // runtime-chunked form with a choice per replica.
  return tep_u<L, -1, true, MOM, WD, KEEP, P>(l, a, cfg, s, t);
}

template <class L, bool KEEP, int P>
hipError_t tep_conf(const L &l, const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const bool mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom) return wd ? tep_form<L, true, true, KEEP, P>(l, a, cfg, s, t) : tep_form<L, true, false, KEEP, P>(l, a, cfg, s, t);
  return wd ? tep_form<L, false, true, KEEP, P>(l, a, cfg, s, t) : tep_form<L, false, false, KEEP, P>(l, a, cfg, s, t);
}

// The launch of launcher L, its own arguments (tables, records) checked by the
// caller; the checks of TaskBarrierArgs are launch_task_elastic's.
template <class L>
hipError_t task_elastic_policy_launch(const L &l, const TaskBarrierArgs &a, bool keep_task_outputs,
                                      const LaunchConfig &cfg, hipStream_t s, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  if (a.step_mask == 0 && (a.momentum > 0.0f || a.wd > 0.0f)) return hipErrorInvalidValue;  // nobody's to be
  if (cfg.policy == 1)
    return keep_task_outputs ? tep_conf<L, true, 1>(l, a, cfg, s, t) : tep_conf<L, false, 1>(l, a, cfg, s, t);
  return keep_task_outputs ? tep_conf<L, true, 0>(l, a, cfg, s, t) : tep_conf<L, false, 0>(l, a, cfg, s, t);
}

}  // namespace cbx
