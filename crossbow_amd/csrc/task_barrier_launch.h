// task_barrier_launch.h -- the host side the four fused task-step barrier
// launches share (launch_task_barrier, launch_task_barrier_variables,
// launch_task_barrier_clipped, launch_task_barrier_clipped_variables): the
// launch check, the grid, the ladders from the run-time arguments to one kernel
// instantiation, and the checks of the tables and the records.
//
// Each object gives a launcher L:
//   L::Step                         its step policy (task_barrier_step.h)
//   L::kSideObject                  a shared object beside the library: only what a door reaches is compiled there,
//                                   the context's forms (no tail, unroll 1 or 2, either policy) and the seam's (a
//                                   tail, unroll 1, nontemporal); the library itself compiles every form
//   L::seam_only<MIXED, MOM, BMOM, WD>()
//                                   a form that only the seam reaches, at policy 1 and unroll 1
//   l.launch<R, ..., TAIL, U>(grid, block, lds, stream, timing, args)
//                                   hipExtLaunchKernelGGL of its kernel, with its own parameters beside `args`
// Any shape that is not compiled is hipErrorInvalidValue, before the launch.
#pragma once

#include "clip_internal.h"
#include "optimise_plan.h"
#include "sma_internal.h"
#include "stream_helpers.h"

namespace cbx {

static_assert(kMaxReplicas <= 64, "step_mask holds one bit per replica");

// The per-variable launches: no table is read past its end.  One entry per
// 256-float chunk of the bulk, and every tail float has a variable.
inline bool task_barrier_tables_cover(const TaskBarrierArgs &a, const VarTables &vt) {
  if (!vt.chunks || !vt.bounds || !vt.mult || vt.nvars == 0 || a.n4 < 0 || a.tail_lo < 0) return false;
  const uint64_t nchunks = ((uint64_t)vt.elements + kOptChunk - 1) / kOptChunk;
  if ((uint64_t)a.n4 * 4u > nchunks * kOptChunk) return false;
  if (a.tail_hi > a.tail_lo && a.tail_hi > (int64_t)vt.elements) return false;
  return true;
}

// The clipped launches: no record pointer is followed that the caller did not
// give.  Every stepping replica has one, 8-byte aligned (record_words), and a
// launch without a stepping replica has nothing to clip (launch_task_barrier
// runs it).  The entries of the replicas that only join are loaded and not
// used: in `full` they take the first stepping replica's.
inline bool task_barrier_fill_records(const TaskBarrierArgs &a, const ClipRecordPtrs &rec, ClipRecordPtrs &full) {
  if (a.nrep < 1 || a.nrep > kMaxReplicas) return false;
  if (a.step_mask == 0) return false;
  const ClipRecord *any = nullptr;
  for (int k = 0; k < a.nrep; ++k) {
    if (((a.step_mask >> k) & 1ull) == 0) continue;
    if (!rec.p[k] || (reinterpret_cast<uintptr_t>(rec.p[k]) & 7u) != 0) return false;
    if (!any) any = rec.p[k];
  }
  for (int k = 0; k < kMaxReplicas; ++k)
    full.p[k] = (k < a.nrep && ((a.step_mask >> k) & 1ull) != 0) ? rec.p[k] : any;
  return true;
}

template <class L, bool MIXED, bool MOM, bool BMOM, bool WD, int P, bool TAIL, int U>
constexpr bool task_barrier_compiled() {
  if (TAIL && P != 1) return false;  // the tail rides the nontemporal policy only
  if (!L::kSideObject) return true;
  if (TAIL) return U == 1;
  return !L::template seam_only<MIXED, MOM, BMOM, WD>() || (P == 1 && U == 1);
}

template <class L, int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
hipError_t tb_go(const L &l, const TaskBarrierArgs &a, dim3 g, int block, unsigned lds, hipStream_t s, Timing t) {
  if constexpr (task_barrier_compiled<L, MIXED, MOM, BMOM, WD, P, TAIL, U>()) {
    l.template launch<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>(g, dim3(block), lds, s, t, a);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <class L, int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P>
hipError_t tb_u(const L &l, const TaskBarrierArgs &a, const LaunchConfig &cfg0, hipStream_t s, Timing t) {
  const LaunchConfig cfg = small_launch_shape(cfg0, a.n4);
  const bool tail = a.tail_hi > a.tail_lo;
  // Every wave's chunk (64 lanes x unroll float4s, first_elem) is whole, so no
  // bounds check sits in the kernel's loop.  The context's padded buffers are
  // whole kPadFloat4s; the bulk of a caller-owned buffer is whole chunks only
  // (e.g. 1,280 float4s), and may be empty when a tail is all there is.  The
  // check stands in front of the context's launches too: the arena's whole
  // kPadFloat4s and the setter's shapes always pass it.
  if (cfg.block <= 0 || cfg.block % 64 != 0 || (L::kSideObject && cfg.block > 256) || cfg.unroll < 1 || a.n4 < 0 ||
      a.n4 % (64ll * cfg.unroll) != 0 || (a.n4 == 0 && !tail))
    return hipErrorInvalidValue;
  dim3 g = a.n4 > 0 ? grid_for(a.n4, cfg) : dim3(0);
  // Buffer streams per lane: a stepping replica reads w, g (, last_i) and
  // writes w (, last_i) (, s, g; a clipped step keeps g always); one that only
  // joins reads s, w and writes w.
  int steps = 0;
  for (int r = 0; r < a.nrep; ++r) steps += (int)((a.step_mask >> r) & 1ull);
  const int joins = a.nrep - steps;
  constexpr bool kKeepsG = MOM || WD || L::Step::kClips;
  const int reads = 1 + (BMOM ? 1 : 0) + steps * (2 + (MOM ? 1 : 0)) + joins * 2;
  const int writes = 1 + (BMOM ? 1 : 0) + steps * (1 + (MOM ? 1 : 0) + (KEEP ? 1 + (kKeepsG ? 1 : 0) : 0)) + joins;
  // the cap is sized by the bulk's grid: the few tail workgroups are not counted
  const unsigned lds = lds_for_occupancy(cfg, reads, writes, g.x);
  if (tail) {  // caller-owned buffers: the tail rides the same launch, in front
    TaskBarrierArgs b = a;
    b.tail_blocks = (int)((b.tail_hi - b.tail_lo + cfg.block - 1) / cfg.block);
    g.x += (unsigned)b.tail_blocks;
    if (cfg.unroll == 2) return tb_go<L, R, MIXED, MOM, BMOM, WD, KEEP, P, true, 2>(l, b, g, cfg.block, lds, s, t);
    if (cfg.unroll == 1) return tb_go<L, R, MIXED, MOM, BMOM, WD, KEEP, P, true, 1>(l, b, g, cfg.block, lds, s, t);
    return hipErrorInvalidValue;
  }
  if (cfg.unroll == 2) return tb_go<L, R, MIXED, MOM, BMOM, WD, KEEP, P, false, 2>(l, a, g, cfg.block, lds, s, t);
  if (cfg.unroll == 1) return tb_go<L, R, MIXED, MOM, BMOM, WD, KEEP, P, false, 1>(l, a, g, cfg.block, lds, s, t);
  return hipErrorInvalidValue;
}

template <class L, bool MOM, bool WD, bool KEEP, int P>
hipError_t tb_form(const L &l, const TaskBarrierArgs &a, bool bmom, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const uint64_t all = a.nrep >= 64 ? ~0ull : ((1ull << a.nrep) - 1ull);
  // Every participating replica steps, with the base model's momentum on iff
  // theirs is (what the setters produce): the BSP case, unrolled for R <= kChunk.
  if (a.nrep > 0 && a.step_mask == all && bmom == MOM) {
    switch (a.nrep) {
      case 1: return tb_u<L, 1, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 2: return tb_u<L, 2, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 3: return tb_u<L, 3, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 4: return tb_u<L, 4, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 5: return tb_u<L, 5, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 6: return tb_u<L, 6, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 7: return tb_u<L, 7, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      case 8: return tb_u<L, 8, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
      default: return tb_u<L, -1, false, MOM, MOM, WD, KEEP, P>(l, a, cfg, s, t);
    }
  }
  // Anything else (some replicas only join, no replica at all, base and replica
  // momentum that differ): the runtime-chunked form with a branch per replica.
  return bmom ? tb_u<L, -1, true, MOM, true, WD, KEEP, P>(l, a, cfg, s, t)
              : tb_u<L, -1, true, MOM, false, WD, KEEP, P>(l, a, cfg, s, t);
}

template <class L, bool KEEP, int P>
hipError_t tb_conf(const L &l, const TaskBarrierArgs &a, const LaunchConfig &cfg, hipStream_t s, Timing t) {
  const bool bmom = a.blast != nullptr, mom = a.momentum > 0.0f, wd = a.wd > 0.0f;
  if (mom)
    return wd ? tb_form<L, true, true, KEEP, P>(l, a, bmom, cfg, s, t) : tb_form<L, true, false, KEEP, P>(l, a, bmom, cfg, s, t);
  return wd ? tb_form<L, false, true, KEEP, P>(l, a, bmom, cfg, s, t) : tb_form<L, false, false, KEEP, P>(l, a, bmom, cfg, s, t);
}

// The launch of object L, its own arguments (tables, records) checked by the caller.
template <class L>
hipError_t task_barrier_launch(const L &l, const TaskBarrierArgs &a, bool keep_task_outputs, const LaunchConfig &cfg,
                               hipStream_t s, Timing t) {
  if (a.nrep < 0 || a.nrep > kMaxReplicas) return hipErrorInvalidValue;
  if (a.nrep < 64 && (a.step_mask >> a.nrep) != 0) return hipErrorInvalidValue;
  if (cfg.policy == 1)
    return keep_task_outputs ? tb_conf<L, true, 1>(l, a, cfg, s, t) : tb_conf<L, false, 1>(l, a, cfg, s, t);
  return keep_task_outputs ? tb_conf<L, true, 0>(l, a, cfg, s, t) : tb_conf<L, false, 0>(l, a, cfg, s, t);
}

}  // namespace cbx
