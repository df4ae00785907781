// stats_plan.h -- the piece table of the model-statistics reduction
// (stats_kernels.hip, cbx_model_stats).  Plain C++, no HIP: the builder is
// tested on the CPU (tests/native/stats_plan_test.cpp).
//
// A model buffer is a run of variables whose offsets are a running sum
// (ModelDef::offset, model.c:127-157), not multiples of 16 bytes, so a float4
// may straddle two variables.  The buffer is cut into fixed tiles of
// kStatsTile floats, every tile at the variable boundaries inside it, and
// every such segment into at most three pieces: the floats up to the next
// 16-byte boundary, whole float4s, and the floats after the last one.  A
// piece so lies in one variable and one tile; an aligned piece starts on a
// 16-byte boundary and holds whole float4s (the kernel's float4 path), every
// other piece has at most 3 floats (the masked scalar path), except where a
// segment holds no whole float4 at all.  Pieces are in offset order, so the
// pieces of variable v are pieces[var_first[v] .. var_first[v + 1]).
#pragma once

#include <cstdint>
#include <vector>

namespace cbx {

// Floats per tile: 16 KiB of every buffer, 16 float4 trips of one wave.
constexpr uint32_t kStatsTile = 4096;
// One-wave workgroups each walk about this many pieces (at most kStatsMaxGrid
// workgroups): a fixed function of the piece count, never a tunable.
constexpr uint32_t kStatsPiecesPerGroup = 3;
constexpr uint32_t kStatsMaxGrid = 16384;

struct StatsPiece {
  uint32_t lo, hi;   // floats [lo, hi) of the buffer
  uint32_t var;      // the variable they belong to
  uint32_t aligned;  // 1: lo and hi are multiples of 4 (float4 path)
};

struct StatsPlan {
  std::vector<StatsPiece> pieces;
  std::vector<uint32_t> var_first;  // nvars + 1 entries
  int64_t elements = 0;
};

inline uint32_t stats_grid(size_t npieces) {
  size_t g = (npieces + kStatsPiecesPerGroup - 1) / kStatsPiecesPerGroup;
  if (g < 1) g = 1;
  return (uint32_t)(g > kStatsMaxGrid ? kStatsMaxGrid : g);
}

// var_elements[0 .. nvars): floats per variable, in offset order; they must
// sum to `elements`.  nvars == 0 (or var_elements == nullptr) is one variable
// of `elements` floats.  False on negative counts, a wrong sum, or more than
// 2^32 - 1 bytes per buffer (the kernels use 32-bit byte offsets).
inline bool build_stats_plan(const long long *var_elements, int nvars, long long elements, StatsPlan *out) {
  out->pieces.clear();
  out->var_first.clear();
  out->elements = 0;
  if (elements <= 0 || elements > (long long)(0xffffffffull / 4)) return false;
  const long long one[1] = {elements};
  if (nvars <= 0 || var_elements == nullptr) {
    var_elements = one;
    nvars = 1;
  }
  long long sum = 0;
  for (int v = 0; v < nvars; ++v) {
    if (var_elements[v] < 0 || var_elements[v] > elements) return false;
    sum += var_elements[v];
  }
  if (sum != elements) return false;
  auto push = [out](uint64_t lo, uint64_t hi, int v, bool aligned) {
    if (lo < hi) out->pieces.push_back(StatsPiece{(uint32_t)lo, (uint32_t)hi, (uint32_t)v, aligned ? 1u : 0u});
  };
  uint64_t vlo = 0;
  for (int v = 0; v < nvars; ++v) {
    out->var_first.push_back((uint32_t)out->pieces.size());
    const uint64_t vhi = vlo + (uint64_t)var_elements[v];
    for (uint64_t a = vlo; a < vhi;) {
      const uint64_t tile_end = (a / kStatsTile + 1) * kStatsTile;
      const uint64_t b = tile_end < vhi ? tile_end : vhi;
      const uint64_t a4 = (a + 3) / 4 * 4, b4 = b / 4 * 4;
      if (a4 < b4) {
        push(a, a4, v, false);
        push(a4, b4, v, true);
        push(b4, b, v, false);
      } else {
        push(a, b, v, false);
      }
      a = b;
    }
    vlo = vhi;
  }
  out->var_first.push_back((uint32_t)out->pieces.size());
  out->elements = elements;
  return true;
}

}  // namespace cbx
