// The piece-table builder of the model-statistics reduction
// (crossbow_amd/csrc/stats_plan.h) on the CPU, under ASan + UBSan
// (tests/test_stats_abi.py builds and runs it).  For each case: the pieces
// tile [0, n) exactly once and in order, no piece crosses a variable or a
// tile boundary, an aligned piece starts and ends on 16 bytes, every other
// piece is short, and var_first brackets each variable's pieces.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stats_plan.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static size_t check_case(const std::vector<long long> &vars, long long n) {
  cbx::StatsPlan plan;
  CHECK(cbx::build_stats_plan(vars.empty() ? nullptr : vars.data(), (int)vars.size(), n, &plan));
  const std::vector<long long> one = {n};
  const std::vector<long long> &vs = vars.empty() ? one : vars;
  CHECK(plan.elements == n);
  CHECK(plan.var_first.size() == vs.size() + 1);
  CHECK(plan.var_first.front() == 0);
  CHECK(plan.var_first.back() == plan.pieces.size());
  std::vector<int> covered((size_t)n, 0);
  std::vector<long long> vlo(vs.size() + 1, 0);
  for (size_t v = 0; v < vs.size(); ++v) vlo[v + 1] = vlo[v] + vs[v];
  unsigned long long at = 0;
  for (size_t p = 0; p < plan.pieces.size(); ++p) {
    const cbx::StatsPiece &pc = plan.pieces[p];
    CHECK(pc.lo < pc.hi);
    CHECK(pc.lo == at);  // in order, no gap, no overlap
    CHECK(pc.hi <= (unsigned long long)n);
    at = pc.hi;
    for (unsigned i = pc.lo; i < pc.hi; ++i) covered[i]++;
    CHECK(pc.var < vs.size());
    CHECK((long long)pc.lo >= vlo[pc.var] && (long long)pc.hi <= vlo[pc.var + 1]);  // one variable
    CHECK(pc.lo / cbx::kStatsTile == (pc.hi - 1) / cbx::kStatsTile);               // one tile
    CHECK(p >= plan.var_first[pc.var] && p < plan.var_first[pc.var + 1]);
    if (pc.aligned) {
      CHECK((pc.lo * 4ull) % 16 == 0 && (pc.hi * 4ull) % 16 == 0);
    } else {
      CHECK(pc.hi - pc.lo <= 6);  // under two float4s: no whole aligned one inside
      CHECK(pc.aligned == 0);
    }
  }
  CHECK(at == (unsigned long long)n);
  for (long long i = 0; i < n; ++i) CHECK(covered[(size_t)i] == 1);
  CHECK(cbx::stats_grid(plan.pieces.size()) >= 1);
  CHECK((size_t)cbx::stats_grid(plan.pieces.size()) * cbx::kStatsPiecesPerGroup >= plan.pieces.size() ||
        cbx::stats_grid(plan.pieces.size()) == cbx::kStatsMaxGrid);
  return plan.pieces.size();
}

int main() {
  size_t pieces = 0;
  pieces += check_case({1, 3, 35, 4093, 4096, 1000}, 9228);  // boundaries at 1, 4, 39, 4132, 8228
  pieces += check_case({}, 1);
  pieces += check_case({1}, 1);
  // a variable list that does not sum to n, a negative count, no elements
  cbx::StatsPlan plan;
  const long long bad[2] = {5, 6};
  CHECK(!cbx::build_stats_plan(bad, 2, 12, &plan));
  const long long neg[2] = {-1, 13};
  CHECK(!cbx::build_stats_plan(neg, 2, 12, &plan));
  CHECK(!cbx::build_stats_plan(nullptr, 0, 0, &plan));
  CHECK(!cbx::build_stats_plan(nullptr, 0, 1ll << 30, &plan));  // 2^32 bytes: past the 32-bit offsets
  std::printf("ok %zu pieces\n", pieces);
  return 0;
}
