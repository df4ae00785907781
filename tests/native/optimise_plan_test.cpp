// The chunk-table builder of the per-variable replica step
// (crossbow_amd/csrc/optimise_plan.h) on the CPU, under ASan + UBSan
// (tests/test_optimise_plan.py builds and runs it).  For each case: the
// variable the kernel's lookup finds for every float (the chunk's entry, and
// in a mixed chunk the search of the boundary array from it) equals a
// brute-force walk over the variables; a chunk is flagged mixed iff a
// boundary between two variables lies strictly inside it; the rejected
// inputs are rejected.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "optimise_plan.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static size_t check_case(const std::vector<long long> &vars) {
  long long n = 0;
  for (long long e : vars) n += e;
  cbx::OptimisePlan plan;
  CHECK(cbx::build_optimise_plan(vars.data(), (int)vars.size(), n, &plan));
  const uint32_t V = (uint32_t)vars.size();
  CHECK(plan.elements == n && plan.nvars == (int)V);
  CHECK(plan.bounds.size() == (size_t)V + 1);
  CHECK(plan.bounds.front() == 0 && plan.bounds.back() == (uint32_t)n);
  CHECK(plan.chunks.size() == (size_t)((n + cbx::kOptChunk - 1) / cbx::kOptChunk));
  // brute force: the variable of every float
  std::vector<uint32_t> owner;
  owner.reserve((size_t)n);
  for (uint32_t v = 0; v < V; ++v) {
    CHECK(plan.bounds[v + 1] - plan.bounds[v] == (uint32_t)vars[v]);
    for (long long k = 0; k < vars[v]; ++k) owner.push_back(v);
  }
  CHECK(owner.size() == (size_t)n);
  size_t mixed_chunks = 0;
  for (size_t c = 0; c < plan.chunks.size(); ++c) {
    const uint32_t entry = plan.chunks[c];
    const uint64_t lo = (uint64_t)c * cbx::kOptChunk, hi = lo + cbx::kOptChunk;
    bool inside = false;  // a boundary between two variables strictly inside the chunk
    for (uint32_t v = 1; v < V; ++v) inside = inside || (plan.bounds[v] > lo && plan.bounds[v] < hi);
    CHECK(cbx::opt_chunk_mixed(entry) == inside);
    mixed_chunks += inside ? 1 : 0;
    CHECK(cbx::opt_chunk_var(entry) < V);
    CHECK(cbx::opt_chunk_var(entry) == owner[(size_t)lo]);
    for (uint64_t f = lo; f < hi && f < (uint64_t)n; ++f) {
      const uint32_t v = cbx::opt_chunk_mixed(entry)
                             ? cbx::variable_of(plan.bounds.data(), V, cbx::opt_chunk_var(entry), (uint32_t)f)
                             : cbx::opt_chunk_var(entry);
      CHECK(v == owner[(size_t)f]);
    }
  }
  return mixed_chunks;
}

int main() {
  size_t mixed = 0;
  const std::vector<long long> V = {1, 3, 35, 4093, 4096, 1000, 12295};
  mixed += check_case(V);
  for (size_t at : {(size_t)0, (size_t)3, V.size()}) {  // a zero-length variable: first, in the middle, last
    std::vector<long long> z = V;
    z.insert(z.begin() + (long)at, 0);
    mixed += check_case(z);
  }
  mixed += check_case({0, 0, 5, 0, 0, 251, 0, 256, 0});  // runs of empty variables, one on a chunk boundary
  mixed += check_case({1});
  mixed += check_case(std::vector<long long>(2000, 1));
  CHECK(check_case({256, 256, 512}) == 0);  // boundaries on chunk edges only: nothing mixed
  // a variable list that does not sum to n, a negative count, no variables,
  // no elements, too many bytes
  cbx::OptimisePlan plan;
  const long long bad[2] = {5, 6};
  CHECK(!cbx::build_optimise_plan(bad, 2, 12, &plan));
  CHECK(!cbx::build_optimise_plan(bad, 2, 10, &plan));
  const long long neg[2] = {-1, 13};
  CHECK(!cbx::build_optimise_plan(neg, 2, 12, &plan));
  CHECK(!cbx::build_optimise_plan(nullptr, 0, 12, &plan));
  CHECK(!cbx::build_optimise_plan(bad, 0, 11, &plan));
  const long long none[1] = {0};
  CHECK(!cbx::build_optimise_plan(none, 1, 0, &plan));
  const long long big[1] = {1ll << 30};
  CHECK(!cbx::build_optimise_plan(big, 1, 1ll << 30, &plan));  // 2^32 bytes: past the 32-bit offsets
  const long long wrap[2] = {(1ll << 62) + 6, (1ll << 62) + 6};  // a sum that would wrap is refused, not added up
  CHECK(!cbx::build_optimise_plan(wrap, 2, 12, &plan));
  CHECK(plan.chunks.empty() && plan.bounds.empty() && plan.elements == 0);
  std::printf("ok %zu mixed chunks\n", mixed);
  return 0;
}
