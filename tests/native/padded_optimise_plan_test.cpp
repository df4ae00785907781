// The padded chunk table of the fused task-step barrier with per-variable
// rates (build_padded_optimise_plan, crossbow_amd/csrc/optimise_plan.h) on the
// CPU, under ASan + UBSan (tests/test_step_and_synchronise_variables_abi.py
// builds and runs it).  The rule: the table runs over the padded length in
// whole chunks, so a kernel that sweeps the pad reads no table past its end;
// every float of [0, n) keeps its own variable, in a last partial chunk too;
// every pad float belongs to the pseudo-variable nvars.
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

constexpr long long kPadFloats = 4096;  // kPadFloat4 float4s

static size_t check_case(const std::vector<long long> &vars) {
  long long n = 0;
  for (long long e : vars) n += e;
  const long long padded = (n + kPadFloats - 1) / kPadFloats * kPadFloats;
  cbx::OptimisePlan plan;
  CHECK(cbx::build_padded_optimise_plan(vars.data(), (int)vars.size(), n, padded, &plan));
  const uint32_t V = (uint32_t)vars.size();
  CHECK(plan.nvars == (int)V + 1 && plan.elements == padded);
  CHECK(plan.bounds.size() == (size_t)V + 2);
  CHECK(plan.bounds[V] == (uint32_t)n && plan.bounds[V + 1] == (uint32_t)padded);
  CHECK(padded % cbx::kOptChunk == 0);
  CHECK(plan.chunks.size() == (size_t)(padded / cbx::kOptChunk));  // one entry per chunk of the sweep
  std::vector<uint32_t> owner;
  for (uint32_t v = 0; v < V; ++v)
    for (long long k = 0; k < vars[v]; ++k) owner.push_back(v);
  size_t pad_floats = 0;
  for (size_t c = 0; c < plan.chunks.size(); ++c) {
    const uint32_t entry = plan.chunks[c];
    CHECK(cbx::opt_chunk_var(entry) <= V);
    for (uint64_t f = (uint64_t)c * cbx::kOptChunk; f < (uint64_t)(c + 1) * cbx::kOptChunk; ++f) {
      const uint32_t v = cbx::opt_chunk_mixed(entry)
                             ? cbx::variable_of(plan.bounds.data(), V + 1, cbx::opt_chunk_var(entry), (uint32_t)f)
                             : cbx::opt_chunk_var(entry);
      if (f < (uint64_t)n) {
        CHECK(v == owner[(size_t)f]);
      } else {
        CHECK(v == V);
        ++pad_floats;
      }
    }
  }
  CHECK(pad_floats == (size_t)(padded - n));
  return pad_floats;
}

int main() {
  size_t pad = 0;
  pad += check_case({1, 3, 35, 4093, 4096, 1000, 12295});  // 21,523 floats: a last partial chunk, 3,053 pad floats
  pad += check_case({2049, 2050});                         // 4,099: one float4 past a pad quantum
  pad += check_case({1});
  pad += check_case({255, 1, 0});                          // n on a chunk boundary, an empty last variable
  pad += check_case({4095, 0, 0});
  CHECK(check_case({4096}) == 0);                          // no pad: the pseudo-variable is empty, no chunk names it
  CHECK(check_case({1000, 3096, 4096}) == 0);
  cbx::OptimisePlan plan;
  const long long two[2] = {5, 6};
  CHECK(!cbx::build_padded_optimise_plan(two, 2, 11, 10, &plan));   // a padded length below n
  CHECK(!cbx::build_padded_optimise_plan(two, 2, 12, 4096, &plan)); // variables that do not sum to n
  CHECK(!cbx::build_padded_optimise_plan(nullptr, 0, 11, 4096, &plan));
  const long long big[1] = {(1ll << 30) - 1};
  CHECK(!cbx::build_padded_optimise_plan(big, 1, (1ll << 30) - 1, 1ll << 30, &plan));  // the padded bytes pass 2^32
  CHECK(plan.chunks.empty() && plan.bounds.empty() && plan.elements == 0 && plan.nvars == 0);
  std::printf("ok %zu pad floats\n", pad);
  return 0;
}
