// task_barrier_adaptive_kernels.hip -- the replicas' pending task steps with
// layer-wise adaptive rates (LARS, and LARC as its capped form) fused into the
// one-GPU SMA barrier (cbx_step_and_synchronise_adaptive,
// cbx_sma_plan_step_and_optimise_adaptive), for CDNA4 (gfx950).
//
// Per stepping replica the sequence is three launches (adaptive_rate_kernels.hip:
// pass, trust, step) and then the barrier; here every stepping replica's pass is
// one launch, every trust ratio a second, and the steps ride the barrier:
//
//   replica_norms_kernel   variable_norm_kernel's wave per piece with a second
//                          grid dimension: blockIdx.y picks w, g and slab of one
//                          stepping replica from a pointer block in the kernel
//                          arguments.  The piece walk, the loads, the fp64 sums
//                          and the butterfly are that kernel's, so a slab holds
//                          the bits the per-replica pass leaves.
//   replica_trust_kernel   variable_trust_kernel's wave per variable, again with
//                          the stepping replica in blockIdx.y.  Lane 0 writes the
//                          record and the dense trust entry into the replica's
//                          own scratch, and the finished rate
//                          (rate_k * mult[v]) * t into row v, column k of the
//                          rate matrix (adaptive_steps_internal.h).
//   task_barrier_adaptive_kernel
//                          task_barrier_kernel behind the AdaptiveStep policy
//                          (task_barrier_body.inc, task_barrier_step.h): the
//                          per-variable kernel whose rate comes out of the
//                          matrix.  A uniform 256-float chunk reads the rates of
//                          a whole replica chunk in one scalar load.
//
// The two small kernels' text is adaptive_rate_kernels.hip's a second time:
// that object's code is pinned, so a fix to the piece walk, add_sq, either
// summation order or the ratio belongs in both files.
//
// This file is a shared object of its own (libcrossbow_sma_adaptive_steps.so):
// no other object's device code is touched by it.
#include <hip/hip_ext.h>

#include "adaptive_steps_internal.h"
#include "task_barrier_launch.h"
#include "task_barrier_step.h"

namespace cbx {
namespace {

static_assert(sizeof(AdaptiveRecord) == 32 && sizeof(AdaptivePartial) == 32 && sizeof(StatsPiece) == 16,
              "the layouts of adaptive_rate_kernels.hip");

// What blockIdx.y picks in the pass: 3 pointers per stepping replica.
struct NormPtrs {
  const float *w[kMaxReplicas];
  const float *g[kMaxReplicas];
  AdaptivePartial *slab[kMaxReplicas];
};
// And in the trust kernel.
struct TrustPtrs {
  const AdaptivePartial *slab[kMaxReplicas];
  AdaptiveRecord *rec[kMaxReplicas];
  float *trust[kMaxReplicas];
  float rate[kMaxReplicas];        // -learning rate of the stepping replica
  unsigned char col[kMaxReplicas]; // its slot among the participating replicas
};
static_assert(sizeof(NormPtrs) + 2 * sizeof(void *) + 8 <= 4096 &&
                  sizeof(TrustPtrs) + sizeof(AdaptiveParams) + 4 * sizeof(void *) + 8 <= 4096 &&
                  sizeof(TaskBarrierArgs) + 3 * sizeof(void *) + 8 <= 4096,
              "every kernel argument block must stay under HIP's 4 KB");

template <int P>
__device__ __forceinline__ v4f ldg4(const float *base, uint32_t off) {
  const v4f *p = reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <int P>
__device__ __forceinline__ float ldg1(const float *base, uint32_t off) {
  const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

// adaptive_rate_kernels.hip's rule, per buffer.
__device__ __forceinline__ void add_sq(double &q, uint32_t &nf, float x) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const double xd = fin ? (double)x : 0.0;
  q = fma(xd, xd, q);  // the product is exact: one rounding, the add's
  nf += fin ? 0u : 1u;
}

// float4 loads in flight per lane and buffer before the first add.
constexpr int kNormDepth = 8;

// One-wave workgroups; workgroup (b, j) walks pieces b, b + gridDim.x, ... of
// stepping replica j.  variable_norm_kernel per piece.
template <int P>
__global__ __launch_bounds__(64) void replica_norms_kernel(const NormPtrs ptrs, const StatsPiece *__restrict__ pieces,
                                                           uint32_t npieces) {
  const uint32_t lane = threadIdx.x;
  // wave-uniform: the three pointers come out of the argument block by scalar loads
  const float *__restrict__ w = ptrs.w[blockIdx.y];
  const float *__restrict__ g = ptrs.g[blockIdx.y];
  AdaptivePartial *__restrict__ slab = ptrs.slab[blockIdx.y];
  for (uint32_t p = blockIdx.x; p < npieces; p += gridDim.x) {
    const StatsPiece pc = pieces[p];  // wave-uniform
    double qw = 0.0, qg = 0.0;
    uint32_t nf = 0;
    if (pc.aligned) {
      const uint32_t lo4 = pc.lo >> 2, hi4 = pc.hi >> 2;
      for (uint32_t j = lo4; j < hi4; j += 64u * kNormDepth) {
        v4f x[kNormDepth], y[kNormDepth];
        // A float4 past the piece's end is not loaded: it adds +0 and counts
        // nothing, which leaves the non-negative sums' bits alone.
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)kNormDepth; ++u) {
          const uint32_t i4 = j + u * 64u + lane;
          x[u] = i4 < hi4 ? ldg4<P>(w, i4 * 16u) : v4f(0.0f);
          y[u] = i4 < hi4 ? ldg4<P>(g, i4 * 16u) : v4f(0.0f);
        }
        __builtin_amdgcn_sched_barrier(0);  // every load of the group in flight first
#pragma unroll
        for (int u = 0; u < kNormDepth; ++u) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            add_sq(qw, nf, x[u][k]);
            add_sq(qg, nf, y[u][k]);
          }
        }
      }
    } else {
      // At most 3 floats, or a segment without a whole float4: one per lane.
      for (uint32_t i = pc.lo + lane; i < pc.hi; i += 64u) {
        const float x = ldg1<P>(w, i * 4u), y = ldg1<P>(g, i * 4u);
        add_sq(qw, nf, x);
        add_sq(qg, nf, y);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // fixed xor butterfly: every lane ends with the same bits
      qw += __shfl_xor(qw, o);
      qg += __shfl_xor(qg, o);
      nf += __shfl_xor(nf, o);
    }
    if (lane == 0) {
      slab[p].w_sq = qw;
      slab[p].g_sq = qg;
      slab[p].nonfinite = nf;
      slab[p].reserved = 0;
    }
  }
}

// Partials in flight per lane of the trust kernel.
constexpr int kTrustDepth = 16;

// Workgroup (v, j): variable v of stepping replica j, variable_trust_kernel's
// sums and rule.  v >= nvars is the pad's pseudo-variable: no floats of the
// model, no record, multiplier 1 and ratio 1.
__global__ __launch_bounds__(64) void replica_trust_kernel(const TrustPtrs ptrs, const uint32_t *__restrict__ var_first,
                                                           const uint32_t *__restrict__ enable,
                                                           const float *__restrict__ mult, const uint32_t nvars,
                                                           const AdaptiveParams prm, float *__restrict__ matrix) {
  const uint32_t lane = threadIdx.x, v = blockIdx.x, j = blockIdx.y;
  const float rate = ptrs.rate[j];
  float *const cell = matrix + (size_t)v * kMaxReplicas + ptrs.col[j];
  if (v >= nvars) {
    if (lane == 0) *cell = (rate * 1.0f) * 1.0f;
    return;
  }
  const AdaptivePartial *__restrict__ slab = ptrs.slab[j];
  const uint32_t lo = var_first[v], hi = var_first[v + 1];
  double W = 0.0, G = 0.0;
  unsigned long long K = 0;
  // Lane l adds partials lo + l, lo + l + 64, ... in that order; their loads go
  // out kTrustDepth at a time.  A slot past the end adds +0.
  for (uint32_t i0 = lo + lane; i0 < hi; i0 += 64u * kTrustDepth) {
    AdaptivePartial p[kTrustDepth];
#pragma unroll
    for (uint32_t u = 0; u < (uint32_t)kTrustDepth; ++u) {
      const uint32_t i = i0 + u * 64u;
      p[u] = i < hi ? slab[i] : AdaptivePartial{0.0, 0.0, 0ull, 0ull};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kTrustDepth; ++u) {
      W += p[u].w_sq;
      G += p[u].g_sq;
      K += p[u].nonfinite;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    W += __shfl_xor(W, o);
    G += __shfl_xor(G, o);
    K += __shfl_xor(K, o);
  }
  if (lane == 0) {
    float t = 1.0f;
    uint32_t flags = 0;
    if (enable[v] == 0u) {
      flags = kAdaptiveExcluded;
    } else if (lo == hi) {
      // a variable without floats: nothing to apply
    } else if (W == 0.0 || G == 0.0 || K > 0) {
      flags = kAdaptiveDegenerate;
    } else {
      const double nw = sqrt(W), ng = sqrt(G);
      const double den = (ng + (double)prm.weight_decay * nw) + (double)prm.epsilon;
      // W and G are finite and positive here, so den > 0 and t is a number:
      // +inf at most, where the cast overflows, which mode 1 caps.
      t = (float)(((double)prm.trust * nw) / den);
      flags = kAdaptiveApplied;
      if (prm.mode == 1 && t > 1.0f) {
        t = 1.0f;
        flags |= kAdaptiveCapped;
      }
    }
    AdaptiveRecord *rec = ptrs.rec[j];
    rec[v].w_sq = W;
    rec[v].g_sq = G;
    rec[v].nonfinite = K;
    rec[v].trust = t;
    rec[v].flags = flags;
    ptrs.trust[j][v] = t;
    *cell = (rate * mult[v]) * t;  // the step's two fp32 multiplies, in its order
  }
}

// The template parameters are task_barrier_kernel's.  chunks / bounds: the
// tables of optimise_plan.h over at least a.n4 * 4 floats (and a.tail_hi);
// matrix: nvars rows of kMaxReplicas finished rates.
template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
__global__ __launch_bounds__(256) void task_barrier_adaptive_kernel(const TaskBarrierArgs a,
                                                                    const uint32_t *__restrict__ chunks,
                                                                    const uint32_t *__restrict__ bounds,
                                                                    const uint32_t nvars,
                                                                    const float *__restrict__ matrix) {
  const typename step_policy<AdaptiveStep, R>::type step{chunks, bounds, nvars, matrix};
#include "task_barrier_body.inc"
}

struct AdaptiveLauncher {
  typedef AdaptiveStep Step;
  static constexpr bool kSideObject = true;
  // The variables object's rule: base momentum beside stepping replicas that
  // have none, weight decay on, is the seam's shape only.
  template <bool MIXED, bool MOM, bool BMOM, bool WD>
  static constexpr bool seam_only() {
    return MIXED && !MOM && BMOM && WD;
  }
  const VarTables &vt;
  const float *matrix;
  template <int R, bool MIXED, bool MOM, bool BMOM, bool WD, bool KEEP, int P, bool TAIL, int U>
  void launch(dim3 g, dim3 b, unsigned lds, hipStream_t s, Timing t, const TaskBarrierArgs &a) const {
    hipExtLaunchKernelGGL((task_barrier_adaptive_kernel<R, MIXED, MOM, BMOM, WD, KEEP, P, TAIL, U>), g, b, lds, s,
                          t.start, t.stop, 0, a, vt.chunks, vt.bounds, vt.nvars, matrix);
  }
};

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_replica_norms(const ReplicaSteps &rs, const AdaptiveTables &t, const float *mult,
                                const AdaptiveParams &p, const RateMatrix &m, uint32_t rows, int policy,
                                hipStream_t stream, Timing pass, Timing reduce) {
  if (rs.count < 1 || rs.count > kMaxReplicas || !t.dev || t.npieces == 0 || t.nvars == 0 || !mult || !m.dev ||
      (rows != t.nvars && rows != t.nvars + 1) || rows > m.rows)
    return hipErrorInvalidValue;
  NormPtrs np;
  TrustPtrs tp;
  std::memset(&np, 0, sizeof(np));
  std::memset(&tp, 0, sizeof(tp));
  uint64_t cols = 0;
  for (int j = 0; j < rs.count; ++j) {
    const AdaptiveScratch *s = rs.scratch[j];
    if (!rs.w[j] || !rs.g[j] || !aligned16(rs.w[j]) || !aligned16(rs.g[j]) || !s || !s->dev ||
        s->npieces != t.npieces || s->nvars != t.nvars || rs.col[j] < 0 || rs.col[j] >= kMaxReplicas ||
        ((cols >> rs.col[j]) & 1ull))
      return hipErrorInvalidValue;
    for (int i = 0; i < j; ++i)  // two replicas in one scratch would race
      if (rs.scratch[i]->dev == s->dev) return hipErrorInvalidValue;
    cols |= 1ull << rs.col[j];
    np.w[j] = rs.w[j];
    np.g[j] = rs.g[j];
    np.slab[j] = s->slab();
    tp.slab[j] = s->slab();
    tp.rec[j] = s->records();
    tp.trust[j] = s->trust();
    tp.rate[j] = rs.rate[j];
    tp.col[j] = (unsigned char)rs.col[j];
  }
  const dim3 block(64);
  const dim3 grid(stats_grid(t.npieces), (unsigned)rs.count);
  if (policy == 1)
    hipExtLaunchKernelGGL((replica_norms_kernel<1>), grid, block, 0, stream, pass.start, pass.stop, 0, np, t.pieces(),
                          t.npieces);
  else
    hipExtLaunchKernelGGL((replica_norms_kernel<0>), grid, block, 0, stream, pass.start, pass.stop, 0, np, t.pieces(),
                          t.npieces);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipExtLaunchKernelGGL(replica_trust_kernel, dim3(rows, (unsigned)rs.count), block, 0, stream, reduce.start,
                        reduce.stop, 0, tp, (const uint32_t *)t.var_first(), (const uint32_t *)t.enable(), mult,
                        t.nvars, p, m.dev);
  return hipGetLastError();
}

hipError_t launch_task_barrier_adaptive(const TaskBarrierArgs &a, const VarTables &vt, const RateMatrix &m,
                                        bool keep_task_outputs, const LaunchConfig &cfg, hipStream_t stream,
                                        Timing t) {
  if (!task_barrier_tables_cover(a, vt)) return hipErrorInvalidValue;
  // every row a chunk entry or a boundary search can name is in the matrix
  if (!m.dev || m.rows < vt.nvars || (reinterpret_cast<uintptr_t>(m.dev) & 255u) != 0 || a.step_mask == 0)
    return hipErrorInvalidValue;
  return task_barrier_launch(AdaptiveLauncher{vt, m.dev}, a, keep_task_outputs, cfg, stream, t);
}

hipError_t rate_matrix_alloc(RateMatrix &m, const AdaptiveTables &t) {
  rate_matrix_free(m);
  if (!t.dev || t.nvars == 0) return hipErrorInvalidValue;
  const uint32_t rows = t.nvars + 1;  // the pad's pseudo-variable
  const size_t bytes = (size_t)rows * kMaxReplicas * sizeof(float);
  float *dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), bytes);
  if (e != hipSuccess) return e;
  // As adaptive_scratch_alloc: the memset has run before a non-blocking stream reads.
  e = hipMemset(dev, 0, bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return e;
  }
  m.dev = dev;
  m.rows = rows;
  return hipSuccess;
}

void rate_matrix_free(RateMatrix &m) {
  if (m.dev) (void)hipFree(m.dev);
  m = RateMatrix();
}

}  // namespace cbx
