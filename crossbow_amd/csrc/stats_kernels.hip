// stats_kernels.hip -- per-variable model statistics and replica divergence,
// reduced on the device (cbx_model_stats, the checkpoint guard,
// cbx_sma_plan_buffer_stats).  The reference checksums a buffer with a host
// loop on every store and load (clib-multigpu/databuffer.c:141-162, 218, 255,
// behind COMPUTE_CHECKSUM); here one pass over HBM reads the reference buffer
// (the base model z) and up to kMaxReplicas buffers (every local w, or s)
// once and yields, per variable and per buffer, the sum, the sum of squares,
// the squared distance to the reference, the largest magnitude and the count
// of non-finite values.
//
//   pass      one wave per piece of the host-built piece table (stats_plan.h):
//             aligned pieces by 16-byte loads, the others one float per lane;
//             replicas in register-resident chunks of kChunk whose loads are
//             all issued before the first use, as in the fused SMA kernel.
//             A model of more than kChunk buffers re-reads a piece's 16 KiB
//             of the reference once per further chunk, from cache.  Every
//             lane accumulates in fp64 from the first add ((double)x and x*x
//             are exact, x - ref rounds once); the wave folds its lanes with
//             a fixed xor butterfly and lane 0 writes one partial record per
//             (piece, buffer) to a slab.
//   reduce    a wave per (variable, buffer) sums that variable's records: lane
//             l takes records l, l + 64, ... in piece order, then the same
//             butterfly.  A second launch of the same kernel sums the
//             variables' records into the whole-model record.
//
// No float atomics and no order that depends on arrival: piece table, grid
// and summation tree are fixed functions of the variable list, so two calls
// on the same data return the same bits (a slab of partial records plus a
// reduce at the launch boundary).
#include <hip/hip_ext.h>

#include "context_internal.h"
#include "stats_internal.h"

using cbx::host::fail;

namespace cbx {
namespace {

template <int P>
__device__ __forceinline__ v4f ldo4(const float *base, uint32_t off) {
  const v4f *p = reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <int P>
__device__ __forceinline__ float ldo1(const float *base, uint32_t off) {
  const float *p = reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

struct Acc {
  double s = 0.0, q = 0.0, d = 0.0;
  float m = 0.0f;
  uint32_t nf = 0;
};

__device__ __forceinline__ bool is_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// A non-finite x counts and adds nothing else; a finite x beside a non-finite
// reference adds everything but the distance.
__device__ __forceinline__ void acc_ref(Acc &a, float x, bool fin, double xd) {
  a.s += xd;
  a.q = fma(xd, xd, a.q);
  a.m = fmaxf(a.m, fin ? fabsf(x) : 0.0f);
  a.nf += fin ? 0u : 1u;
}

__device__ __forceinline__ void acc_buf(Acc &a, float x, bool rfin, double rd) {
  const bool fin = is_finite(x);
  const double xd = fin ? (double)x : 0.0;
  acc_ref(a, x, fin, xd);
  const double df = (fin && rfin) ? xd - rd : 0.0;
  a.d = fma(df, df, a.d);
}

// Fixed xor butterfly over the 64 lanes: every lane ends with the same bits.
__device__ __forceinline__ void wave_fold(Acc &a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.s += __shfl_xor(a.s, o);
    a.q += __shfl_xor(a.q, o);
    a.d += __shfl_xor(a.d, o);
    a.m = fmaxf(a.m, __shfl_xor(a.m, o));
    a.nf += __shfl_xor(a.nf, o);
  }
}

__device__ __forceinline__ void put(cbx_buffer_stats *out, const Acc &a) {
  out->sum = a.s;
  out->sum_sq = a.q;
  out->dist_sq = a.d;
  out->nonfinite = a.nf;
  out->max_abs = a.m;
  out->reserved = 0;
}

// One element of the reference and of the chunk's buffers.
template <int RR>
__device__ __forceinline__ void elem(Acc &ra, Acc (&acc)[RR], float z, const float (&x)[RR], int live) {
  const bool rfin = is_finite(z);
  const double rd = rfin ? (double)z : 0.0;
  acc_ref(ra, z, rfin, rd);
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    if (r >= live) break;
    acc_buf(acc[r], x[r], rfin, rd);
  }
}

// R > 0: exactly R buffers, unrolled; R == -1: a.nbufs buffers in chunks of
// kChunk.  One-wave workgroups; workgroup g walks pieces g, g + grid, ...
template <int R>
__global__ __launch_bounds__(64) void stats_pass_kernel(const StatsArgs a) {
  constexpr int RR = (R > 0) ? R : kChunk;
  const uint32_t lane = threadIdx.x;
  const int nb = (R > 0) ? R : a.nbufs;
  const uint32_t nbt = (uint32_t)nb + 1u;
  for (uint32_t p = blockIdx.x; p < a.npieces; p += gridDim.x) {
    const StatsPiece pc = a.pieces[p];
    cbx_buffer_stats *rec = a.slab + (size_t)p * nbt;
    for (int c = 0; c == 0 || c < nb; c += RR) {
      const int live = (R > 0) ? RR : (nb - c < RR ? nb - c : RR);
      Acc ra, acc[RR];
      if (pc.aligned) {
        for (uint32_t i4 = (pc.lo >> 2) + lane; i4 < (pc.hi >> 2); i4 += 64u) {
          const uint32_t off = i4 * 16u;
          // the reference with a plain load: a later chunk finds it in cache
          const v4f zv = ldo4<0>(a.ref, off);
          v4f xv[RR];
#pragma unroll
          for (int r = 0; r < RR; ++r) {
            if (r >= live) break;
            xv[r] = ldo4<1>(a.bufs[c + r], off);
          }
          // every load of the chunk in flight before the first use (see the
          // fused SMA kernel)
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float x[RR];
#pragma unroll
            for (int r = 0; r < RR; ++r) {
              if (r >= live) break;
              x[r] = xv[r][j];
            }
            elem<RR>(ra, acc, zv[j], x, live);
          }
        }
      } else {
        for (uint32_t i = pc.lo + lane; i < pc.hi; i += 64u) {
          const uint32_t off = i * 4u;
          const float z = ldo1<0>(a.ref, off);
          float x[RR];
#pragma unroll
          for (int r = 0; r < RR; ++r) {
            if (r >= live) break;
            x[r] = ldo1<1>(a.bufs[c + r], off);
          }
          __builtin_amdgcn_sched_barrier(0);
          elem<RR>(ra, acc, z, x, live);
        }
      }
      if (c == 0) {
        wave_fold(ra);  // its dist_sq stays 0
        if (lane == 0) put(rec, ra);
      }
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (r >= live) break;
        wave_fold(acc[r]);
        if (lane == 0) put(rec + 1 + c + r, acc[r]);
      }
      if constexpr (R > 0) break;
    }
  }
}

// out[s * nb + b] = the sum of in[i * nb + b] over i in [seg[s], seg[s + 1]),
// one wave per (s, b).
__global__ __launch_bounds__(64) void stats_reduce_kernel(const cbx_buffer_stats *in, const uint32_t *seg, uint32_t nb,
                                                         cbx_buffer_stats *out) {
  const uint32_t s = blockIdx.x / nb, b = blockIdx.x % nb;
  const uint32_t lo = seg[s], hi = seg[s + 1];
  double sum = 0.0, sq = 0.0, dist = 0.0;
  float m = 0.0f;
  unsigned long long nf = 0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 64u) {
    const cbx_buffer_stats *r = in + (size_t)i * nb + b;
    sum += r->sum;
    sq += r->sum_sq;
    dist += r->dist_sq;
    m = fmaxf(m, r->max_abs);
    nf += r->nonfinite;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    sq += __shfl_xor(sq, o);
    dist += __shfl_xor(dist, o);
    m = fmaxf(m, __shfl_xor(m, o));
    nf += __shfl_xor(nf, o);
  }
  if (threadIdx.x == 0) {
    cbx_buffer_stats *o = out + (size_t)s * nb + b;
    o->sum = sum;
    o->sum_sq = sq;
    o->dist_sq = dist;
    o->nonfinite = nf;
    o->max_abs = m;
    o->reserved = 0;
  }
}

int grow(char **p, size_t *have, size_t need) {
  if (*have >= need) return CBX_OK;
  if (*p) {
    HIP_TRY(hipFree(*p));
    *p = nullptr;
    *have = 0;
  }
  need = (need + 4095) / 4096 * 4096;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(p), need);
  if (e != hipSuccess) return fail(CBX_ERR_HIP, "statistics scratch of %zu bytes: %s", need, hipGetErrorString(e));
  *have = need;
  return CBX_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int stats_run(StatsScratch &s, hipStream_t stream, const float *ref, const float *const *bufs, int nbufs,
              const long long *var_elements, int nvars, long long elements, cbx_buffer_stats *totals,
              cbx_buffer_stats *vars) {
  static_assert(sizeof(cbx_buffer_stats) == 40, "cbx_buffer_stats is 40 bytes without padding");
  if (!ref || !totals || nbufs < 0 || nbufs > kMaxReplicas || (nbufs > 0 && !bufs))
    return fail(CBX_ERR_INVALID, "buffer statistics: need a reference, 0..%d buffers and a result array", kMaxReplicas);
  if (nvars < 0 || (nvars > 0 && !var_elements)) return fail(CBX_ERR_INVALID, "buffer statistics: bad variable list");
  if (!aligned16(ref)) return fail(CBX_ERR_INVALID, "buffer statistics: the reference buffer is not 16-byte aligned");
  for (int i = 0; i < nbufs; ++i)
    if (!bufs[i] || !aligned16(bufs[i]))
      return fail(CBX_ERR_INVALID, "buffer statistics: buffer %d is null or not 16-byte aligned", i);

  // The piece table: rebuilt and uploaded only when the variable list changes.
  std::vector<long long> key;
  key.push_back(elements);
  for (int v = 0; v < nvars; ++v) key.push_back(var_elements[v]);
  if (!s.uploaded || key != s.key) {
    s.uploaded = false;
    if (!build_stats_plan(var_elements, nvars, elements, &s.plan))
      return fail(CBX_ERR_INVALID, "buffer statistics: %d variables do not sum to %lld elements (or over 2^32 bytes)",
                  nvars, elements);
    s.key = key;
  }
  const size_t V = s.plan.var_first.size() - 1;
  const size_t np = s.plan.pieces.size();
  const size_t nb = (size_t)nbufs + 1;
  const size_t pieces_bytes = np * sizeof(StatsPiece);
  const size_t seg_bytes = (V + 1 + 2) * sizeof(uint32_t);
  if (!s.uploaded) {
    TRY(grow(&s.table, &s.table_bytes, pieces_bytes + seg_bytes));
    std::vector<uint32_t> seg(s.plan.var_first);
    seg.push_back(0u);
    seg.push_back((uint32_t)V);
    HIP_TRY(hipMemcpyAsync(s.table, s.plan.pieces.data(), pieces_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s.table + pieces_bytes, seg.data(), seg_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // `seg` is this call's
    s.uploaded = true;
  }
  const size_t out_records = (1 + V) * nb;
  TRY(grow(&s.records, &s.records_bytes, (out_records + np * nb) * sizeof(cbx_buffer_stats)));
  if (!s.start) {
    HIP_TRY(hipEventCreate(&s.start));
    HIP_TRY(hipEventCreate(&s.mid));
    HIP_TRY(hipEventCreate(&s.stop));
  }
  s.timed = false;

  StatsArgs a = {};
  for (int i = 0; i < nbufs; ++i) a.bufs[i] = bufs[i];
  a.ref = ref;
  a.pieces = reinterpret_cast<const StatsPiece *>(s.table);
  const uint32_t *seg = reinterpret_cast<const uint32_t *>(s.table + pieces_bytes);
  cbx_buffer_stats *rec_total = reinterpret_cast<cbx_buffer_stats *>(s.records);
  cbx_buffer_stats *rec_vars = rec_total + nb;
  a.slab = rec_total + out_records;
  a.npieces = (uint32_t)np;
  a.nbufs = nbufs;
  const dim3 grid(stats_grid(np)), block(64);
  if (nbufs == kChunk)
    hipExtLaunchKernelGGL((stats_pass_kernel<kChunk>), grid, block, 0, stream, s.start, s.mid, 0, a);
  else
    hipExtLaunchKernelGGL((stats_pass_kernel<-1>), grid, block, 0, stream, s.start, s.mid, 0, a);
  HIP_TRY(hipGetLastError());
  hipExtLaunchKernelGGL(stats_reduce_kernel, dim3((unsigned)(V * nb)), block, 0, stream, nullptr, nullptr, 0,
                        (const cbx_buffer_stats *)a.slab, seg, (uint32_t)nb, rec_vars);
  HIP_TRY(hipGetLastError());
  hipExtLaunchKernelGGL(stats_reduce_kernel, dim3((unsigned)nb), block, 0, stream, nullptr, s.stop, 0,
                        (const cbx_buffer_stats *)rec_vars, seg + V + 1, (uint32_t)nb, rec_total);
  HIP_TRY(hipGetLastError());
  s.host.resize(out_records);
  HIP_TRY(hipMemcpyAsync(s.host.data(), s.records, out_records * sizeof(cbx_buffer_stats), hipMemcpyDeviceToHost,
                         stream));
  HIP_TRY(hipStreamSynchronize(stream));
  s.timed = true;
  std::copy(s.host.begin(), s.host.begin() + nb, totals);
  if (vars) std::copy(s.host.begin() + nb, s.host.end(), vars);
  return CBX_OK;
}

int stats_last_ms(StatsScratch &s, float *pass_ms, float *total_ms) {
  *pass_ms = *total_ms = -1.0f;
  if (!s.timed) return CBX_OK;
  HIP_TRY(hipEventElapsedTime(pass_ms, s.start, s.mid));
  HIP_TRY(hipEventElapsedTime(total_ms, s.start, s.stop));
  return CBX_OK;
}

void stats_free(StatsScratch &s) {
  if (s.table) (void)hipFree(s.table);
  if (s.records) (void)hipFree(s.records);
  for (hipEvent_t e : {s.start, s.mid, s.stop})
    if (e) (void)hipEventDestroy(e);
  s = StatsScratch();
}

}  // namespace cbx
