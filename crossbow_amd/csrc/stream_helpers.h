// stream_helpers.h -- the device helpers every streaming kernel of the
// library is written with (sma_kernels.hip, averaging_kernels.hip): float4
// loads / stores with a load-store policy, wave-contiguous indexing, and the
// launch grid.  Device code only; not part of the C-ABI.
#pragma once

#include "sma_internal.h"

namespace cbx {

template <int P>
__device__ __forceinline__ v4f ld(const v4f *p) {
  if constexpr (P == 1) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <int P>
__device__ __forceinline__ void st(v4f *p, v4f v) {
  if constexpr (P == 1) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// Uniform (SGPR) base + 32-bit lane byte offset: lets the compiler use the
// global_load/store "saddr + voffset" form, one VGPR per address instead of a
// 64-bit pair per stream (18+ streams per lane at R = 8).
template <int P>
__device__ __forceinline__ v4f ldo(const v4f *base, uint32_t off) {
  return ld<P>(reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(base) + off));
}

template <int P>
__device__ __forceinline__ void sto(v4f *base, uint32_t off, v4f v) {
  st<P>(reinterpret_cast<v4f *>(reinterpret_cast<char *>(base) + off), v);
}

// Wave-contiguous indexing: with U float4s per lane, wave w of block b owns
// the 64*U consecutive float4s starting at (b * waves_per_block + w) * 64 * U,
// lane l the float4s base + 64 u.  Each wave-instruction still moves one
// contiguous KiB, and a wave's U instructions per stream cover U KiB in a
// row (U = 2 at 64-thread blocks measured best: scripts/sweep.py --interleave).
template <int U>
__device__ __forceinline__ uint32_t first_elem(uint32_t block) {
  return (block * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64u * U + (threadIdx.x & 63u);
}

template <int U>
__device__ __forceinline__ uint32_t first_elem() {
  return first_elem<U>(blockIdx.x);
}

__device__ __forceinline__ v4f vfma(v4f a, v4f b, v4f c) {
  return __builtin_elementwise_fma(a, b, c);
}

// Grid for a range of n4 float4s (a multiple of block*unroll).
inline dim3 grid_for(int64_t n4, const LaunchConfig &cfg) {
  const int64_t per_block = (int64_t)cfg.block * cfg.unroll;
  int64_t blocks = (n4 + per_block - 1) / per_block;
  if (cfg.blocks_per_cu > 0) {
    const int64_t cap = (int64_t)cfg.num_cus * cfg.blocks_per_cu;
    if (blocks > cap) blocks = cap;
  }
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

}  // namespace cbx
