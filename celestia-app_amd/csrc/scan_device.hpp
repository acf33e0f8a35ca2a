// Prefix sums over flat positions in workgroups of 256 lanes, shared by the parsers of a resident
// square (blob_parse.hip, tx_parse.hip): the block scan, the one-workgroup scan of the block
// sums, and the address of an ODS share in Q0. Every result is a place in a prefix sum, so none
// depends on a schedule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cel_internal.hpp"

namespace cel {
namespace scan {

constexpr uint32_t kWaves = 4;  // per workgroup of 256 lanes

// The cell of ODS share `share` < k * k of a square of width 2k = 2 << klog.
__device__ __forceinline__ const uint4* cell_of(const uint8_t* eds, uint32_t klog, uint32_t share) {
  const uint64_t row = share >> klog, col = share & ((1u << klog) - 1u);
  return reinterpret_cast<const uint4*>(eds + ((row << (klog + 1)) + col) * kShare);
}

// Inclusive prefix sums of N counters over the 256 lanes of a workgroup, in lane order; the
// workgroup's totals in tot (every lane). sh: kWaves * N words.
template <class T, int N>
__device__ __forceinline__ void block_scan(T (&v)[N], T (&tot)[N], T* sh) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T t[N];
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = __shfl_up(v[i], d, 64);
    if (lane >= (uint32_t)d) {
#pragma unroll
      for (int i = 0; i < N; i++) v[i] += t[i];
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int i = 0; i < N; i++) sh[wave * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++) tot[i] = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; w++) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      if (w < wave) v[i] += sh[w * N + i];
      tot[i] += sh[w * N + i];
    }
  }
}

// The exclusive prefix sum of `blocks` block sums of N counters in place by one workgroup, each
// lane a contiguous slice; the totals in tot (every lane). part: 257 * N words.
template <class T, int N>
__device__ __forceinline__ void scan_blocks(T* sums, uint64_t blocks, T (&tot)[N], T* part) {
  const uint64_t per = (blocks + 255) / 256;
  const uint64_t b0 = (uint64_t)threadIdx.x * per < blocks ? (uint64_t)threadIdx.x * per : blocks;
  const uint64_t b1 = b0 + per < blocks ? b0 + per : blocks;
  T mine[N];
  for (int i = 0; i < N; i++) mine[i] = 0;
  for (uint64_t b = b0; b < b1; b++)
    for (int i = 0; i < N; i++) mine[i] += sums[b * N + i];
  for (int i = 0; i < N; i++) part[threadIdx.x * N + i] = mine[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    T run[N];
    for (int i = 0; i < N; i++) run[i] = 0;
    for (uint32_t t = 0; t < 256; t++)
      for (int i = 0; i < N; i++) {
        const T v = part[t * N + i];
        part[t * N + i] = run[i];
        run[i] += v;
      }
    for (int i = 0; i < N; i++) part[256 * N + i] = run[i];
  }
  __syncthreads();
  T run[N];
  for (int i = 0; i < N; i++) {
    run[i] = part[threadIdx.x * N + i];
    tot[i] = part[256 * N + i];
  }
  for (uint64_t b = b0; b < b1; b++)
    for (int i = 0; i < N; i++) {
      const T v = sums[b * N + i];
      sums[b * N + i] = run[i];
      run[i] += v;
    }
}

inline uint32_t log2_of(uint32_t k) {
  uint32_t l = 0;
  while ((1u << l) < k) l++;
  return l;
}

}  // namespace scan
}  // namespace cel
