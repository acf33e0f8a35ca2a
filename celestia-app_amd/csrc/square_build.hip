// The data square written on the device (gfx950): every share of the k x k ODS goes straight
// into quadrant Q0 of an EDS buffer, from the layout square.cpp exports (cel_square_layout)
// and the tx bytes already in device memory. The extension then runs in place.
//
//   k_square_build  32 lanes per share, one 16-byte store per lane: the lanes of a share
//                   write its 512 contiguous bytes, share s at cell (s / k, s % k) of the
//                   EDS (row pitch 2k shares). Per share, by the kind of its segment:
//     COMPACT  16 bytes per lane copied from the host-built compact shares;
//     PAD      ns || info byte 1 || zeros, generated;
//     BLOB     share j of a blob: ns || info || [4-byte big-endian length, j = 0] || blob
//              bytes from 0 (j = 0, at share byte 34) or 478 + 482 (j - 1) (at share byte
//              30) || zeros past the blob's end. Share byte p >= 30 is blob byte P + p - 30
//              with P = -4 for j = 0 (the length sits where blob bytes -4 .. -1 would), so
//              lane q's 16 bytes are blob bytes P + 16 q - 30 .. + 15: five aligned dwords
//              funnelled with v_alignbyte_b32 by the address's low two bits, which are the
//              same for every lane of the share (16 q keeps them).
//
// Bounds.
//   reads   a lane reads only aligned dwords that hold at least one byte of its own blob
//           (the contract of cel_dev_create_commitments: up to 3 bytes before a blob's first
//           and after its last byte are touched, never used); the share table holds k * k
//           entries, each a segment index the host checked; a COMPACT share reads compact
//           share off + j, which the host checked against the compact share count.
//   writes  lane (s, q) writes 16 bytes at cell (s / k, s % k), s < k * k: inside Q0, and
//           every byte of Q0 on every call (scratch is reused across calls).
//   grid    k * k * 32 lanes exactly (the block is 256 lanes, or all of them for k <= 2), so
//           no lane is left without a share.
#include <hip/hip_runtime.h>

#include "blob_plan.hpp"
#include "cel_internal.hpp"

namespace cel {

namespace {

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-byte load

// Mask of the bytes b of a dword at blob position lo with 0 <= lo + b < len.
__device__ __forceinline__ uint32_t inside(int64_t lo, int64_t len) {
  if (lo <= -4 || lo >= len) return 0u;
  uint32_t m = 0xFFFFFFFFu;
  if (lo < 0) m <<= 8u * (uint32_t)(-lo);
  const int64_t v = len - lo;
  if (v < 4) m &= 0xFFFFFFFFu >> (8u * (uint32_t)(4 - v));
  return m;
}

__global__ __launch_bounds__(256) void k_square_build(const uint8_t* __restrict__ txs,
                                                      const cel_square_segment* __restrict__ segs,
                                                      const uint32_t* __restrict__ share_seg,
                                                      const uint4* __restrict__ compact, uint8_t* __restrict__ eds,
                                                      uint32_t klog, uint32_t nshares) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = t >> 5, q = t & 31u;
  if (s >= nshares) return;
  const cel_square_segment* __restrict__ g = segs + share_seg[s];
  const uint32_t kind = g->kind, j = s - g->start;
  uint32_t d[4] = {0u, 0u, 0u, 0u};
  if (kind == CEL_SEG_COMPACT) {
    const uint4 v = compact[(g->off + j) * (kShare / 16) + q];
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  } else {
    const bool is_blob = kind == CEL_SEG_BLOB;
    const uint32_t* __restrict__ nsw = reinterpret_cast<const uint32_t*>(g->ns);
    const uint32_t len32 = g->len;
    if (is_blob && q >= 1) {
      const int64_t len = len32;
      const int64_t P = j == 0 ? -4 : (int64_t)blob::kSparseFirst + (int64_t)blob::kSparseCont * (j - 1);
      const int64_t pos0 = P + 16 * (int64_t)q - 30;  // blob position of share byte 16 q
      const uintptr_t A = (uintptr_t)txs + (uintptr_t)g->off + (uintptr_t)pos0;
      const uint32_t a = (uint32_t)A & 3u;
      const uint32_t* __restrict__ Q = reinterpret_cast<const uint32_t*>(A - a);
      const int64_t D0 = pos0 - a;  // blob position of Q[0]'s first byte; dword i holds D0 + 4 i .. + 3
      uint32_t x[5];
      if (D0 + 3 >= 0 && D0 + 16 < len) {  // all five dwords hold a byte of the blob
        const u32x4u v = *reinterpret_cast<const u32x4u*>(Q);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        x[4] = Q[4];
      } else {
#pragma unroll
        for (int i = 0; i < 5; i++) x[i] = (D0 + 4 * i + 3 >= 0 && D0 + 4 * i < len) ? Q[i] : 0u;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = __builtin_amdgcn_alignbyte(x[i + 1], x[i], a) & inside(pos0 + 4 * i, len);
    }
    if (q == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = nsw[i];
    } else if (q == 1) {  // share bytes 16 .. 31: ns[16 .. 28], the info byte, two payload bytes
      const uint32_t first = is_blob ? (j == 0 ? 1u : 0u) : 1u;
      const uint32_t info = is_blob ? (((g->share_version << 1) | first) & 0xFFu) : 1u;
      d[0] = nsw[4]; d[1] = nsw[5]; d[2] = nsw[6];
      d[3] = (d[3] & 0xFFFF0000u) | (nsw[7] & 0xFFu) | (info << 8);
      if (is_blob && j == 0) d[3] |= ((len32 >> 24) << 16) | (((len32 >> 16) & 0xFFu) << 24);
    } else if (q == 2 && is_blob && j == 0) {  // share bytes 32, 33: the length's low half
      d[0] |= ((len32 >> 8) & 0xFFu) | ((len32 & 0xFFu) << 8);
    }
  }
  const uint32_t row = s >> klog, col = s & ((1u << klog) - 1u);
  uint8_t* dst = eds + (((uint64_t)row << (klog + 1)) + col) * kShare + 16u * q;
  *reinterpret_cast<uint4*>(dst) = make_uint4(d[0], d[1], d[2], d[3]);
}

}  // namespace

// d_segs, d_share_seg (k * k entries) and d_compact (16-byte aligned) are the uploaded plan;
// d_eds is 16-byte aligned. Asynchronous on s.
hipError_t launch_square_build(const uint8_t* d_txs, const cel_square_segment* d_segs, const uint32_t* d_share_seg,
                               const uint8_t* d_compact, uint8_t* d_eds, uint32_t k, hipStream_t s) {
  const uint32_t nshares = k * k, lanes = nshares * 32u;
  const uint32_t block = lanes < 256u ? lanes : 256u;
  uint32_t klog = 0;
  while ((1u << klog) < k) klog++;
  const Range r("square.build");
  k_square_build<<<lanes / block, block, 0, s>>>(d_txs, d_segs, d_share_seg, reinterpret_cast<const uint4*>(d_compact),
                                                 d_eds, klog, nshares);
  return hipGetLastError();
}

}  // namespace cel
