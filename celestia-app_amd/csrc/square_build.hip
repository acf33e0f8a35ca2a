// The data square written on the device (gfx950): every share of the k x k ODS goes straight
// into quadrant Q0 of an EDS buffer, from the layout square.cpp exports (cel_square_layout)
// and the tx bytes already in device memory. The extension then runs in place.
//
//   k_square_build  32 lanes per share, one 16-byte store per lane: the lanes of a share
//                   write its 512 contiguous bytes, share s at cell (s / k, s % k) of the
//                   EDS (row pitch 2k shares). Per share, by the kind of its segment
//                   (share_lane, the body both kernels call):
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
//
//   k_square_build_batch  the same for every block of a chunk in one launch (the batched block
//                   path, cel_block_extend_batch): the chunk's blocks have their shares,
//                   segments and compact shares concatenated in one plan, and block b's record
//                   (bb::BlockRec, block_batch_plan.hpp) says where its part of each starts,
//                   where its txs start, its log2 k and where its EDS lies in the chunk's
//                   buffer. Lane mapping as above over the chunk's shares: global share s reads
//                   the share table for its segment's index in the chunk (share_seg[s]), the
//                   segment -> block table for its block (seg_block[]), and the record; its
//                   share within the block is s - first_share, its share within the segment
//                   that minus the segment's start.
//                   The block is found through the tables, not by a search over first_share:
//                   the share table exists anyway (a share must find its segment), widening its
//                   entries to chunk-wide segment indices costs nothing, and seg_block adds 4
//                   bytes per segment, where a search would put log2(blocks) dependent loads in
//                   front of every share. Three dependent loads per share (table, block of the
//                   segment beside the segment itself, record), each the same address for the 32
//                   lanes of a share.
//                   A wave holds two shares, which may lie in different blocks (at a k = 1
//                   block every wave does): everything per share, the record and the segment
//                   included, is uniform across its 32 lanes only, and nothing is made
//                   wave-uniform (no readfirstlane).
//
// Bounds of the batch.
//   reads   share_seg[s] for s < total shares (the table's length); seg_block[i] and segs[i]
//           for i a chunk-wide segment index the host wrote (below the chunk's segment count);
//           recs[b] for b < blocks; a COMPACT share reads compact share compact_base + off + j,
//           which the host checked per block against that block's compact share count; blob
//           bytes as above, from txs + txs_base + off.
//   writes  lane (s, q) of block b writes 16 bytes at eds_off + cell ((s - first_share) / k,
//           (s - first_share) % k) of that block's EDS with 0 <= s - first_share < k * k
//           (first_share is the prefix sum of k * k): inside that block's Q0. The blocks'
//           shares partition [0, total), so every byte of every block's Q0 is written, and
//           nothing outside any Q0: no gap between blocks, no other quadrant.
//   grid    total shares * 32 lanes exactly, below 2^32 (the host refuses more). The block is
//           32 d lanes with d the largest of 8 .. 1 that divides the total share count, so no
//           lane is left without a share: 256 lanes unless the total is no multiple of 8 (an
//           odd number of k = 1 or k = 2 blocks), 32 lanes (half a wave) when it is odd.
#include <hip/hip_runtime.h>

#include "block_batch_plan.hpp"
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

// The 16 bytes lane q writes of share j of segment g: the per-share body of both kernels.
// txs: the address the segment's BLOB offset counts from; compact: the compact shares its
// COMPACT offset counts from. Uniform across a share's 32 lanes but for q.
__device__ __forceinline__ uint4 share_lane(uintptr_t txs, const cel_square_segment* __restrict__ g,
                                            const uint4* __restrict__ compact, uint32_t j, uint32_t q) {
  const uint32_t kind = g->kind;
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
      const uintptr_t A = txs + (uintptr_t)g->off + (uintptr_t)pos0;
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
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// Where lane q of share s of a square of width 2^klog writes: cell (s / k, s % k), row pitch 2k.
__device__ __forceinline__ uint8_t* share_dst(uint8_t* eds, uint32_t s, uint32_t klog, uint32_t q) {
  const uint32_t row = s >> klog, col = s & ((1u << klog) - 1u);
  return eds + (((uint64_t)row << (klog + 1)) + col) * kShare + 16u * q;
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
  *reinterpret_cast<uint4*>(share_dst(eds, s, klog, q)) = share_lane((uintptr_t)txs, g, compact, s - g->start, q);
}

__global__ __launch_bounds__(256) void k_square_build_batch(const uint8_t* __restrict__ txs,
                                                            const cel_square_segment* __restrict__ segs,
                                                            const uint32_t* __restrict__ share_seg,
                                                            const uint32_t* __restrict__ seg_block,
                                                            const bb::BlockRec* __restrict__ recs,
                                                            const uint4* __restrict__ compact,
                                                            uint8_t* __restrict__ eds, uint32_t nshares) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = t >> 5, q = t & 31u;
  if (s >= nshares) return;
  const uint32_t gi = share_seg[s];
  const cel_square_segment* __restrict__ g = segs + gi;
  const bb::BlockRec* __restrict__ b = recs + seg_block[gi];
  const uint32_t ls = s - b->first_share;  // the share within its block
  *reinterpret_cast<uint4*>(share_dst(eds + b->eds_off, ls, b->klog, q)) =
      share_lane((uintptr_t)txs + (uintptr_t)b->txs_base, g, compact + (size_t)b->compact_base * (kShare / 16),
                 ls - g->start, q);
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

// The batch: d_segs (with chunk-wide share_seg entries), d_seg_block and d_recs as the header
// describes; total_shares * 32 < 2^32. Asynchronous on s.
hipError_t launch_square_build_batch(const uint8_t* d_txs, const cel_square_segment* d_segs, const uint32_t* d_share_seg,
                                     const uint32_t* d_seg_block, const bb::BlockRec* d_recs, const uint8_t* d_compact,
                                     uint8_t* d_eds, uint32_t total_shares, hipStream_t s) {
  if (total_shares == 0) return hipSuccess;
  if (total_shares >= (1u << 27)) return hipErrorInvalidValue;
  uint32_t d = 8;
  while (total_shares % d) d--;
  const Range r("square.build.batch");
  k_square_build_batch<<<total_shares / d, 32u * d, 0, s>>>(d_txs, d_segs, d_share_seg, d_seg_block, d_recs,
                                                            reinterpret_cast<const uint4*>(d_compact), d_eds,
                                                            total_shares);
  return hipGetLastError();
}

}  // namespace cel
