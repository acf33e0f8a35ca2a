// The batched NMT prover (nmt_prove.hip, api_prove.cpp): the tree index of a resident square,
// the closed form of nmt ProveRange's node selection, and the per-proof table the kernel
// reads. Everything above the device part (the node copy k_prove and k_ns_emit share, the
// launcher declarations) is plain C++ with no HIP in it: tools/prove_select_check.cpp includes
// this header alone and walks it on the host, and tools/index_batch_check.cpp the arithmetic of
// the batch index (many squares' indexes back to back).
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define CEL_PROVE_HD __host__ __device__
#else
#define CEL_PROVE_HD
#endif

namespace cel {
namespace prove {

constexpr uint32_t kRecordBytes = 96;  // a node on the device: 90 bytes and 6 zero bytes
constexpr uint32_t kMaxLevels = 16;

// ------------------------------------------------------------------ tree index
//
// Every node of the 4k row and column NMTs of one 2k x 2k square, as 96-byte records. With
// W = 2k and L = log2(W):
//   level 0      the W * W leaf records, [row][col]: the leaf of cell (r, c) is leaf c of
//                row tree r and leaf r of column tree c, so it is stored once;
//   level l >= 1 [2W trees][W >> l] records, the W row trees first, then the W column trees;
//                level L holds the 2W roots.
// Behind the records a tail the build alone uses: the roots' RFC-6962 leaf digests, a DAH
// for a caller that wants none, the push-order flag and the status.

// First record of level l (l = 0 .. L + 1; L + 1 gives the record count).
CEL_PROVE_HD inline uint64_t index_level_rec(uint32_t W, uint32_t l) {
  if (l == 0) return 0;
  return (uint64_t)W * W + (uint64_t)2 * W * (W - (W >> (l - 1)));
}

// Record of node `pos` of level l of tree `index` along `axis` (0 = row, 1 = column).
CEL_PROVE_HD inline uint64_t index_record(uint32_t W, uint32_t axis, uint32_t index, uint32_t l, uint32_t pos) {
  if (l == 0) return axis ? (uint64_t)pos * W + index : (uint64_t)index * W + pos;
  return index_level_rec(W, l) + (uint64_t)(axis ? W + index : index) * (W >> l) + pos;
}

struct IndexLayout {
  uint32_t W, L;
  uint64_t level_off[kMaxLevels];  // byte offset of level l, l = 0 .. L
  uint64_t records;                // all levels
  uint64_t leafd_off;              // [2W][32] RFC-6962 leaf digests of the roots
  uint64_t dah_off;                // 32 bytes
  uint64_t bad_off, status_off;    // int32 each
  uint64_t bytes;
};

// k a power of two, 1 <= k <= 2048.
inline IndexLayout index_layout(uint32_t k) {
  IndexLayout x{};
  x.W = 2 * k;
  while ((1u << x.L) < x.W) x.L++;
  for (uint32_t l = 0; l <= x.L; l++) x.level_off[l] = index_level_rec(x.W, l) * kRecordBytes;
  x.records = index_level_rec(x.W, x.L + 1);
  x.leafd_off = x.records * kRecordBytes;  // a multiple of 32
  x.dah_off = x.leafd_off + (uint64_t)2 * x.W * 32;
  x.bad_off = x.dah_off + 32;
  x.status_off = x.bad_off + 4;
  x.bytes = x.status_off + 4 + 8;  // to a multiple of 16
  return x;
}

// ------------------------------------------------------------------ batch index
//
// The indexes of n squares of one width, back to back: square sq's is a whole single-square
// index (records and tail) at byte slice_base(W, sq), over the cells at eds_base(W, sq) of the n
// squares' cells. Record numbers inside a slice stay 32-bit; the two bases are 64-bit byte
// offsets (256 squares at k = 128 are 4.8 GB of index). The kernels of the batch build
// (nmt_kernels.hip), k_prove_squares and the k_ns_*_squares kernels address through these, and
// tools/index_batch_check.cpp walks them against index_record and index_layout.

// Records of one index, all levels: index_level_rec(W, L + 1).
CEL_PROVE_HD inline uint64_t index_records(uint32_t W) { return (uint64_t)W * W + (uint64_t)2 * W * (W - 1); }
constexpr uint32_t kIndexTailFixed = 48;  // DAH, push-order flag, status, padding to 16
// index_layout(k).bytes in closed form: a multiple of 16.
CEL_PROVE_HD inline uint64_t index_bytes(uint32_t W) {
  return index_records(W) * kRecordBytes + (uint64_t)2 * W * 32 + kIndexTailFixed;
}
CEL_PROVE_HD inline uint64_t slice_base(uint32_t W, uint32_t sq) { return (uint64_t)sq * index_bytes(W); }
CEL_PROVE_HD inline uint64_t eds_base(uint32_t W, uint32_t sq) { return (uint64_t)sq * W * W * 512u; }
// Byte offset of level l inside a slice: index_layout's level_off[l].
CEL_PROVE_HD inline uint64_t slice_level_off(uint32_t W, uint32_t l) { return index_level_rec(W, l) * kRecordBytes; }
// The tail inside a slice: leaf digests [2W][32], DAH, push-order flag, status.
CEL_PROVE_HD inline uint64_t slice_leafd_off(uint32_t W) { return index_records(W) * kRecordBytes; }
CEL_PROVE_HD inline uint64_t slice_dah_off(uint32_t W) { return slice_leafd_off(W) + (uint64_t)2 * W * 32; }
CEL_PROVE_HD inline uint64_t slice_bad_off(uint32_t W) { return slice_dah_off(W) + 32; }
CEL_PROVE_HD inline uint64_t slice_status_off(uint32_t W) { return slice_bad_off(W) + 4; }
// Cell of leaf p of tree `index` along `axis`, inside its square: below W * W.
CEL_PROVE_HD inline uint64_t request_cell(uint32_t W, uint32_t axis, uint32_t index, uint32_t p) {
  return axis ? (uint64_t)p * W + index : (uint64_t)index * W + p;
}
// One launch takes the square in a grid dimension of 16 bits: a call over more squares is
// rejected (CEL_EINVAL), not split.
constexpr uint32_t kMaxSquares = 65535;

// ------------------------------------------------- ProveRange's nodes, closed form
//
// nmt ProveRange(start, end) over 2^L leaves lists, left to right, the roots of the maximal
// subtrees outside [start, end) (proof.cpp: collect). With s = start and e1 = end - 1 these
// are the left siblings along s's path, from the top down (every level l whose bit of s is
// set: node (s >> l) ^ 1), then the right siblings along e1's path, from the bottom up
// (every level l whose bit of e1 is clear: node (e1 >> l) ^ 1).

struct NodeAt {
  uint32_t level, pos;
};

CEL_PROVE_HD inline uint32_t node_count(uint32_t L, uint32_t s, uint32_t e1) {
  return (uint32_t)__builtin_popcount(s) + L - (uint32_t)__builtin_popcount(e1);
}

// Node j of the proof, j < node_count(L, s, e1); {L, 0} beyond it.
CEL_PROVE_HD inline NodeAt node_at(uint32_t L, uint32_t s, uint32_t e1, uint32_t j) {
  const uint32_t left = (uint32_t)__builtin_popcount(s);
  if (j < left) {
    for (uint32_t l = L; l-- > 0;)
      if ((s >> l) & 1u) {
        if (j == 0) return NodeAt{l, (s >> l) ^ 1u};
        j--;
      }
  } else {
    j -= left;
    for (uint32_t l = 0; l < L; l++)
      if (!((e1 >> l) & 1u)) {
        if (j == 0) return NodeAt{l, (e1 >> l) ^ 1u};
        j--;
      }
  }
  return NodeAt{L, 0};
}

// One proof of a batch as the kernel reads it: ProveRange(start, end) on tree `index` along
// `axis`, its nodes from packed node node0 on, its shares from share leaf0 on.
struct Request {
  uint32_t axis, index;
  int32_t start, end;
  uint64_t node0, leaf0;
};
static_assert(sizeof(Request) == 32, "Request layout");

// One proof of a batch over many squares (k_prove_squares): the request and the square it
// names, whose cells and index slice lie at eds_base / slice_base.
struct SquareRequest {
  Request r;
  uint32_t square, pad;
};
static_assert(sizeof(SquareRequest) == 40, "SquareRequest layout");

}  // namespace prove
}  // namespace cel

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"

namespace cel {

constexpr uint32_t kNodeHalves = kNode / 2;         // 45
constexpr uint32_t kRecordHalves = kNodeWords * 2;  // 48
constexpr uint32_t kShareVecs = kShare / 16;        // 32

// A proof's nn <= 64 nodes out of the index as packed 90-byte nodes at `out`, by one wave: lane
// j < nn holds the record number of node j in `rec`. The wave copies the 45 * nn halfwords,
// lane t the t-th of each 64: it takes the record number of node t / 45 from that node's lane
// and reads halfword t % 45 of the record. Every lane takes every turn (the trip count is the
// wave's), so the lane a record number is read from is always active.
__device__ __forceinline__ void copy_proof_nodes(uint32_t rec, uint32_t nn, const uint16_t* __restrict__ index,
                                                 uint16_t* out, uint32_t lane) {
  const uint32_t halves = nn * kNodeHalves;
  for (uint32_t base = 0; base < halves; base += 64) {
    const uint32_t t = base + lane;
    const uint32_t j = t < halves ? t / kNodeHalves : 0u;
    const uint32_t r = (uint32_t)__shfl((int)rec, (int)j, 64);
    if (t < halves) out[t] = index[(uint64_t)r * kRecordHalves + (t - j * kNodeHalves)];
  }
}

// The index of the square at eds (nmt_kernels.hip: the single-square commit's leaf and level
// kernels, every level written to its own place in d_index), the packed roots, and the DAH
// (nullable) as launch_commit gives them. status: device int32, nullable.
hipError_t launch_tree_index(const uint8_t* eds, uint32_t k, void* d_index, uint8_t* row_roots, uint8_t* col_roots,
                             uint8_t* dah, int32_t* status, bool order_check, hipStream_t s);
// n proofs from d_index (nmt_prove.hip). d_req: the n requests in device memory. d_leaves
// nullable (then eds is not read); both 16-byte aligned. d_nodes 2-byte aligned.
hipError_t launch_prove(const uint8_t* eds, const void* d_index, uint32_t k, const prove::Request* d_req, uint32_t n,
                        uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s);

// The batch index of the nsq <= prove::kMaxSquares squares at eds (nmt_kernels.hip): per square
// what launch_tree_index gives, square sq's index at prove::slice_base, its roots at
// row_roots / col_roots + sq * 2k * 90, its DAH at dah + 32 * sq (dah nullable: each slice's
// tail). status: device, [nsq], nullable; each slice's tail gets its own as well then.
hipError_t launch_tree_index_batch(const uint8_t* eds, uint32_t k, uint32_t nsq, void* d_index, uint8_t* row_roots,
                                   uint8_t* col_roots, uint8_t* dah, int32_t* status, bool order_check,
                                   hipStream_t s);
// n proofs over the squares of a batch index (nmt_prove.hip): request i names its square.
hipError_t launch_prove_squares(const uint8_t* eds, const void* d_index, uint32_t k, const prove::SquareRequest* d_req,
                                uint32_t n, uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s);

}  // namespace cel
#endif
