// NMT range proofs in batches from the tree index of a resident square (nmt_prove.hpp).
//
// Replaces, for many proofs over one square, the reference's per-proof tree rebuild
// (pkg/proof/proof.go:151-201: a row NMT pushed on the CPU for each ProveRange) and this
// library's own per-proof path (cel_axis_trees' download of every node, then
// cel_nmt_prove_range per proof on the host): the index keeps every node on the device and
// the kernel below selects and packs each proof's nodes there.
//
// k_prove: one wave per proof, four proofs per workgroup.
//   nodes   A proof has at most 2 log2(2k) <= 24 nodes. Lane j < nnodes works out where node
//           j lies (prove::node_at, no recursion) and keeps its record number. Then the wave
//           copies the proof's 90 * nnodes output bytes as halfwords, lane t the t-th: it
//           takes the record number of node t / 45 from that node's lane and reads halfword
//           t % 45 of the record. A proof's output is 2-byte aligned and no more (90 bytes
//           per node, any node0), so the halfword is the widest store that is aligned for
//           every proof. With adjacent lanes on adjacent halfwords every store instruction
//           covers 128 contiguous bytes and a proof's nodes leave as whole lines but for its
//           two ends; a lane per node writing its 45 halfwords (put_root's way, right for
//           one root per lane) would put the 64 lanes of every store 90 bytes apart.
//   shares  Leaf i of the proof is cell (index, start + i) of a row, (start + i, index) of
//           a column: 32 lanes copy one share as 16-byte words, so a row's leaves are one
//           contiguous copy and a column's are whole 512-byte pieces 2k * 512 bytes apart.
// k_prove_squares: the same over a batch index (nmt_prove.hpp: n indexes back to back). The
//           request carries its square; the wave adds the square's two 64-bit byte bases
//           (prove::eds_base, prove::slice_base) to the pointers, and the rest is k_prove's.
// Bounds: the requests are checked on the host (api_prove.cpp: index < 2k, 0 <= start <
// end <= 2k), so every record number is below the index's record count and every cell inside
// the square; the outputs are sized by the same prefix sums the host gives the caller. For a
// batch index the host also checks square < n_squares before anything is enqueued, and the
// caller's buffers hold n_squares squares and slices: a record number below the record count
// and a cell below 4k^2, added to the base of a square below n_squares, lie inside them. The
// bases are 64-bit, so no product wraps (tools/index_batch_check.cpp walks the last record and
// cell of square 299 at k = 128).
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "nmt_prove.hpp"

namespace cel {

using prove::Request;
using prove::SquareRequest;

constexpr uint32_t kProofsPerGroup = 4;

// Proof q of the square whose cells are at eds and whose index is at index, by one wave.
__device__ __forceinline__ void prove_one(const uint8_t* __restrict__ eds, const uint16_t* __restrict__ index,
                                          uint32_t W, uint32_t L, const Request& q, uint8_t* __restrict__ leaves,
                                          uint8_t* __restrict__ nodes, uint32_t lane) {
  const uint32_t s = (uint32_t)q.start, e1 = (uint32_t)q.end - 1u;
  const uint32_t nn = prove::node_count(L, s, e1);
  uint32_t rec = 0;
  if (lane < nn) {
    const prove::NodeAt a = prove::node_at(L, s, e1, lane);
    rec = (uint32_t)prove::index_record(W, q.axis, q.index, a.level, a.pos);
  }
  copy_proof_nodes(rec, nn, index, reinterpret_cast<uint16_t*>(nodes + q.node0 * kNode), lane);
  if (!leaves) return;
  const uint4* cells = reinterpret_cast<const uint4*>(eds);
  uint4* lo = reinterpret_cast<uint4*>(leaves + q.leaf0 * kShare);
  const uint32_t vecs = (uint32_t)(q.end - q.start) * kShareVecs;
  for (uint32_t t = lane; t < vecs; t += 64) {
    const uint32_t p = s + t / kShareVecs;
    const uint64_t cell = prove::request_cell(W, q.axis, q.index, p);
    lo[t] = cells[cell * kShareVecs + t % kShareVecs];
  }
}

__global__ __launch_bounds__(256) void k_prove(const uint8_t* __restrict__ eds, const uint16_t* __restrict__ index,
                                               uint32_t W, uint32_t L, const Request* __restrict__ req, uint32_t n,
                                               uint8_t* __restrict__ leaves, uint8_t* __restrict__ nodes) {
  const uint32_t lane = threadIdx.x & 63u;
  // the same for the whole wave: the request loads become scalar loads
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * kProofsPerGroup + (threadIdx.x >> 6));
  if (i >= n) return;
  const Request q = req[i];
  prove_one(eds, index, W, L, q, leaves, nodes, lane);
}

// k_prove over the squares of a batch index: the request names its square, and the wave forms
// the two bases (cells, index slice) once, from scalar values.
__global__ __launch_bounds__(256) void k_prove_squares(const uint8_t* __restrict__ eds,
                                                       const uint8_t* __restrict__ index, uint32_t W, uint32_t L,
                                                       const SquareRequest* __restrict__ req, uint32_t n,
                                                       uint8_t* __restrict__ leaves, uint8_t* __restrict__ nodes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * kProofsPerGroup + (threadIdx.x >> 6));
  if (i >= n) return;
  const SquareRequest q = req[i];
  prove_one(eds + prove::eds_base(W, q.square),
            reinterpret_cast<const uint16_t*>(index + prove::slice_base(W, q.square)), W, L, q.r, leaves, nodes, lane);
}

hipError_t launch_prove(const uint8_t* eds, const void* d_index, uint32_t k, const Request* d_req, uint32_t n,
                        uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s) {
  if (!n) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_prove");
  hipLaunchKernelGGL(k_prove, dim3((n + kProofsPerGroup - 1) / kProofsPerGroup), dim3(64 * kProofsPerGroup), 0, s, eds,
                     static_cast<const uint16_t*>(d_index), x.W, x.L, d_req, n, d_leaves, d_nodes);
  return hipGetLastError();
}

hipError_t launch_prove_squares(const uint8_t* eds, const void* d_index, uint32_t k, const SquareRequest* d_req,
                                uint32_t n, uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s) {
  if (!n) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_prove_squares");
  hipLaunchKernelGGL(k_prove_squares, dim3((n + kProofsPerGroup - 1) / kProofsPerGroup), dim3(64 * kProofsPerGroup), 0,
                     s, eds, static_cast<const uint8_t*>(d_index), x.W, x.L, d_req, n, d_leaves, d_nodes);
  return hipGetLastError();
}

}  // namespace cel
