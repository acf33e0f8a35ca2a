// Namespaced Merkle tree roots and the DataAvailabilityHeader hash on gfx950.
//
// Replaces, for the 4k axes of a 2k x 2k EDS:
//   rsmt2d RowRoots/ColRoots [dep] -> wrapper.ErasuredNamespacedMerkleTree.Push/Root
//   (pkg/wrapper/nmt_wrapper.go:93-124) -> nmt v0.22.0 HashLeaf / HashNode with
//   IgnoreMaxNamespace (text copy: test/util/malicious/hasher.go:196-310), and
//   DataAvailabilityHeader.Hash (pkg/da/data_availability_header.go:92-108) ->
//   go-square/merkle RFC-6962.
//
// Work decomposition (one message per lane everywhere):
//   k_leaf   : one lane per EDS cell. A cell's row leaf and column leaf are the same
//              bytes (the Q0 test of nmt_wrapper.go:138-140 is symmetric), so each
//              leaf is hashed once: 4k^2 x 9 compressions instead of the reference's
//              8k^2 x 9. Also checks the honest push order on Q0. One square's commit.
//   k_leaf_quad* : a batch's leaves and level 1: one lane per 2x2 block of cells hashes
//              its four leaves and the two row and two column nodes over them, so no
//              leaf record is written. For k >= 16 two launches, one kernel per class of
//              tile: k_leaf_quad_q0 (the blocks inside Q0: records, namespaces, the push
//              order) and k_leaf_quad_par (the three quarters outside: digests only);
//              the tile numbering of each is quad_tiles.hpp. Below 16, k_leaf_quad.
//   k_level  : one lane per inner node of one tree level, all 4k trees at once.
//   k_level_split : a batch's levels above level 1: the nodes outside Q0 as 32-byte digests
//              under a hash with their constant words folded, the Q0 nodes as records.
//   k_dah    : one workgroup per square, RFC-6962 over the 4k roots.
// Nodes live on the device as 96-byte records (90 B node + 6 zero bytes) = 24 dwords; a
// slab's row-subtree records carry a mark in dword 23 (k_slab_status).
//
// This file is the EDS commit, and the build of a square's tree index (launch_tree_index: the
// single-square commit with every level kept, nmt_prove.hpp; the proofs from it are
// nmt_prove.hip), and the same for many squares in one launch per step (launch_tree_index_batch:
// k_leaf_index, k_level_index, k_merkle_index, with their bounds argument, near the end of the
// file). The row-sharded mode is nmt_slab.hip; single trees, the
// repair's axes roots, exported trees and the byte-slice hash are nmt_trees.hip.
#include <hip/hip_runtime.h>

#include <climits>

#include "cel_internal.hpp"
#include "nmt_device.hpp"
#include "nmt_host.hpp"
#include "nmt_prove.hpp"
#include "quad_tiles.hpp"
#include "sha256_device.hpp"

namespace cel {

// load_node / store_node / put_digest, hash_node / hash_pair and the RFC-6962 hashes:
// nmt_device.hpp

// --------------------------------------------------------------------- leaves

// leaf_hash / make_leaf_node (the 542-byte leaf message of a share), ns_less: nmt_device.hpp

// grid: x = cell block (256 cells from cell0), y = square. Writes leaf nodes [sq][W*W][24]
// of cells [cell0, cell1).
template <bool ORDER, bool PF>
__global__ __launch_bounds__(256) void k_leaf(const uint8_t* __restrict__ eds, uint32_t k, uint32_t* __restrict__ leaves,
                                              int32_t* __restrict__ bad_axis, uint32_t cell0, uint32_t cell1) {
  const uint32_t W = 2 * k;
  const uint32_t cell = cell0 + blockIdx.x * 256u + threadIdx.x;
  if (cell >= cell1) return;
  const uint32_t r = cell / W, c = cell % W;
  const uint64_t sq_eds = (uint64_t)W * W * kShare;
  const uint32_t* sh = reinterpret_cast<const uint32_t*>(eds + blockIdx.y * sq_eds + (uint64_t)cell * kShare);
  const bool q0 = (r < k) && (c < k);
  {
    uint32_t nd[kNodeWords];
    make_leaf_node<PF>(sh, q0, nd);
    store_node(leaves + ((uint64_t)blockIdx.y * W * W + cell) * kNodeWords, nd);
  }
  // The push-order check runs after the hash: done first, its share prefixes stay live
  // across the nine compressions (103 VGPRs, 4 waves/SIMD, against 52 and 8).
  __builtin_amdgcn_sched_barrier(0);
  if (ORDER && q0) {
    if (c > 0 && ns_less(sh, sh - kShare / 4)) atomicMin(bad_axis + blockIdx.y, (int32_t)r);
    if (r > 0 && ns_less(sh, sh - (uint64_t)W * kShare / 4)) atomicMin(bad_axis + blockIdx.y, (int32_t)(W + c));
  }
}

// ---------------------------------------------------------------- inner nodes

// The root-level outputs of tree t's root o in square sq (k_level's last level, k_leaf_quad
// at W = 2).
__device__ __forceinline__ void put_root(const uint32_t (&o)[kNodeWords], uint32_t sq, uint32_t t, uint32_t W,
                                         uint32_t* __restrict__ leafd, uint8_t* __restrict__ row_out,
                                         uint8_t* __restrict__ col_out) {
  {  // 90-byte record at a 2-byte aligned address: 45 halfword stores
    uint8_t* r = (t < W ? row_out + ((uint64_t)sq * W + t) * kNode : col_out + ((uint64_t)sq * W + (t - W)) * kNode);
    uint16_t* r16 = reinterpret_cast<uint16_t*>(r);
#pragma unroll
    for (int i = 0; i < 45; i++) r16[i] = (uint16_t)(o[i / 2] >> (16 * (i & 1)));
  }
  if (leafd) {
    uint32_t st[8];
    rfc_leaf90(o, st);
    uint4* d = reinterpret_cast<uint4*>(leafd + ((uint64_t)sq * 2 * W + t) * 8);
    d[0] = make_uint4(st[0], st[1], st[2], st[3]);
    d[1] = make_uint4(st[4], st[5], st[6], st[7]);
  }
}

// One tree level for all trees (hash_pair: nmt_device.hpp). Input addressing:
//   FROM_LEAVES: tree t < W is row t (children leaves (t, 2j), (t, 2j+1));
//                tree t >= W is column t-W (children (2j, c), (2j+1, c)).
//   otherwise  : in[sq][t][2j], in[sq][t][2j+1] with `nin` nodes per tree.
// At the root level the lane writes its root, packed to 90 bytes, straight into the
// caller's row_out / col_out ([nsq][W][90]); with leafd != nullptr it also hashes the root
// as an RFC-6962 leaf of the DAH tree (2 compressions) so the per-square DAH kernel starts
// from leaf digests.
template <bool FROM_LEAVES>
__global__ __launch_bounds__(256) void k_level(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t W,
                                               uint32_t nin, uint32_t trees, uint32_t* __restrict__ leafd,
                                               uint8_t* __restrict__ row_out, uint8_t* __restrict__ col_out) {
  const uint32_t nout = nin / 2;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= trees * nout) return;
  const uint32_t t = idx / nout, j = idx % nout;
  uint64_t li, ri;
  if (FROM_LEAVES) {
    const uint64_t sq = (uint64_t)blockIdx.y * W * W;
    if (t < W) { li = sq + (uint64_t)t * W + 2 * j; ri = li + 1; }
    else { li = sq + (uint64_t)(2 * j) * W + (t - W); ri = li + W; }
  } else {
    const uint64_t sq = (uint64_t)blockIdx.y * trees * nin;
    li = sq + (uint64_t)t * nin + 2 * j;
    ri = li + 1;
  }
  uint32_t o[kNodeWords];
  hash_pair(in, li, ri, o);
  const uint64_t oi = (uint64_t)blockIdx.y * trees * nout + idx;
  store_node(out + oi * kNodeWords, o);
  if (row_out) put_root(o, blockIdx.y, t, W, leafd, row_out, col_out);
}

// ------------------------------------------------------- a batch's split levels

// A batch keeps every level in two classes, told apart by position alone. A node is a
// parity node if its subtree lies outside Q0: every node of row trees k..2k-1 and column
// trees k..2k-1, and the upper half of every level of the mixed trees (rows and columns
// 0..k-1). Its namespaces are 0xFF*29 whatever the shares hold, so it is kept as its
// digest (8 big-endian state words) and hashed by hash_parity_node. The lower half of a
// mixed tree's level are Q0 nodes: 96-byte records through hash_node, also where a Q0
// subtree's namespaces happen to be 0xFF*29. A level of n nodes per tree, per square:
//   Q records [2k mixed trees][n/2]            mixed tree m: row m, or column m - k
//   P digests [2k mixed trees][n/2] | [2k parity trees][n]
//                                              parity tree p: row k + p, or column p
// Both are plain pair reductions: node i of the next level is the hash of nodes 2i, 2i+1 of
// this one in either array, so a level's lanes need no tree arithmetic, and a wave is of
// one class. At n = 2 the next level is the roots: mixed tree m's is HashNode(Q[m], P[m])
// (the join), parity tree p's the hash of P[2k + 2p], P[2k + 2p + 1].
__host__ __device__ constexpr uint32_t q_nodes(uint32_t k, uint32_t n) { return k * n; }
__host__ __device__ constexpr uint32_t p_nodes(uint32_t k, uint32_t n) { return 3 * k * n; }
// node i of tree t (rows 0..2k-1, then columns) in a level of n nodes per tree
__device__ __forceinline__ uint32_t q_node(uint32_t k, uint32_t n, uint32_t t, uint32_t i) {
  return (t < k ? t : t - k) * (n / 2) + i;
}
__device__ __forceinline__ uint32_t p_node(uint32_t k, uint32_t n, uint32_t t, uint32_t i) {
  const uint32_t W = 2 * k, a = t < W ? t : t - W;
  if (a < k) return (t < W ? a : k + a) * (n / 2) + (i - n / 2);
  return k * n + (t < W ? a - k : a) * n + i;
}

// One split level of a batch: nq Q0 nodes and np parity nodes per square out of twice as
// many. grid: x = bq blocks of Q0 lanes, then the parity lanes' blocks; y = square.
// ROOT: the last level (n = 2). The Q0 lanes are the 2k joins: the parity half's digest
// becomes a record in registers and hash_node decides the max namespace as everywhere;
// the parity lanes hash the 2k all-parity roots. Both write their root as k_level does.
template <bool ROOT>
__global__ __launch_bounds__(256) void k_level_split(const uint32_t* __restrict__ qin, uint32_t* __restrict__ qout,
                                                     const uint32_t* __restrict__ pin, uint32_t* __restrict__ pout,
                                                     uint32_t nq, uint32_t np, uint32_t bq, uint32_t k,
                                                     uint32_t* __restrict__ leafd, uint8_t* __restrict__ row_out,
                                                     uint8_t* __restrict__ col_out) {
  const uint32_t sq = blockIdx.y, W = 2 * k;
  if (blockIdx.x < bq) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nq) return;
    uint32_t o[kNodeWords];
    if (ROOT) {
      uint32_t L[kNodeWords], R[kNodeWords], d[8];
      load_node(qin + ((uint64_t)sq * nq + i) * kNodeWords, L);
      load_digest(pin + ((uint64_t)sq * 3 * np + i) * 8, d);
      parity_record(d, R);
      hash_node(L, R, o);
      put_root(o, sq, i < k ? i : W + (i - k), W, leafd, row_out, col_out);
    } else {
      hash_pair(qin + (uint64_t)sq * 2 * nq * kNodeWords, 2 * i, 2 * i + 1, o);
      store_node(qout + ((uint64_t)sq * nq + i) * kNodeWords, o);
    }
  } else {
    const uint32_t i = (blockIdx.x - bq) * 256u + threadIdx.x;
    if (i >= np) return;
    // ROOT: the square's digests are [2k of the joins][2k pairs]
    const uint32_t* in = pin + (ROOT ? (uint64_t)sq * 3 * np + np : (uint64_t)sq * 2 * np) * 8;
    uint32_t dl[8], dr[8], d[8];
    load_digest(in + (uint64_t)i * 16, dl);
    load_digest(in + (uint64_t)i * 16 + 8, dr);
    hash_parity_node<false>(dl, dr, d);
    if (ROOT) {
      uint32_t o[kNodeWords];
      parity_record(d, o);
      put_root(o, sq, i < k ? k + i : W + i, W, leafd, row_out, col_out);
    } else {
      store_digest(pout + ((uint64_t)sq * np + i) * 8, d);
    }
  }
}

// ------------------------------------------------- leaves and level 1 in one lane

// One lane per 2x2 block of EDS cells (rows 2bi, 2bi+1, columns 2bj, 2bj+1): the four
// leaves (9 compressions each), the two row and the two column level-1 nodes over them
// (3 each), written where k_level<false> reads a level of W/2 nodes: out[sq][tree][W/2],
// row trees first. The leaf records never reach memory (W*W records written once and read
// twice), and the leaves-to-level-1 launch goes.
//   Order of work: leaf 00, leaf 01, row node (00,01); leaf 10, column node (00,10);
// leaf 11, column node (01,11), row node (10,11). A leaf is kept across the hashes between
// as its 8 digest words; its namespaces are read from the share again when a record is
// formed (leaf_record). Leaves and nodes run in rolled loops with one leaf_hash and one
// hash_node site: unrolled, the kernel is 32 compression bodies of straight-line code,
// several times the instruction cache, with every wave at another place in it.
//   A wave is an 8x8 tile of blocks (narrower squares: k wide, 64/k block rows): row and
// column nodes both leave it as runs of 8 records, 768 bytes, per tree. The push-order
// check is k_leaf's, per cell.
//   A level-1 node outside Q0 (its left leaf is) is hashed by hash_parity_node from the two
// leaf digests and leaves as a digest into pout; a Q0 node goes through hash_node and leaves
// as a record into out (split levels, above).
//   The tile lies wholly inside or outside Q0 for k >= 16, and there each class has a
// kernel of its own, each wave one tile of its class (quad_tiles.hpp):
//   k_leaf_quad_par : no class tests, no records, no hash_node, no order check: every leaf
//              starts block 0 from kLeafParMid, every node is hash_parity_node with all 64
//              rounds unrolled. Three quarters of a batch's lanes.
//   k_leaf_quad_q0  : every cell is Q0; leaf_hash and hash_node have one form of block 0
//              each (a Q0 share that carries 0xFF*29 is hashed like any other, to the same
//              bytes), and the push-order check as before.
//   k_leaf_quad     : k < 16, where a tile mixes the classes: the class per lane, the
//              wave-uniform parity starts of leaf_hash and hash_node where a wave allows,
//              hash_parity_node with rounds 32..63 rolled. ROOTS: W = 2, the one block's
//              level-1 nodes are the four roots, all through hash_node (out = roots [sq][4],
//              put_root as k_level's last level).
// One kernel for both classes was 64,316 bytes of code against a 64 KB instruction cache
// (hence the rolled rounds) and 133 VGPRs, three waves per SIMD, with every wave using half
// of it. Apart, the parity kernel is 45,396 bytes and 86 VGPRs, the Q0 kernel 33,240 and 152
// (ORDER, no prefetch; profiles/quad_split_isa.txt), both without scratch.
//   Waves per SIMD: the Q0 kernel and the mixed one are built for three (held to four the
// mixed kernel spilled 10 dwords and the headline step was ~2.5 % slower, ~4 % at five,
// ~3 % left alone at two: profiles/r7_leaf_quad_waves.txt). The parity kernel fits four and
// five without a spill and is still built for three: on the headline step four waves were
// 0.7 % slower and five 1.4 %, ranges apart each time (profiles/quad_split_ab.txt).
//   quad_block is the lane's work for all three; C says what the kernel knows of its cells.
template <Cells C, bool ORDER, bool PF, bool ROOTS>
__device__ __forceinline__ void quad_block(const uint8_t* __restrict__ eds, uint32_t k, uint32_t sq, uint32_t bi,
                                           uint32_t bj, uint32_t* __restrict__ out, uint32_t* __restrict__ pout,
                                           int32_t* __restrict__ bad_axis, uint32_t* __restrict__ leafd,
                                           uint8_t* __restrict__ row_out, uint8_t* __restrict__ col_out) {
  static_assert(C == Cells::kAny || !ROOTS, "the roots case is a mixed block");
  const uint32_t W = 2 * k, trees = 2 * W;
  const uint64_t sq_eds = (uint64_t)W * W * kShare;
  const uint32_t* sh00 =
      reinterpret_cast<const uint32_t*>(eds + sq * sq_eds + ((uint64_t)(2 * bi) * W + 2 * bj) * kShare);
  auto in_q0 = [&](uint32_t r, uint32_t c) { return C == Cells::kAny ? (r < k) && (c < k) : C == Cells::kQ0; };
  // leaf digests (SHA state words): dA of cell 00, then, 00 being done with, of cell 11;
  // dB of cell 01, dC of cell 10
  uint32_t dA[8], dB[8], dC[8];
#pragma unroll 1
  for (uint32_t s = 0; s < 4; s++) {  // cell s = (s >> 1, s & 1) of the block
    const uint32_t r = 2 * bi + (s >> 1), c = 2 * bj + (s & 1);
    const uint32_t* sh = sh00 + ((uint64_t)(s >> 1) * W + (s & 1)) * (kShare / 4);
    const bool q0 = in_q0(r, c);
    {
      uint32_t st[8];
      leaf_hash<PF, C>(st, sh, q0);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        if (s == 0 || s == 3) dA[i] = st[i];
        if (s == 1) dB[i] = st[i];
        if (s == 2) dC[i] = st[i];
      }
    }
    // nodes this leaf completes, the leaf being their right child: s = 1: row (00,01);
    // s = 2: column (00,10); s = 3: column (01,11), then row (10,11)
    const uint32_t nn = s == 3 ? 2u : (s ? 1u : 0u);
#pragma unroll 1
    for (uint32_t n = 0; n < nn; n++) {
      const uint32_t lc = s < 3 ? 0u : 1u + n;  // the left child's cell
      const bool row = (s == 1) || (s == 3 && n == 1);
      const uint32_t* shl = sh00 + ((uint64_t)(lc >> 1) * W + (lc & 1)) * (kShare / 4);
      const bool q0l = in_q0(2 * bi + (lc >> 1), 2 * bj + (lc & 1));
      const uint32_t t = row ? r : W + c, idx = row ? bj : bi;  // the node's tree and index in level 1
      auto children = [&](uint32_t (&dl)[8], uint32_t (&dr)[8]) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          dl[i] = lc == 0 ? dA[i] : (lc == 1 ? dB[i] : dC[i]);
          dr[i] = s == 1 ? dB[i] : (s == 2 ? dC[i] : dA[i]);
        }
      };
      if (ROOTS || q0l) {  // k is even: the right child of a Q0 left child is in Q0 too
        uint32_t o[kNodeWords];
        {
          uint32_t L[kNodeWords], R[kNodeWords], dl[8], dr[8];
          children(dl, dr);
          leaf_record(shl, q0l, dl, L);
          leaf_record(sh, q0, dr, R);
          hash_node<C == Cells::kAny>(L, R, o);
        }
        if (ROOTS) {
          store_node(out + (((uint64_t)sq * trees + t) * k + idx) * kNodeWords, o);
          put_root(o, sq, t, W, leafd, row_out, col_out);
        } else {
          store_node(out + ((uint64_t)sq * q_nodes(k, k) + q_node(k, k, t, idx)) * kNodeWords, o);
        }
      } else {
        uint32_t dl[8], dr[8], o[8];
        children(dl, dr);
        hash_parity_node<C == Cells::kAny>(dl, dr, o);
        store_digest(pout + ((uint64_t)sq * p_nodes(k, k) + p_node(k, k, t, idx)) * 8, o);
      }
    }
    // after the hashes, as in k_leaf: done first, the share prefixes stay live across them
    __builtin_amdgcn_sched_barrier(0);
    if (ORDER && q0) {
      if (c > 0 && ns_less(sh, sh - kShare / 4)) atomicMin(bad_axis + sq, (int32_t)r);
      if (r > 0 && ns_less(sh, sh - (uint64_t)W * kShare / 4)) atomicMin(bad_axis + sq, (int32_t)(W + c));
    }
  }
}

// k < 16. grid: x = 256 blocks, y = square.
template <bool ORDER, bool PF, bool ROOTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_leaf_quad(
    const uint8_t* __restrict__ eds, uint32_t k, uint32_t* __restrict__ out, uint32_t* __restrict__ pout,
    int32_t* __restrict__ bad_axis, uint32_t* __restrict__ leafd, uint8_t* __restrict__ row_out,
    uint8_t* __restrict__ col_out) {
  const uint32_t tw = k < 8 ? k : 8u, th = 64 / tw, tiles_x = k / tw;
  const uint32_t g = blockIdx.x * 256u + threadIdx.x, tile = g / 64, l = g % 64;
  const uint32_t bi = (tile / tiles_x) * th + l / tw, bj = (tile % tiles_x) * tw + l % tw;
  if (bi >= k) return;
  quad_block<Cells::kAny, ORDER, PF, ROOTS>(eds, k, blockIdx.y, bi, bj, out, pout, bad_axis, leafd, row_out, col_out);
}

// k >= 16, the Q0 tiles. grid: x = quad::groups_for(quad::q0_tiles(k)), y = square.
template <bool ORDER, bool PF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_leaf_quad_q0(
    const uint8_t* __restrict__ eds, uint32_t k, uint32_t* __restrict__ out, int32_t* __restrict__ bad_axis) {
  const uint32_t g = blockIdx.x * quad::kGroupLanes + threadIdx.x;
  const uint32_t tile = g / quad::kTileLanes, l = g % quad::kTileLanes;
  if (tile >= quad::q0_tiles(k)) return;
  const quad::TilePos at = quad::q0_tile(tile, k);
  quad_block<Cells::kQ0, ORDER, PF, false>(eds, k, blockIdx.y, at.row * quad::kTileSide + l / quad::kTileSide,
                                           at.col * quad::kTileSide + l % quad::kTileSide, out, nullptr, bad_axis,
                                           nullptr, nullptr, nullptr);
}

// k >= 16, the parity tiles. grid: x = quad::groups_for(quad::par_tiles(k)), y = square.
template <bool PF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_leaf_quad_par(
    const uint8_t* __restrict__ eds, uint32_t k, uint32_t* __restrict__ pout) {
  const uint32_t g = blockIdx.x * quad::kGroupLanes + threadIdx.x;
  const uint32_t tile = g / quad::kTileLanes, l = g % quad::kTileLanes;
  if (tile >= quad::par_tiles(k)) return;
  const quad::TilePos at = quad::par_tile(tile, k);
  quad_block<Cells::kParity, false, PF, false>(eds, k, blockIdx.y, at.row * quad::kTileSide + l / quad::kTileSide,
                                               at.col * quad::kTileSide + l % quad::kTileSide, nullptr, pout, nullptr,
                                               nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------ RFC-6962

// rfc_leaf90 (SHA256(0x00 || item90)), rfc_inner (SHA256(0x01 || l || r)) and sha_empty:
// nmt_device.hpp

// One workgroup per item list: items[g][n] 96-byte records -> 32-byte root (BE words in
// out[g*8..]). The 90-byte row / column roots are packed by the root level or k_dah_leaves.
// out_src / host_out (one square, optional): after the DAH, the workgroup copies out_bytes
// (a multiple of 16) from out_src (roots | dah | status, written before the copy) to host_out,
// page-locked host memory, with 16-byte stores: the results cross PCIe inside this launch
// instead of in a separate copy after it.
// dah and status may both lie inside [out_src, out_src + out_bytes) (the one-square path
// copies that block out to host_out after writing it), so neither of the two nor out_src is
// __restrict__: the copy-out loads must see thread 0's dah / status stores.
__global__ __launch_bounds__(1024) void k_merkle(const uint32_t* __restrict__ items, const uint32_t* __restrict__ leafd,
                                                uint32_t n, uint8_t* dah, const int32_t* __restrict__ bad_axis,
                                                int32_t* status, const uint8_t* out_src,
                                                uint8_t* __restrict__ host_out, uint32_t out_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hs[];  // n * 8 words
  const uint32_t g = blockIdx.x;
  const uint32_t* it = items + (uint64_t)g * n * kNodeWords;
  if (leafd) {
    for (uint32_t i = threadIdx.x; i < n * 8; i += blockDim.x) hs[i] = leafd[(uint64_t)g * n * 8 + i];
  } else {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      uint32_t R[kNodeWords], st[8];
      load_node(it + (uint64_t)i * kNodeWords, R);
      rfc_leaf90(R, st);
#pragma unroll
      for (int j = 0; j < 8; j++) hs[i * 8 + j] = st[j];
    }
  }
  __syncthreads();
  uint32_t cnt = n;
  while (cnt > 1) {
    const uint32_t half = cnt / 2;
    uint32_t st[8];
    for (uint32_t base = 0; base < half; base += blockDim.x) {
      const uint32_t i = base + threadIdx.x;
      if (i < half) rfc_inner(hs + (2 * i) * 8, hs + (2 * i + 1) * 8, st);
      __syncthreads();
      if (i < half) {
#pragma unroll
        for (int j = 0; j < 8; j++) hs[i * 8 + j] = st[j];
      }
      __syncthreads();
    }
    if (cnt & 1) {
      if (threadIdx.x < 8) hs[half * 8 + threadIdx.x] = hs[(cnt - 1) * 8 + threadIdx.x];
      __syncthreads();
    }
    cnt = half + (cnt & 1);
  }
  if (threadIdx.x == 0) {
    uint32_t st[8];
    if (n == 0) sha_empty(st);
    else
      for (int j = 0; j < 8; j++) st[j] = hs[j];
    for (int j = 0; j < 8; j++) {
      dah[g * 32 + 4 * j] = (uint8_t)(st[j] >> 24);
      dah[g * 32 + 4 * j + 1] = (uint8_t)(st[j] >> 16);
      dah[g * 32 + 4 * j + 2] = (uint8_t)(st[j] >> 8);
      dah[g * 32 + 4 * j + 3] = (uint8_t)st[j];
    }
    if (status) status[g] = (bad_axis && bad_axis[g] != INT_MAX) ? CEL_EORDER : CEL_OK;
  }
  if (host_out) {
    __threadfence();  // thread 0's dah / status stores before the workgroup reads them back
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(out_src);
    uint4* dst = reinterpret_cast<uint4*>(host_out);
    for (uint32_t i = threadIdx.x; i < out_bytes / 16; i += blockDim.x) dst[i] = src[i];
  }
}

// Threads of a k_merkle workgroup: one per pair of the widest level (each level is one
// round of 2-compression hashes then), 64..1024.
static uint32_t merkle_block(uint32_t n) {
  const uint32_t pairs = ((n / 2 + 63) / 64) * 64;
  return pairs < 64 ? 64u : (pairs > 1024 ? 1024u : pairs);
}

// RFC-6962 leaf digests of n node records, one lane each (k_merkle then starts from them),
// and the records packed to 90 bytes: the first n/2 into row_out, the rest into col_out.
__global__ __launch_bounds__(256) void k_dah_leaves(const uint32_t* __restrict__ items, uint32_t n,
                                                    uint32_t* __restrict__ leafd, uint8_t* __restrict__ row_out,
                                                    uint8_t* __restrict__ col_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t R[kNodeWords], st[8];
  load_node(items + (uint64_t)i * kNodeWords, R);
  rfc_leaf90(R, st);
  uint4* d = reinterpret_cast<uint4*>(leafd + (uint64_t)i * 8);
  d[0] = make_uint4(st[0], st[1], st[2], st[3]);
  d[1] = make_uint4(st[4], st[5], st[6], st[7]);
  const uint32_t half = n / 2;
  uint16_t* r16 = reinterpret_cast<uint16_t*>(i < half ? row_out + (uint64_t)i * kNode : col_out + (uint64_t)(i - half) * kNode);
#pragma unroll
  for (int j = 0; j < 45; j++) r16[j] = (uint16_t)(R[j / 2] >> (16 * (j & 1)));
}

__global__ void k_fill_i32(int32_t* p, uint32_t n, int32_t v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ----------------------------------------------------------------- launchers

void launch_fill_i32(int32_t* p, uint32_t n, int32_t v, uint32_t block, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_i32, dim3((n + block - 1) / block), dim3(block), 0, s, p, n, v);
}

void launch_dah_leaves(const uint32_t* items, uint32_t n, uint32_t* leafd, uint8_t* row_out, uint8_t* col_out,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_dah_leaves, dim3((n + 255) / 256), dim3(256), 0, s, items, n, leafd, row_out, col_out);
}

void launch_merkle(const uint32_t* items, const uint32_t* leafd, uint32_t n, uint32_t lists, uint8_t* dah,
                   const int32_t* bad_axis, int32_t* status, hipStream_t s, const uint8_t* out_src, uint8_t* host_out,
                   uint32_t out_bytes) {
  const size_t lds = (size_t)(n ? n : 1) * 8 * 4;
  hipLaunchKernelGGL(k_merkle, dim3(lists), dim3(merkle_block(n)), lds, s, items, leafd, n, dah, bad_axis, status,
                     out_src, host_out, out_bytes);
}

// Workspace: leaves [nsq][W*W] nodes (one square only) | ping [nsq][2W][W/2] |
//            pong [nsq][2W][W/4] | roots [nsq][2W] nodes | bad_axis [nsq] int32 |
//            DAH leaf digests [nsq][2W][8]
// A batch's split levels live inside ping and pong: level 1's Q records and P digests
// (q[0], p[0]) in ping, level 2's in pong, and so on in turn. Level 1 takes
// nsq * k^2 * (96 + 3 * 32) bytes and up to 255 of alignment, half of ping's
// nsq * (k^2 + k) * 384; level 2 half of that against half of ping's size in pong.
struct CommitWork {
  uint32_t *leaves, *ping, *pong, *roots, *leafd;
  uint32_t *q[2], *p[2];
  int32_t* bad;
  size_t size;
};

// One square is committed for its latency (a block's header, a repair's check): k_leaf
// and k_level<true> put 4k^2 lanes on a chain of 9 + 3 compressions. k_leaf_quad has k^2
// lanes on a chain of 48, which at k = 128 leaves three SIMDs of four without a wave. A
// batch fills the device either way, and there the quad kernel's saved traffic counts.
static bool quad_path(uint32_t nsq) { return nsq > 1; }

static CommitWork commit_work(void* work, uint32_t k, uint32_t nsq) {
  const size_t W = 2 * (size_t)k, nb = kNodeWords * 4;
  Carver c(work);
  CommitWork w;
  w.leaves = c.take<uint32_t>(quad_path(nsq) ? 0 : nsq * W * W * nb);
  w.ping = c.take<uint32_t>(nsq * 2 * W * (W / 2 + 1) * nb);
  w.pong = c.take<uint32_t>(nsq * 2 * W * (W / 4 + 1) * nb);
  w.roots = c.take<uint32_t>(nsq * 2 * W * nb);
  w.bad = c.take<int32_t>((size_t)nsq * 4 + 4);
  w.leafd = c.take<uint32_t>(nsq * 2 * W * 32);
  w.size = c.size();
  for (uint32_t i = 0; i < 2; i++) {  // level 1 + i: k >> i nodes per tree
    Carver a(i ? w.pong : w.ping);
    w.q[i] = a.take<uint32_t>((size_t)nsq * q_nodes(k, k >> i) * nb);
    w.p[i] = a.take<uint32_t>((size_t)nsq * p_nodes(k, k >> i) * 32);
  }
  return w;
}

size_t nmt_workspace_size(uint32_t k, uint32_t nsq) { return commit_work(nullptr, k, nsq).size; }

// k_leaf over cells [c0, c1) of nsq squares: the leaf records into `leaves` ([nsq][W * W]), the
// push-order flags into `bad`. The commit's workspace and the tree index (nmt_prove.hpp) each
// pass their own places.
static void launch_leaf(const uint8_t* eds, uint32_t k, uint32_t nsq, uint32_t* leaves, int32_t* bad,
                        bool order_check, uint32_t c0, uint32_t c1, hipStream_t s) {
  dim3 gl((c1 - c0 + 255) / 256, nsq);
  dispatch_order_pf(order_check, latency_bound((uint64_t)(c1 - c0) * nsq), [&](auto order, auto pf) {
    hipLaunchKernelGGL((k_leaf<decltype(order)::value, decltype(pf)::value>), gl, dim3(256), 0, s, eds, k, leaves,
                       bad, c0, c1);
  });
}

// k_level: the level of nin / 2 nodes per tree over `src` (the leaf records if from_leaves,
// else a level of nin nodes per tree) into `out`; ld, ro, co: the root level's outputs.
static void launch_level(bool from_leaves, const uint32_t* src, uint32_t* out, uint32_t W, uint32_t nin,
                         uint32_t nsq, uint32_t* ld, uint8_t* ro, uint8_t* co, hipStream_t s) {
  const uint32_t trees = 2 * W;
  dim3 g((trees * (nin / 2) + 255) / 256, nsq);
  if (from_leaves) hipLaunchKernelGGL(k_level<true>, g, dim3(256), 0, s, src, out, W, nin, trees, ld, ro, co);
  else hipLaunchKernelGGL(k_level<false>, g, dim3(256), 0, s, src, out, W, nin, trees, ld, ro, co);
}

hipError_t launch_commit_leaves(const uint8_t* eds, uint32_t k, uint32_t nsq, void* work, bool order_check,
                                uint32_t row0, uint32_t row1, bool init_bad, hipStream_t s) {
  if (quad_path(nsq)) return hipErrorInvalidValue;  // no leaf area in that workspace
  const uint32_t W = 2 * k;
  const CommitWork w = commit_work(work, k, nsq);
  const Range r("nmt.leaf");
  if (init_bad) launch_fill_i32(w.bad, nsq, INT_MAX, 256, s);
  const uint32_t c0 = row0 * W, c1 = row1 * W;
  if (c1 <= c0) return hipGetLastError();
  launch_leaf(eds, k, nsq, w.leaves, w.bad, order_check, c0, c1, s);
  return hipGetLastError();
}

// The DAH over the roots' leaf digests (written by the root level), and the status.
static hipError_t commit_dah(const CommitWork& w, uint32_t k, uint32_t nsq, uint8_t* row_roots, uint8_t* dah,
                             int32_t* status, hipStream_t s, uint8_t* host_out, uint32_t out_bytes) {
  const Range r("dah");
  if (dah)
    launch_merkle(w.roots, w.leafd, 4 * k, nsq, dah, w.bad, status, s, host_out ? row_roots : nullptr, host_out,
                  out_bytes);
  return hipGetLastError();
}

// One square's tree levels from the leaf area down to the roots, then the DAH. One launch
// per level, all 4k trees at once: every lane hashes one node, no idle lanes. The last
// level writes the root records, packed into row_roots / col_roots.
static hipError_t commit_levels(const CommitWork& w, uint32_t k, uint32_t nsq, uint8_t* row_roots,
                                uint8_t* col_roots, uint8_t* dah, int32_t* status, hipStream_t s, uint8_t* host_out,
                                uint32_t out_bytes) {
  const uint32_t W = 2 * k;
  uint32_t nin = W;
  const uint32_t* src = w.leaves;
  uint32_t* dst = w.ping;
  bool first = true;
  roctxRangePushA("nmt.levels");
  while (nin > 1) {
    const uint32_t nout = nin / 2;
    uint32_t* out = (nout == 1) ? w.roots : dst;
    uint32_t* ld = (nout == 1 && dah) ? w.leafd : nullptr;  // dah == nullptr: roots only
    uint8_t* ro = (nout == 1) ? row_roots : nullptr;
    uint8_t* co = (nout == 1) ? col_roots : nullptr;
    launch_level(first, src, out, W, nin, nsq, ld, ro, co, s);
    first = false;
    src = out;
    dst = (dst == w.ping) ? w.pong : w.ping;
    nin = nout;
  }
  roctxRangePop();
  return commit_dah(w, k, nsq, row_roots, dah, status, s, host_out, out_bytes);
}

hipError_t launch_commit_trees(uint32_t k, uint32_t nsq, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                               int32_t* status, void* work, hipStream_t s, uint8_t* host_out, uint32_t out_bytes) {
  if (quad_path(nsq)) return hipErrorInvalidValue;
  return commit_levels(commit_work(work, k, nsq), k, nsq, row_roots, col_roots, dah, status, s, host_out, out_bytes);
}

// Leaves and level 1 of every square: level 1's Q records and P digests into q[0] / p[0], by
// k_leaf_quad_q0 and k_leaf_quad_par for k >= 16, by the one k_leaf_quad below; at k = 1 the
// roots.
static hipError_t launch_commit_quads(const uint8_t* eds, uint32_t k, uint32_t nsq, const CommitWork& w,
                                      bool order_check, uint8_t* row_roots, uint8_t* col_roots, bool want_dah,
                                      hipStream_t s) {
  const Range r("nmt.leaf");
  launch_fill_i32(w.bad, nsq, INT_MAX, 256, s);
  const uint32_t tw = k < 8 ? k : 8u, th = 64 / tw;  // a wave's tile of blocks, as in the kernel
  const uint64_t lanes = (uint64_t)((k + th - 1) / th) * (k / tw) * 64;
  dim3 g((uint32_t)((lanes + 255) / 256), nsq);
  if (k == 1) {
    uint32_t* ld = want_dah ? w.leafd : nullptr;
    if (order_check)
      hipLaunchKernelGGL((k_leaf_quad<true, false, true>), g, dim3(256), 0, s, eds, k, w.roots, nullptr, w.bad, ld,
                         row_roots, col_roots);
    else
      hipLaunchKernelGGL((k_leaf_quad<false, false, true>), g, dim3(256), 0, s, eds, k, w.roots, nullptr, w.bad, ld,
                         row_roots, col_roots);
    return hipGetLastError();
  }
  if (!quad::split_width(k)) {  // a wave's tile mixes Q0 and parity blocks
    dispatch_order_pf(order_check, latency_bound(lanes * nsq), [&](auto order, auto pf) {
      hipLaunchKernelGGL((k_leaf_quad<decltype(order)::value, decltype(pf)::value, false>), g, dim3(256), 0, s, eds,
                         k, w.q[0], w.p[0], w.bad, nullptr, nullptr, nullptr);
    });
    return hipGetLastError();
  }
  // A kernel per tile class, each with its own code size and register budget. Each launch
  // takes the prefetching leaf hash by its own lane count: the two run one after the other.
  const uint32_t gq = quad::groups_for(quad::q0_tiles(k)), gp = quad::groups_for(quad::par_tiles(k));
  dispatch_order_pf(order_check, latency_bound((uint64_t)gq * quad::kGroupLanes * nsq), [&](auto order, auto pf) {
    hipLaunchKernelGGL((k_leaf_quad_q0<decltype(order)::value, decltype(pf)::value>), dim3(gq, nsq),
                       dim3(quad::kGroupLanes), 0, s, eds, k, w.q[0], w.bad);
  });
  dispatch_order_pf(false, latency_bound((uint64_t)gp * quad::kGroupLanes * nsq), [&](auto, auto pf) {
    hipLaunchKernelGGL((k_leaf_quad_par<decltype(pf)::value>), dim3(gp, nsq), dim3(quad::kGroupLanes), 0, s, eds, k,
                       w.p[0]);
  });
  return hipGetLastError();
}

// A batch's split levels from level 1 (k nodes per tree in q[0] / p[0]; k >= 2) down to the
// roots: one launch per level with the Q0 lanes and the parity lanes in block ranges of
// their own, the last one the joins and the all-parity roots.
static hipError_t commit_levels_split(const CommitWork& w, uint32_t k, uint32_t nsq, uint8_t* row_roots,
                                      uint8_t* col_roots, bool want_dah, hipStream_t s) {
  const Range r("nmt.levels");
  uint32_t at = 0;
  for (uint32_t n = k; n > 2; n /= 2, at ^= 1) {
    const uint32_t nq = q_nodes(k, n / 2), np = p_nodes(k, n / 2), bq = (nq + 255) / 256;
    hipLaunchKernelGGL(k_level_split<false>, dim3(bq + (np + 255) / 256, nsq), dim3(256), 0, s, w.q[at], w.q[at ^ 1],
                       w.p[at], w.p[at ^ 1], nq, np, bq, k, nullptr, nullptr, nullptr);
  }
  const uint32_t nr = 2 * k, bq = (nr + 255) / 256;  // 2k joins, 2k all-parity roots
  hipLaunchKernelGGL(k_level_split<true>, dim3(2 * bq, nsq), dim3(256), 0, s, w.q[at], nullptr, w.p[at], nullptr, nr,
                     nr, bq, k, want_dah ? w.leafd : nullptr, row_roots, col_roots);
  return hipGetLastError();
}

// The tree index of one square (nmt_prove.hpp): the single-square commit's launches with
// every level kept, level l written at its own place in d_index. A caller that wants no DAH
// still gets its status: the DAH then goes to the index's tail.
hipError_t launch_tree_index(const uint8_t* eds, uint32_t k, void* d_index, uint8_t* row_roots, uint8_t* col_roots,
                             uint8_t* dah, int32_t* status, bool order_check, hipStream_t s) {
  const prove::IndexLayout x = prove::index_layout(k);
  uint8_t* base = static_cast<uint8_t*>(d_index);
  auto level = [&](uint32_t l) { return reinterpret_cast<uint32_t*>(base + x.level_off[l]); };
  uint32_t* leafd = reinterpret_cast<uint32_t*>(base + x.leafd_off);
  int32_t* bad = reinterpret_cast<int32_t*>(base + x.bad_off);
  if (!dah) dah = base + x.dah_off;
  {
    const Range r("index.leaf");
    launch_fill_i32(bad, 1, INT_MAX, 256, s);
    launch_leaf(eds, k, 1, level(0), bad, order_check, 0, x.W * x.W, s);
  }
  {
    const Range r("index.levels");
    for (uint32_t l = 1; l <= x.L; l++) {
      const bool root = l == x.L;
      launch_level(l == 1, level(l - 1), level(l), x.W, x.W >> (l - 1), 1, root ? leafd : nullptr,
                   root ? row_roots : nullptr, root ? col_roots : nullptr, s);
    }
  }
  const Range r("dah");
  launch_merkle(level(x.L), leafd, 2 * x.W, 1, dah, bad, status, s, nullptr, nullptr, 0);
  return hipGetLastError();
}

// ------------------------------------------------------------- the batch tree index
//
// The tree index of n squares in one launch per step (nmt_prove.hpp: n single-square indexes
// back to back). These are k_leaf, k_level and k_merkle with the square's stride on both sides
// the index's size: square blockIdx.y reads and writes inside its own slice, every level at
// its slice_level_off, the leaf digests, the push-order flag, the DAH of a caller that wants none
// and the status in the slice's tail. They are kernels of their own, so the instantiations the
// commit and the single-square index launch take no new parameter; the hashing (make_leaf_node,
// hash_pair, put_root, rfc_*) is shared.
//
// Bounds. The host checks k (a power of two up to 512) and nsq (1 .. prove::kMaxSquares, the
// grid's y or x extent) and that the index holds nsq * index_bytes(W) bytes, the cells
// nsq * W * W * 512, the roots nsq * 2W * 90 and a caller's DAH nsq * 32. A lane's cell is below
// W * W and its level-l node below 2W * (W >> l), so with record = index_level_rec(W, l) + node
// every record is below index_records(W); the tail offsets are below index_bytes(W). All of
// them are added to slice = blockIdx * index_bytes(W) in 64 bits.

__global__ __launch_bounds__(256) void k_index_bad_init(uint8_t* __restrict__ index, uint64_t slice, uint64_t bad_off,
                                                        uint32_t nsq) {
  const uint32_t sq = blockIdx.x * 256u + threadIdx.x;
  if (sq < nsq) *reinterpret_cast<int32_t*>(index + (uint64_t)sq * slice + bad_off) = INT_MAX;
}

// grid: x = block of 256 cells, y = square. The leaf records of square y into level 0 of its slice.
template <bool ORDER, bool PF>
__global__ __launch_bounds__(256) void k_leaf_index(const uint8_t* __restrict__ eds, uint32_t k,
                                                    uint8_t* __restrict__ index, uint64_t slice, uint64_t bad_off) {
  const uint32_t W = 2 * k;
  const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
  if (cell >= W * W) return;
  const uint32_t r = cell / W, c = cell % W;
  uint8_t* base = index + (uint64_t)blockIdx.y * slice;
  const uint32_t* sh =
      reinterpret_cast<const uint32_t*>(eds + prove::eds_base(W, blockIdx.y) + (uint64_t)cell * kShare);
  const bool q0 = (r < k) && (c < k);
  {
    uint32_t nd[kNodeWords];
    make_leaf_node<PF>(sh, q0, nd);
    store_node(reinterpret_cast<uint32_t*>(base) + (uint64_t)cell * kNodeWords, nd);
  }
  __builtin_amdgcn_sched_barrier(0);  // as in k_leaf: the order check after the hash
  if (ORDER && q0) {
    int32_t* bad = reinterpret_cast<int32_t*>(base + bad_off);
    if (c > 0 && ns_less(sh, sh - kShare / 4)) atomicMin(bad, (int32_t)r);
    if (r > 0 && ns_less(sh, sh - (uint64_t)W * kShare / 4)) atomicMin(bad, (int32_t)(W + c));
  }
}

// k_level inside a slice: the level at in_off (nin nodes per tree, or the leaf records) into the
// level at out_off. At the root level (row_out != nullptr) also the packed roots, [nsq][W][90]
// each, and the roots' leaf digests at leafd_off.
template <bool FROM_LEAVES>
__global__ __launch_bounds__(256) void k_level_index(uint8_t* __restrict__ index, uint64_t slice, uint64_t in_off,
                                                     uint64_t out_off, uint32_t W, uint32_t nin, uint32_t trees,
                                                     uint64_t leafd_off, uint8_t* __restrict__ row_out,
                                                     uint8_t* __restrict__ col_out) {
  const uint32_t nout = nin / 2;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= trees * nout) return;
  const uint32_t t = idx / nout, j = idx % nout;
  uint8_t* base = index + (uint64_t)blockIdx.y * slice;
  uint64_t li, ri;
  if (FROM_LEAVES) {
    if (t < W) { li = (uint64_t)t * W + 2 * j; ri = li + 1; }
    else { li = (uint64_t)(2 * j) * W + (t - W); ri = li + W; }
  } else {
    li = (uint64_t)t * nin + 2 * j;
    ri = li + 1;
  }
  uint32_t o[kNodeWords];
  hash_pair(reinterpret_cast<const uint32_t*>(base + in_off), li, ri, o);
  store_node(reinterpret_cast<uint32_t*>(base + out_off) + (uint64_t)idx * kNodeWords, o);
  if (row_out) {
    const uint64_t roots = (uint64_t)blockIdx.y * W * kNode;
    put_root(o, 0, t, W, reinterpret_cast<uint32_t*>(base + leafd_off), row_out + roots, col_out + roots);
  }
}

// k_merkle for square blockIdx.x of a batch index: RFC-6962 over the n = 4k leaf digests of its
// slice. The DAH to dah + 32 * square, or to the slice's tail; with want_status the status to
// the slice's tail and to status[square].
__global__ __launch_bounds__(1024) void k_merkle_index(uint8_t* __restrict__ index, uint64_t slice, uint64_t leafd_off,
                                                       uint32_t n, uint8_t* __restrict__ dah, uint64_t dah_off,
                                                       uint64_t bad_off, uint64_t status_off,
                                                       int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hs[];  // n * 8 words
  uint8_t* base = index + (uint64_t)blockIdx.x * slice;
  const uint32_t* leafd = reinterpret_cast<const uint32_t*>(base + leafd_off);
  for (uint32_t i = threadIdx.x; i < n * 8; i += blockDim.x) hs[i] = leafd[i];
  __syncthreads();
  uint32_t cnt = n;  // a power of two, at least 4
  while (cnt > 1) {
    const uint32_t half = cnt / 2;
    uint32_t st[8];
    for (uint32_t b = 0; b < half; b += blockDim.x) {
      const uint32_t i = b + threadIdx.x;
      if (i < half) rfc_inner(hs + (2 * i) * 8, hs + (2 * i + 1) * 8, st);
      __syncthreads();
      if (i < half) {
#pragma unroll
        for (int j = 0; j < 8; j++) hs[i * 8 + j] = st[j];
      }
      __syncthreads();
    }
    cnt = half;
  }
  if (threadIdx.x == 0) {
    uint8_t* out = dah ? dah + (uint64_t)blockIdx.x * 32 : base + dah_off;
    for (int j = 0; j < 8; j++) {
      const uint32_t v = hs[j];
      out[4 * j] = (uint8_t)(v >> 24);
      out[4 * j + 1] = (uint8_t)(v >> 16);
      out[4 * j + 2] = (uint8_t)(v >> 8);
      out[4 * j + 3] = (uint8_t)v;
    }
    if (status) {
      const int32_t st = *reinterpret_cast<const int32_t*>(base + bad_off) != INT_MAX ? CEL_EORDER : CEL_OK;
      *reinterpret_cast<int32_t*>(base + status_off) = st;
      status[blockIdx.x] = st;
    }
  }
}

hipError_t launch_tree_index_batch(const uint8_t* eds, uint32_t k, uint32_t nsq, void* d_index, uint8_t* row_roots,
                                   uint8_t* col_roots, uint8_t* dah, int32_t* status, bool order_check,
                                   hipStream_t s) {
  if (!nsq) return hipSuccess;
  if (nsq > prove::kMaxSquares) return hipErrorInvalidValue;
  const prove::IndexLayout x = prove::index_layout(k);
  const uint32_t W = x.W;
  const uint64_t slice = prove::index_bytes(W);
  uint8_t* index = static_cast<uint8_t*>(d_index);
  {
    const Range r("index_batch.leaf");
    hipLaunchKernelGGL(k_index_bad_init, dim3((nsq + 255) / 256), dim3(256), 0, s, index, slice,
                       prove::slice_bad_off(W), nsq);
    dim3 gl((W * W + 255) / 256, nsq);
    dispatch_order_pf(order_check, latency_bound((uint64_t)W * W * nsq), [&](auto order, auto pf) {
      hipLaunchKernelGGL((k_leaf_index<decltype(order)::value, decltype(pf)::value>), gl, dim3(256), 0, s, eds, k, index,
                         slice, prove::slice_bad_off(W));
    });
  }
  {
    const Range r("index_batch.levels");
    const uint32_t trees = 2 * W;
    for (uint32_t l = 1; l <= x.L; l++) {
      const bool root = l == x.L;
      const uint32_t nin = W >> (l - 1);
      dim3 g((trees * (nin / 2) + 255) / 256, nsq);
      const uint64_t in_off = prove::slice_level_off(W, l - 1), out_off = prove::slice_level_off(W, l);
      uint8_t* ro = root ? row_roots : nullptr;
      uint8_t* co = root ? col_roots : nullptr;
      if (l == 1)
        hipLaunchKernelGGL(k_level_index<true>, g, dim3(256), 0, s, index, slice, in_off, out_off, W, nin, trees,
                           prove::slice_leafd_off(W), ro, co);
      else
        hipLaunchKernelGGL(k_level_index<false>, g, dim3(256), 0, s, index, slice, in_off, out_off, W, nin, trees,
                           prove::slice_leafd_off(W), ro, co);
    }
  }
  const Range r("index_batch.dah");
  const uint32_t n = 2 * W;
  hipLaunchKernelGGL(k_merkle_index, dim3(nsq), dim3(merkle_block(n)), (size_t)n * 32, s, index, slice,
                     prove::slice_leafd_off(W), n, dah, prove::slice_dah_off(W), prove::slice_bad_off(W),
                     prove::slice_status_off(W), status);
  return hipGetLastError();
}

hipError_t launch_commit(const uint8_t* eds, uint32_t k, uint32_t nsq, uint8_t* row_roots, uint8_t* col_roots,
                         uint8_t* dah, int32_t* status, void* work, bool order_check, hipStream_t s) {
  if (!quad_path(nsq)) {
    hipError_t e = launch_commit_leaves(eds, k, nsq, work, order_check, 0, 2 * k, true, s);
    if (e == hipSuccess) e = launch_commit_trees(k, nsq, row_roots, col_roots, dah, status, work, s);
    return e;
  }
  const CommitWork w = commit_work(work, k, nsq);
  hipError_t e = launch_commit_quads(eds, k, nsq, w, order_check, row_roots, col_roots, dah != nullptr, s);
  if (e == hipSuccess && k > 1) e = commit_levels_split(w, k, nsq, row_roots, col_roots, dah != nullptr, s);
  if (e == hipSuccess) e = commit_dah(w, k, nsq, row_roots, dah, status, s, nullptr, 0);
  return e;
}


}  // namespace cel
