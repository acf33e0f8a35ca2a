// Namespace queries on the tree index of a resident square (nmt_namespace.hpp): for n
// namespaces and the 2k rows of the square, which rows hold the namespace (or prove that they
// do not), where, and the proofs. Replaces a walk over downloaded trees on the host
// (proof.axis_trees, then proof.nmt_prove_namespace per row).
//
// k_ns_find     one wave per namespace and 64 rows, four waves per workgroup. Lane r reads the
//               root record of its row (level L of the index) and writes an empty pair when the
//               namespace is outside the root's range: of n * 2k pairs all but a few end here,
//               64 to a wave (a wave per pair, the first version, spent 55 us at n = 1024 on
//               dispatching 262,144 waves that read one root each). The rows that remain are
//               taken one after the other by the whole wave: lane c compares the min namespace
//               of leaves c, c + 64, ... with the namespace (8 big-endian words, the 29-byte
//               lexicographic order); two ballots per turn give the counts of leaves below and
//               at-or-below it, and nsq::classify the pair. Every pair is written exactly once.
// k_ns_sums     the three counters (entries, nodes, leaves) of each block of 256 pairs
// k_ns_scan     one workgroup: the exclusive prefix sum of the block sums in place, each lane a
//               contiguous slice; the totals
// k_ns_compact  the same blocks again: a lane's exclusive prefix inside its block plus the
//               block's base is its entry's place and the place of its nodes and shares. The
//               order is (namespace index, row), the sums do not depend on any schedule.
// k_ns_emit     k_prove's scheme (nmt_prove.hip), one wave per entry: lane j works out where
//               node j lies, the wave copies the packed nodes as coalesced halfwords and the
//               shares as 16-byte words. The last node of an absence entry is the level-0
//               record of its leaf.
//
// Bounds. k and n are checked on the host (api_namespace.cpp: k a width of the index, n * 2k
// below 2^32), and the workspace is carved for them (nsq::carve). k_ns_find reads record
// row * W + c with row, c < W, and the root record of row < W: inside the index whatever the
// cells hold. Its counts are counts of lanes with c < W, so lt <= le <= W, and nsq::classify
// yields an entry only when lt < W: start < end <= W for an inclusion entry and start = lt < W
// for an absence entry, on any cells, ordered or not. k_ns_emit reads the records
// prove::index_record names for such a range (below the record count, as in k_prove), the
// leaf record row * W + start, and cells (row, start .. end - 1). It writes entry e's nodes at
// [node0, node0 + nnodes) and shares at [leaf0, leaf0 + (end - start)): the prefix sums of
// exactly those counts, which the plan call has given the caller to size the outputs with. It
// runs over no more entries than the plan holds (head->totals.entries), whatever the caller passes.
//
// Over a batch index (k_ns_find_squares, k_ns_compact_squares, k_ns_emit_squares; the sums and
// the scan are the same kernels). A query is a (square, namespace) pair; the host checks every
// square < n_squares <= prove::kMaxSquares before it uploads the table (api_namespace.cpp), and
// the caller's index holds n_squares slices and its cells n_squares squares. k_ns_find_squares
// reads what k_ns_find reads, inside the slice at prove::slice_base of the query's square;
// pairs, sums and entries are indexed by query and row as before, so the workspace argument is
// unchanged and the order stays (query, row), fixed by pair number. k_ns_compact_squares reads
// row ns_idx < n of the query table. k_ns_emit_squares takes the square from the entry, skips
// an entry whose square is not below the n_squares it was launched for, and otherwise reads
// what k_ns_emit reads inside that square's cells and slice; both bases are 64-bit. A plan's
// head says which sort it is, and each emit kernel does nothing on the other sort.
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "nmt_namespace.hpp"

namespace cel {

using nsq::Pair;
using nsq::Request;
using nsq::Sums;

namespace {

constexpr uint32_t kWavesPerGroup = 4;

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_amdgcn_perm(0u, x, 0x00010203u); }

// The min namespace (bytes 0 .. 28) and max namespace (29 .. 57) of a record's first 15 dwords
// as 8 big-endian compare words.
__device__ __forceinline__ void min_be(const uint32_t (&r)[8], uint32_t (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = bswap(r[i]);
  o[7] = r[7] << 24;
}
// -1, 0, 1: a below, equal to, above b
__device__ __forceinline__ int ns_cmp(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  int res = 0;
#pragma unroll
  for (int i = 0; i < 8; i++)
    if (res == 0 && a[i] != b[i]) res = a[i] > b[i] ? 1 : -1;
  return res;
}

// One wave of the find: query qi (its 8 raw words in `raw`) against rows row0 .. row0 + 63 of the
// square whose index is at `index`.
__device__ __forceinline__ void ns_find_rows(const uint32_t* __restrict__ index, uint32_t W, uint32_t L,
                                             const uint32_t (&raw)[8], uint32_t qi, uint32_t row0,
                                             Pair* __restrict__ pairs, uint32_t lane) {
  uint32_t nid[8];
  min_be(raw, nid);
  // lane r: does the root of row row0 + r hold the namespace? An empty pair if not.
  const uint32_t myrow = row0 + lane;
  bool inside = false;
  if (myrow < W) {
    const uint4* root = reinterpret_cast<const uint4*>(index + prove::index_record(W, 0, myrow, L, 0) * kNodeWords);
    const uint4 a = root[0], b = root[1], c = root[2], d = root[3];
    const uint32_t r[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    uint32_t rmin[8], rmax[8];
#pragma unroll
    for (int i = 0; i < 7; i++) {
      rmin[i] = bswap(r[i]);
      rmax[i] = bswap(__builtin_amdgcn_alignbyte(r[8 + i], r[7 + i], 1));
    }
    rmin[7] = r[7] << 24;
    rmax[7] = (r[14] >> 8) << 24;
    inside = ns_cmp(rmin, nid) <= 0 && ns_cmp(nid, rmax) <= 0;
    if (!inside) pairs[(uint64_t)qi * W + myrow] = Pair{0, 0, 0, 0};
  }
  // the rows that do, one after the other, the whole wave on each: the mask is the wave's
  for (uint64_t todo = __ballot(inside); todo; todo &= todo - 1) {
    const uint32_t row = row0 + (uint32_t)__builtin_ctzll(todo);
    uint32_t lt = 0, le = 0;
    const uint32_t* leaves = index + (uint64_t)row * W * kNodeWords;
    // every lane takes every turn: the ballots count the lanes whose leaf exists
    for (uint32_t base = 0; base < W; base += 64) {
      const uint32_t c = base + lane;
      int cmp = 1;
      if (c < W) {
        const uint4* q = reinterpret_cast<const uint4*>(leaves + (uint64_t)c * kNodeWords);
        const uint4 a = q[0], b = q[1];
        const uint32_t r[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t m[8];
        min_be(r, m);
        cmp = ns_cmp(m, nid);
      }
      lt += (uint32_t)__popcll(__ballot(cmp < 0));
      le += (uint32_t)__popcll(__ballot(cmp <= 0));
    }
    if (lane == 0) pairs[(uint64_t)qi * W + row] = nsq::classify(true, lt, le, W);
  }
}

__global__ __launch_bounds__(256) void k_ns_find(const uint32_t* __restrict__ index, uint32_t W, uint32_t L,
                                                 const uint32_t* __restrict__ ns, uint32_t n,
                                                 Pair* __restrict__ pairs) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t groups = (W + 63u) / 64u;  // of 64 rows, per namespace
  // n * groups <= n * W < 2^32
  const uint64_t g64 = (uint64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (g64 >= (uint64_t)n * groups) return;
  const uint32_t g = __builtin_amdgcn_readfirstlane((uint32_t)g64);
  const uint32_t qi = g / groups, row0 = (g - qi * groups) * 64u;
  uint32_t raw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) raw[i] = ns[(uint64_t)qi * 8 + i];
  ns_find_rows(index, W, L, raw, qi, row0, pairs, lane);
}

// k_ns_find over a batch index: query qi is a (square, namespace) pair, the square in the three
// bytes that pad its namespace to 32 (nsq::query_square), and the wave reads the root level and
// the leaves of that square's slice.
__global__ __launch_bounds__(256) void k_ns_find_squares(const uint8_t* __restrict__ index, uint32_t W, uint32_t L,
                                                         const uint32_t* __restrict__ ns, uint32_t n,
                                                         Pair* __restrict__ pairs) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t groups = (W + 63u) / 64u;
  const uint64_t g64 = (uint64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (g64 >= (uint64_t)n * groups) return;
  const uint32_t g = __builtin_amdgcn_readfirstlane((uint32_t)g64);
  const uint32_t qi = g / groups, row0 = (g - qi * groups) * 64u;
  uint32_t raw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) raw[i] = ns[(uint64_t)qi * 8 + i];
  const uint32_t sq = nsq::query_square(raw[7]);
  ns_find_rows(reinterpret_cast<const uint32_t*>(index + prove::slice_base(W, sq)), W, L, raw, qi, row0, pairs, lane);
}

// The counters of pair p; zero beyond the table.
__device__ __forceinline__ void pair_counts(const Pair* __restrict__ pairs, uint64_t p, uint64_t npairs, uint32_t L,
                                            Pair& pr, uint32_t& e, uint32_t& nn, uint32_t& nl) {
  pr = Pair{0, 0, 0, 0};
  if (p < npairs) pr = pairs[p];
  e = pr.entry ? 1u : 0u;
  nn = nsq::entry_nodes(L, pr);
  nl = nsq::entry_leaves(pr);
}

// Inclusive prefix sums of (a, b, c) over the 256 lanes of a workgroup, in lane order; the
// workgroup's totals in tot (every lane). sh: 4 * 3 words.
__device__ __forceinline__ void block_scan3(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t (&tot)[3], uint32_t* sh) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t ta = (uint32_t)__shfl_up((int)a, d, 64), tb = (uint32_t)__shfl_up((int)b, d, 64),
                   tc = (uint32_t)__shfl_up((int)c, d, 64);
    if (lane >= (uint32_t)d) {
      a += ta;
      b += tb;
      c += tc;
    }
  }
  if (lane == 63) {
    sh[wave * 3] = a;
    sh[wave * 3 + 1] = b;
    sh[wave * 3 + 2] = c;
  }
  __syncthreads();
  tot[0] = tot[1] = tot[2] = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWavesPerGroup; w++) {
    if (w < wave) {
      a += sh[w * 3];
      b += sh[w * 3 + 1];
      c += sh[w * 3 + 2];
    }
    tot[0] += sh[w * 3];
    tot[1] += sh[w * 3 + 1];
    tot[2] += sh[w * 3 + 2];
  }
}

__global__ __launch_bounds__(256) void k_ns_sums(const Pair* __restrict__ pairs, uint64_t npairs, uint32_t L,
                                                 Sums* __restrict__ block_sums) {
  __shared__ uint32_t sh[kWavesPerGroup * 3];
  Pair pr;
  uint32_t e, nn, nl, tot[3];
  pair_counts(pairs, (uint64_t)blockIdx.x * nsq::kScanBlock + threadIdx.x, npairs, L, pr, e, nn, nl);
  block_scan3(e, nn, nl, tot, sh);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = Sums{tot[0], tot[1], tot[2]};
}

__global__ __launch_bounds__(256) void k_ns_scan(Sums* __restrict__ block_sums, uint64_t blocks, uint32_t W,
                                                 nsq::Head* __restrict__ head) {
  __shared__ Sums part[256];
  const uint64_t per = (blocks + 255) / 256;
  const uint64_t b0 = (uint64_t)threadIdx.x * per < blocks ? (uint64_t)threadIdx.x * per : blocks;
  const uint64_t b1 = b0 + per < blocks ? b0 + per : blocks;
  Sums mine{0, 0, 0};
  for (uint64_t b = b0; b < b1; b++) {
    const Sums v = block_sums[b];
    mine.entries += v.entries;
    mine.nodes += v.nodes;
    mine.leaves += v.leaves;
  }
  part[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    Sums run{0, 0, 0};
    for (uint32_t t = 0; t < 256; t++) {
      const Sums v = part[t];
      part[t] = run;
      run.entries += v.entries;
      run.nodes += v.nodes;
      run.leaves += v.leaves;
    }
    head->totals = run;
    head->W = W;
  }
  __syncthreads();
  Sums run = part[threadIdx.x];
  for (uint64_t b = b0; b < b1; b++) {
    const Sums v = block_sums[b];
    block_sums[b] = run;
    run.entries += v.entries;
    run.nodes += v.nodes;
    run.leaves += v.leaves;
  }
}

// A block of the compaction. SQUARES: the plan is over a batch index, and the entry takes its
// query's square above its kind (nsq::entry_kind / nsq::entry_square) from the query table ns.
template <bool SQUARES>
__device__ __forceinline__ void ns_compact_block(const Pair* __restrict__ pairs, uint64_t npairs, uint32_t W,
                                                 uint32_t L, const Sums* __restrict__ block_sums,
                                                 const uint32_t* __restrict__ ns, Request* __restrict__ req,
                                                 uint32_t* sh) {
  const uint64_t p = (uint64_t)blockIdx.x * nsq::kScanBlock + threadIdx.x;
  Pair pr;
  uint32_t e, nn, nl, tot[3];
  pair_counts(pairs, p, npairs, L, pr, e, nn, nl);
  uint32_t ie = e, in = nn, il = nl;
  block_scan3(ie, in, il, tot, sh);
  if (!e) return;
  const Sums base = block_sums[blockIdx.x];
  // the entry's place is below the number of pairs, the size of req
  Request r;
  r.ns_idx = (uint32_t)(p / W);
  r.row = (uint32_t)(p % W);
  r.start = (int32_t)pr.start;
  r.end = (int32_t)pr.end;
  r.kind = SQUARES ? nsq::entry_pack(pr.kind, nsq::query_square(ns[(uint64_t)r.ns_idx * 8 + 7])) : pr.kind;
  r.nnodes = nn;
  r.node0 = base.nodes + (in - nn);
  r.leaf0 = base.leaves + (il - nl);
  req[base.entries + (ie - 1)] = r;
}

__global__ __launch_bounds__(256) void k_ns_compact(const Pair* __restrict__ pairs, uint64_t npairs, uint32_t W,
                                                    uint32_t L, const Sums* __restrict__ block_sums,
                                                    Request* __restrict__ req) {
  __shared__ uint32_t sh[kWavesPerGroup * 3];
  ns_compact_block<false>(pairs, npairs, W, L, block_sums, nullptr, req, sh);
}

__global__ __launch_bounds__(256) void k_ns_compact_squares(const Pair* __restrict__ pairs, uint64_t npairs,
                                                            uint32_t W, uint32_t L,
                                                            const Sums* __restrict__ block_sums,
                                                            const uint32_t* __restrict__ ns,
                                                            Request* __restrict__ req) {
  __shared__ uint32_t sh[kWavesPerGroup * 3];
  ns_compact_block<true>(pairs, npairs, W, L, block_sums, ns, req, sh);
}

// Entry q, of kind `kind`, of the square whose cells are at eds and whose index is at index.
__device__ __forceinline__ void ns_emit_entry(const uint8_t* __restrict__ eds, const uint16_t* __restrict__ index,
                                              uint32_t W, uint32_t L, const Request& q, uint32_t kind,
                                              uint8_t* __restrict__ leaves, uint8_t* __restrict__ nodes,
                                              uint32_t lane) {
  const uint32_t s = (uint32_t)q.start, e1 = (uint32_t)q.end - 1u;
  const uint32_t nn = q.nnodes;
  const uint32_t np = nn - (kind == nsq::kAbsence ? 1u : 0u);  // ProveRange's nodes
  uint32_t rec = 0;
  if (lane < np) {
    const prove::NodeAt a = prove::node_at(L, s, e1, lane);
    rec = (uint32_t)prove::index_record(W, 0, q.row, a.level, a.pos);
  } else if (lane < nn) {
    rec = (uint32_t)prove::index_record(W, 0, q.row, 0, s);  // the leaf hash
  }
  copy_proof_nodes(rec, nn, index, reinterpret_cast<uint16_t*>(nodes + q.node0 * kNode), lane);
  if (!leaves || kind != nsq::kInclusion) return;
  const uint4* cells = reinterpret_cast<const uint4*>(eds);
  uint4* lo = reinterpret_cast<uint4*>(leaves + q.leaf0 * kShare);
  const uint32_t vecs = (uint32_t)(q.end - q.start) * kShareVecs;
  const uint64_t cell0 = (uint64_t)q.row * W + s;
  for (uint32_t t = lane; t < vecs; t += 64) lo[t] = cells[cell0 * kShareVecs + t];
}

__global__ __launch_bounds__(256) void k_ns_emit(const uint8_t* __restrict__ eds, const uint16_t* __restrict__ index,
                                                 uint32_t W, uint32_t L, const nsq::Head* __restrict__ head,
                                                 uint32_t n_entries, uint8_t* __restrict__ leaves,
                                                 uint8_t* __restrict__ nodes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
  if (i >= n_entries || i >= head->totals.entries || head->W != W) return;
  const Request q = reinterpret_cast<const Request*>(reinterpret_cast<const uint8_t*>(head) + nsq::kReqOff)[i];
  ns_emit_entry(eds, index, W, L, q, q.kind, leaves, nodes, lane);
}

// k_ns_emit over a batch index, on a plan made over one (the head's width carries
// nsq::kSquaresPlan; on any other plan the kernel does nothing): the entry names its square above
// its kind, and the wave forms the two bases once. An entry whose square is not below n_squares,
// which no plan made for these n_squares holds, is skipped.
__global__ __launch_bounds__(256) void k_ns_emit_squares(const uint8_t* __restrict__ eds,
                                                         const uint8_t* __restrict__ index, uint32_t W, uint32_t L,
                                                         uint32_t n_squares, const nsq::Head* __restrict__ head,
                                                         uint32_t n_entries, uint8_t* __restrict__ leaves,
                                                         uint8_t* __restrict__ nodes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
  if (i >= n_entries || i >= head->totals.entries || head->W != (W | nsq::kSquaresPlan)) return;
  const Request q = reinterpret_cast<const Request*>(reinterpret_cast<const uint8_t*>(head) + nsq::kReqOff)[i];
  const uint32_t sq = nsq::entry_square(q.kind);
  if (sq >= n_squares) return;
  ns_emit_entry(eds + prove::eds_base(W, sq), reinterpret_cast<const uint16_t*>(index + prove::slice_base(W, sq)), W,
                L, q, nsq::entry_kind(q.kind), leaves, nodes, lane);
}

}  // namespace

hipError_t launch_ns_plan(const void* d_index, uint32_t k, uint32_t n, const nsq::Work& w, int stages, hipStream_t s) {
  if (!n) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_namespace_plan");
  if (stages & 1) {
    const uint64_t waves = (uint64_t)n * ((x.W + 63) / 64);
    hipLaunchKernelGGL(k_ns_find, dim3((uint32_t)((waves + kWavesPerGroup - 1) / kWavesPerGroup)),
                       dim3(64 * kWavesPerGroup), 0, s, static_cast<const uint32_t*>(d_index), x.W, x.L, w.ns, n,
                       w.pairs);
  }
  if (stages & 2) {
    hipLaunchKernelGGL(k_ns_sums, dim3((uint32_t)w.blocks), dim3(256), 0, s, w.pairs, w.npairs, x.L, w.block_sums);
    hipLaunchKernelGGL(k_ns_scan, dim3(1), dim3(256), 0, s, w.block_sums, w.blocks, x.W, w.head);
    hipLaunchKernelGGL(k_ns_compact, dim3((uint32_t)w.blocks), dim3(256), 0, s, w.pairs, w.npairs, x.W, x.L,
                       w.block_sums, w.req);
  }
  return hipGetLastError();
}

hipError_t launch_ns_plan_squares(const void* d_index, uint32_t k, uint32_t n, const nsq::Work& w, hipStream_t s) {
  if (!n) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_namespace_plan_squares");
  const uint64_t waves = (uint64_t)n * ((x.W + 63) / 64);
  hipLaunchKernelGGL(k_ns_find_squares, dim3((uint32_t)((waves + kWavesPerGroup - 1) / kWavesPerGroup)),
                     dim3(64 * kWavesPerGroup), 0, s, static_cast<const uint8_t*>(d_index), x.W, x.L, w.ns, n, w.pairs);
  hipLaunchKernelGGL(k_ns_sums, dim3((uint32_t)w.blocks), dim3(256), 0, s, w.pairs, w.npairs, x.L, w.block_sums);
  // the head's width marks the plan as one over a batch index
  hipLaunchKernelGGL(k_ns_scan, dim3(1), dim3(256), 0, s, w.block_sums, w.blocks, x.W | nsq::kSquaresPlan, w.head);
  hipLaunchKernelGGL(k_ns_compact_squares, dim3((uint32_t)w.blocks), dim3(256), 0, s, w.pairs, w.npairs, x.W, x.L,
                     w.block_sums, w.ns, w.req);
  return hipGetLastError();
}

hipError_t launch_ns_emit_squares(const uint8_t* eds, const void* d_index, uint32_t k, uint32_t n_squares,
                                  const void* d_work, uint32_t n_entries, uint8_t* d_leaves, uint8_t* d_nodes,
                                  hipStream_t s) {
  if (!n_entries) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_namespace_emit_squares");
  hipLaunchKernelGGL(k_ns_emit_squares, dim3((n_entries + kWavesPerGroup - 1) / kWavesPerGroup),
                     dim3(64 * kWavesPerGroup), 0, s, eds, static_cast<const uint8_t*>(d_index), x.W, x.L, n_squares,
                     static_cast<const nsq::Head*>(d_work), n_entries, d_leaves, d_nodes);
  return hipGetLastError();
}

hipError_t launch_ns_emit(const uint8_t* eds, const void* d_index, uint32_t k, const void* d_work, uint32_t n_entries,
                          uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s) {
  if (!n_entries) return hipSuccess;
  const prove::IndexLayout x = prove::index_layout(k);
  const Range r("nmt_namespace_emit");
  hipLaunchKernelGGL(k_ns_emit, dim3((n_entries + kWavesPerGroup - 1) / kWavesPerGroup), dim3(64 * kWavesPerGroup), 0,
                     s, eds, static_cast<const uint16_t*>(d_index), x.W, x.L, static_cast<const nsq::Head*>(d_work), n_entries,
                     d_leaves, d_nodes);
  return hipGetLastError();
}

}  // namespace cel
