// The row-sharded mode of the NMT commit on gfx950, and the strided level
// kernel and reducer every path but the EDS commit's own levels builds its trees with.
//
// A rank holds a column slab of one EDS: slab[i][j] = cell (i, c0 + j), i < 2k, j < w,
// w = 2k / nranks. It hashes the slab's leaves once, builds its w column trees in full
// and, for every row, the subtree root over its w-wide slice (an aligned power-of-two
// range, hence a subtree of the row's perfect tree). Rank-ordered subtree roots are
// combined into the row roots after an all-gather.
#include <hip/hip_runtime.h>

#include <climits>

#include "cel_internal.hpp"
#include "nmt_device.hpp"
#include "nmt_host.hpp"
#include "sha256_device.hpp"

namespace cel {

template <bool ORDER, bool PF>
__global__ __launch_bounds__(256) void k_slab_leaf(const uint8_t* __restrict__ slab, uint32_t k, uint32_t c0, uint32_t w,
                                            uint32_t cell0, uint32_t cell1, uint32_t* __restrict__ leaves,
                                            int32_t* __restrict__ bad_axis) {
  const uint32_t W = 2 * k;
  const uint32_t cell = cell0 + blockIdx.x * 256u + threadIdx.x;
  if (cell >= cell1) return;
  const uint32_t i = cell / w, j = cell % w, c = c0 + j;
  const uint32_t* sh = reinterpret_cast<const uint32_t*>(slab + (uint64_t)cell * kShare);
  const bool q0 = (i < k) && (c < k);
  if (ORDER && q0) {
    if (j > 0 && ns_less(sh, sh - kShare / 4)) atomicMin(bad_axis, (int32_t)i);
    if (i > 0 && ns_less(sh, sh - (uint64_t)w * kShare / 4)) atomicMin(bad_axis, (int32_t)(W + c));
  }
  uint32_t nd[kNodeWords];
  make_leaf_node<PF>(sh, q0, nd);
  store_node(leaves + (uint64_t)cell * kNodeWords, nd);
}

// One level of two independent tree sets in one launch (the slab's column trees and row
// subtrees; one set with the other job empty): LevelJob, nmt_host.hpp.
__global__ __launch_bounds__(256) void k_level_pair(LevelJob a, LevelJob b) {
  uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const uint32_t na = a.nin > 1 ? a.trees * (a.nin / 2) : 0u;
  const uint32_t nb = b.nin > 1 ? b.trees * (b.nin / 2) : 0u;
  if (idx >= na + nb) return;
  const LevelJob& j = idx < na ? a : b;
  if (idx >= na) idx -= na;
  const uint32_t nout = j.nin / 2;
  const uint32_t t = idx / nout, l = idx % nout;
  const uint64_t li = (uint64_t)t * j.tstride + (uint64_t)(2 * l) * j.lstride, ri = li + j.lstride;
  uint32_t o[kNodeWords];
  hash_pair(j.in, li, ri, o);
  store_node(j.out + (uint64_t)idx * kNodeWords, o);
}

// Namespace compare of two node records: is R's minNs (bytes 0..28) below L's maxNs
// (bytes 29..57)? Big-endian words: 7 full words, then the 29th byte.
__device__ __forceinline__ bool min_below_max(const uint32_t* __restrict__ R, const uint32_t* __restrict__ L) {
  uint32_t r[8], l[16];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const uint4 v = reinterpret_cast<const uint4*>(R)[q];
    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 v = reinterpret_cast<const uint4*>(L)[q];
    l[4 * q] = v.x; l[4 * q + 1] = v.y; l[4 * q + 2] = v.z; l[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 7; q++) {
    const uint32_t a = bswap32(r[q]), b = bswap32(__builtin_amdgcn_alignbyte(l[8 + q], l[7 + q], 1));
    if (a != b) return a < b;
  }
  return (r[7] & 0xFFu) < ((l[14] >> 8) & 0xFFu);
}

// The finish's status in one workgroup: the max over ranks of the gathered step-2 status
// (first int32 of record r * stride + at), or CEL_EORDER when the push order breaks
// across a slab boundary in a row of Q0: rank r's first leaf namespace (its subtree's
// minNs) below rank r-1's last leaf namespace. That is r-1's subtree maxNs unless its last
// leaf carries the parity namespace, which IgnoreMaxNamespace keeps out of maxNs: rank
// r-1 then set dword 23 of its record (k_slab_status), and any minNs but 0xFF*29 is below
// it. subs: rank r's 2k row-subtree records at subs[r * stride].
__global__ __launch_bounds__(256) void k_shard_status(const uint32_t* __restrict__ subs, uint32_t stride, uint32_t at,
                                                      uint32_t k, uint32_t w, uint32_t nranks, int order_check,
                                                      int32_t* __restrict__ status) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  if (order_check) {
    int mine = 0;
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x)
      for (uint32_t r = 1; r < nranks && r * w < k; r++) {
        const uint32_t* R = subs + ((uint64_t)r * stride + i) * kNodeWords;
        const uint32_t* L = subs + ((uint64_t)(r - 1) * stride + i) * kNodeWords;
        mine |= L[kNodeWords - 1] ? !min_is_parity(R) : min_below_max(R, L);
      }
    if (mine) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t m = 0;
    for (uint32_t r = 0; r < nranks; r++) {
      const int32_t v = (int32_t)subs[((uint64_t)r * stride + at) * kNodeWords];
      m = v > m ? v : m;
    }
    *status = bad ? CEL_EORDER : m;
  }
}

// The slab commit's status, and for every Q0 row i whether the slab's last leaf carries the
// parity namespace: dword 23 of row i's subtree record (record bytes 92..95, past the 90
// node bytes; no hash or pack reads them) is 1 then and 0 otherwise. k_shard_status needs
// it: the subtree's maxNs leaves that leaf out.
__global__ __launch_bounds__(256) void k_slab_status(const int32_t* __restrict__ bad_axis, int32_t* __restrict__ status,
                                                     const uint32_t* __restrict__ leaves, uint32_t* __restrict__ row_sub,
                                                     uint32_t k, uint32_t w) {
  if (threadIdx.x == 0) *status = *bad_axis != INT_MAX ? CEL_EORDER : CEL_OK;
  for (uint32_t i = threadIdx.x; i < k; i += blockDim.x)
    row_sub[(uint64_t)i * kNodeWords + kNodeWords - 1] =
        min_is_parity(leaves + ((uint64_t)i * w + w - 1) * kNodeWords) ? 1u : 0u;
}

void launch_level_pair(const LevelJob& a, const LevelJob& b, hipStream_t s) {
  const uint32_t n = (a.nin > 1 ? a.trees * (a.nin / 2) : 0u) + (b.nin > 1 ? b.trees * (b.nin / 2) : 0u);
  hipLaunchKernelGGL(k_level_pair, dim3((n + 255) / 256), dim3(256), 0, s, a, b);
}

// The reducer (nmt_host.hpp): one k_level_pair launch per level until both sets are down to
// one node per tree.
void reduce_trees_pair(LevelJob a, uint32_t* ping_a, uint32_t* pong_a, uint32_t* roots_a, LevelJob b,
                       uint32_t* ping_b, uint32_t* pong_b, uint32_t* roots_b, hipStream_t s) {
  uint32_t *dst_a = ping_a, *dst_b = ping_b;
  // a set's next level reads what this one wrote, compact, and writes its other buffer
  auto advance = [](LevelJob& j, uint32_t*& dst, uint32_t* ping, uint32_t* pong) {
    if (j.nin < 2) return;
    j = LevelJob{j.out, nullptr, j.nin / 2, j.trees, j.nin / 2, 1};
    dst = dst == ping ? pong : ping;
  };
  while (a.nin > 1 || b.nin > 1) {
    a.out = a.nin == 2 ? roots_a : dst_a;
    b.out = b.nin == 2 ? roots_b : dst_b;
    launch_level_pair(a, b, s);
    advance(a, dst_a, ping_a, pong_a);
    advance(b, dst_b, ping_b, pong_b);
  }
}

// The slab commit's workspace: leaves [2k*w] | ping, pong of the column trees [k*w] |
// the order flag | ping, pong of the row subtrees [k*w]
struct SlabWork {
  uint32_t *leaves, *ping, *pong, *ping2, *pong2;
  int32_t* bad;
  size_t size;
};
static SlabWork slab_work(void* work, uint32_t k, uint32_t w) {
  const size_t nb = kNodeWords * 4, W = 2 * (size_t)k, half = (size_t)k * w * nb + nb;
  Carver c(work);
  SlabWork sw;
  sw.leaves = c.take<uint32_t>(W * w * nb);
  sw.ping = c.take<uint32_t>(half);
  sw.pong = c.take<uint32_t>(half);
  sw.bad = c.take<int32_t>(4);
  sw.ping2 = c.take<uint32_t>(half);
  sw.pong2 = c.take<uint32_t>(half);
  sw.size = c.size();
  return sw;
}

size_t slab_workspace_size(uint32_t k, uint32_t w) { return slab_work(nullptr, k, w).size; }

// Leaves of slab rows [row0, row1) (2k rows of w cells). The half holding rows < k checks
// the push order and must come first in stream order after the flag is reset (init_bad).
hipError_t launch_slab_leaves(const uint8_t* slab, uint32_t k, uint32_t c0, uint32_t w, uint32_t row0, uint32_t row1,
                              void* work, bool order_check, bool init_bad, hipStream_t s) {
  const SlabWork sw = slab_work(work, k, w);
  if (init_bad) launch_fill_i32(sw.bad, 1u, INT_MAX, 64, s);
  const uint32_t cell0 = row0 * w, cell1 = row1 * w;
  if (cell1 <= cell0) return hipGetLastError();
  dim3 gl((cell1 - cell0 + 255) / 256);
  dispatch_order_pf(order_check, latency_bound(2ull * k * w), [&](auto order, auto pf) {
    hipLaunchKernelGGL((k_slab_leaf<decltype(order)::value, decltype(pf)::value>), gl, dim3(256), 0, s, slab, k, c0, w,
                       cell0, cell1, sw.leaves, sw.bad);
  });
  return hipGetLastError();
}

// After every leaf of the slab: w column trees of 2k leaves (leaf i of column j at
// i*w + j) and 2k row subtrees of w leaves (leaf j of row i at i*w + j), both sets one
// level per launch, then the status and the rows' last-leaf marks.
hipError_t launch_slab_trees(uint32_t k, uint32_t w, uint32_t* col_rec, uint32_t* row_sub, int32_t* status,
                             void* work, hipStream_t s) {
  const uint32_t W = 2 * k;
  const size_t nb = kNodeWords * 4;
  const SlabWork sw = slab_work(work, k, w);
  // One-cell-wide slabs: the row subtrees are the leaves. No caller gets here today (the C ABI
  // admits nranks <= k, so w >= 2), and no test can reach it.
  if (w == 1) {
    const hipError_t e = hipMemcpyAsync(row_sub, sw.leaves, (size_t)W * nb, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  const LevelJob cols{sw.leaves, nullptr, W, w, 1, w};
  const LevelJob rows{sw.leaves, nullptr, w, W, w, 1};
  reduce_trees_pair(cols, sw.ping, sw.pong, col_rec, rows, sw.ping2, sw.pong2, row_sub, s);
  hipLaunchKernelGGL(k_slab_status, dim3(1), dim3(256), 0, s, sw.bad, status, sw.leaves, row_sub, k, w);
  return hipGetLastError();
}

// The finish's workspace: ping, pong [2k * nranks / 2] | items [rows 2k | cols 2k] |
// DAH leaf digests [4k][8]
struct FinishWork {
  uint32_t *ping, *pong, *items, *leafd;
  size_t size;
};
static FinishWork finish_work(void* work, uint32_t k, uint32_t nranks) {
  const size_t nb = kNodeWords * 4, W = 2 * (size_t)k;
  Carver c(work);
  FinishWork fw;
  fw.ping = c.take<uint32_t>(W * (nranks / 2 + 1) * nb);
  fw.pong = c.take<uint32_t>(W * (nranks / 2 + 1) * nb);
  fw.items = c.take<uint32_t>(2 * W * nb);
  fw.leafd = c.take<uint32_t>(2 * W * 32);
  fw.size = c.size();
  return fw;
}

size_t shard_finish_workspace_size(uint32_t k, uint32_t nranks) { return finish_work(nullptr, k, nranks).size; }

hipError_t launch_shard_finish(const uint32_t* gathered, uint32_t k, uint32_t nranks, uint8_t* row_roots,
                               uint8_t* col_roots, uint8_t* dah, int32_t* status, void* work, bool order_check,
                               hipStream_t s) {
  const uint32_t W = 2 * k, w = W / nranks;
  const uint32_t S = W + w + 1;  // records per rank: row subtrees, column roots, status
  const uint32_t* row_subs = gathered;
  const size_t nb = kNodeWords * 4;
  const FinishWork fw = finish_work(work, k, nranks);
  // the ranks' step-2 status (max), or EORDER across slab boundaries: one workgroup
  hipLaunchKernelGGL(k_shard_status, dim3(1), dim3(256), 0, s, gathered, S, W + w, k, w, nranks,
                     (order_check && nranks > 1) ? 1 : 0, status);
  // row i's subtree from rank r is gathered[r][i]: trees of nranks leaves, stride S
  hipError_t e = hipSuccess;
  if (nranks == 1) e = hipMemcpyAsync(fw.items, row_subs, (size_t)W * nb, hipMemcpyDeviceToDevice, s);
  else reduce_trees(LevelJob{row_subs, nullptr, nranks, W, 1, S}, fw.ping, fw.pong, fw.items, s);
  // the column roots: rank r's w records at gathered[r][W], in rank order
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(fw.items + (size_t)W * kNodeWords, (size_t)w * nb, gathered + (size_t)W * kNodeWords,
                         (size_t)S * nb, (size_t)w * nb, nranks, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  // the 4k RFC-6962 leaf digests and the packed roots one lane each, then the DAH tree
  // one level per round in one workgroup
  launch_dah_leaves(fw.items, 2 * W, fw.leafd, row_roots, col_roots, s);
  launch_merkle(fw.items, fw.leafd, 2 * W, 1, dah, nullptr, nullptr, s);
  return hipGetLastError();
}

}  // namespace cel
