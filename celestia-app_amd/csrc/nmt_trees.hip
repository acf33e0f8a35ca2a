// NMT and RFC-6962 trees outside the EDS commit on gfx950: one erasured axis or one plain NMT
// over arbitrary leaves (roots), the repair's roots of many gathered axes, the exported trees
// of the proofs (every level kept), and merkle.HashFromByteSlices over byte slices.
// Levels go through the strided level kernel and reducer of nmt_slab.hip (nmt_host.hpp);
// k_reduce_pass is the one level kernel that carries an odd last node up.
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "nmt_device.hpp"
#include "nmt_host.hpp"
#include "sha256_device.hpp"

namespace cel {

// ------------------------------------------------------------ single-tree roots

// SHA256(pre || a[0..la)), processed byte-wise (generic path, small inputs only).
__device__ void sha_bytes(const uint8_t* __restrict__ a, uint32_t la, uint8_t pre, uint32_t (&st)[8]) {
  const uint64_t total = 1ull + la;
  sha256_init(st);
  uint32_t w[16];
  const uint64_t padded = ((total + 8) / 64 + 1) * 64;
  for (uint64_t blk = 0; blk < padded; blk += 64) {
    for (int wi = 0; wi < 16; wi++) {
      uint32_t x = 0;
      for (int j = 0; j < 4; j++) {
        const uint64_t p = blk + 4 * wi + j;
        uint32_t v;
        if (p == 0) v = pre;
        else if (p < total) v = a[p - 1];
        else if (p == total) v = 0x80;
        else if (p >= padded - 8) v = (uint32_t)(((total * 8) >> (8 * (padded - 1 - p))) & 0xFF);
        else v = 0;
        x = (x << 8) | v;
      }
      w[wi] = x;
    }
    sha256_compress(st, w);
  }
}

// Plain NMT over arbitrary leaves (k_leaf assumes 512-byte EDS cells, so leaves are
// hashed by a generic lane-per-leaf kernel over a byte message).
__global__ __launch_bounds__(256) void k_generic_leaf(const uint8_t* __restrict__ leaves, uint32_t n, uint32_t len,
                                                      uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* lf = leaves + (uint64_t)i * len;
  uint32_t st[8];
  sha_bytes(lf, len, 0x00, st);
  uint32_t nd[kNodeWords];
  uint8_t* nb = reinterpret_cast<uint8_t*>(nd);
  for (int j = 0; j < 29; j++) { nb[j] = lf[j]; nb[29 + j] = lf[j]; }
  nb[58] = nb[59] = 0;
  nd[14] &= 0xFFFFu;
  put_digest(nd, st);
  store_node(out + (uint64_t)i * kNodeWords, nd);
}

// Erasured axis: cells (2k x 512 B) with the wrapper's namespace rule.
__global__ __launch_bounds__(256) void k_axis_leaf(const uint8_t* __restrict__ cells, uint32_t k, uint32_t axis,
                                                   uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= 2 * k) return;
  uint32_t nd[kNodeWords];
  make_leaf_node<true>(reinterpret_cast<const uint32_t*>(cells + (uint64_t)i * kShare), (i < k) && (axis < k), nd);
  store_node(out + (uint64_t)i * kNodeWords, nd);
}

// One level of one tree of n nodes, any n: an odd last node moves up unchanged.
__global__ __launch_bounds__(256) void k_reduce_pass(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                     uint32_t n) {
  const uint32_t half = n / 2;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < half) {
    uint32_t o[kNodeWords];
    hash_pair(in, 2 * j, 2 * j + 1, o);
    store_node(out + (uint64_t)j * kNodeWords, o);
  } else if ((n & 1) && j == half) {
    uint32_t x[kNodeWords];
    load_node(in + (uint64_t)(n - 1) * kNodeWords, x);
    store_node(out + (uint64_t)half * kNodeWords, x);
  }
}

__global__ void k_pack_root(const uint32_t* __restrict__ node, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = threadIdx.x;
  if (i >= kNode) return;
  if (n == 0) {  // empty tree: 0*58 || SHA256("")
    if (i < 58) out[i] = 0;
    if (i == 0) {
      uint32_t st[8];
      sha_empty(st);
      for (int j = 0; j < 32; j++) out[58 + j] = (uint8_t)(st[j / 4] >> (24 - 8 * (j % 4)));
    }
    return;
  }
  out[i] = reinterpret_cast<const uint8_t*>(node)[i];
}

// Two buffers of `bytes` each, a level reading one and writing the other: the workspace of
// the single-tree paths and of the byte-slice hash.
struct PairWork {
  uint32_t *a, *b;
  size_t size;
};
static PairWork pair_work(void* work, size_t bytes) {
  Carver c(work);
  PairWork w;
  w.a = c.take<uint32_t>(bytes);
  w.b = c.take<uint32_t>(bytes);
  w.size = c.size();
  return w;
}
static PairWork axis_root_work(void* work, uint32_t k) { return pair_work(work, (size_t)2 * k * kNodeWords * 4); }
static PairWork nmt_root_work(void* work, uint32_t n) { return pair_work(work, (size_t)(n ? n : 1) * kNodeWords * 4); }
static PairWork slices_work(void* work, uint32_t n) { return pair_work(work, (size_t)(n ? n : 1) * 32); }

size_t axis_root_workspace_size(uint32_t k) { return axis_root_work(nullptr, k).size; }
size_t nmt_root_workspace_size(uint32_t n) { return nmt_root_work(nullptr, n).size; }
size_t slices_workspace_size(uint32_t n) { return slices_work(nullptr, n).size; }

// Reduce the n nodes in w.a (one tree) to a root with repeated passes, then pack it.
static hipError_t reduce_tree(const PairWork& w, uint32_t n, uint8_t* root, hipStream_t s) {
  uint32_t* src = w.a;
  uint32_t* dst = w.b;
  while (n > 1) {
    const uint32_t nout = n / 2 + (n & 1);
    hipLaunchKernelGGL(k_reduce_pass, dim3((nout + 255) / 256), dim3(256), 0, s, src, dst, n);
    uint32_t* t = src;
    src = dst;
    dst = t;
    n = nout;
  }
  hipLaunchKernelGGL(k_pack_root, dim3(1), dim3(128), 0, s, src, n, root);
  return hipGetLastError();
}

hipError_t launch_axis_root(const uint8_t* cells, uint32_t k, uint32_t axis, uint8_t* root, void* work,
                            hipStream_t s) {
  const PairWork w = axis_root_work(work, k);
  hipLaunchKernelGGL(k_axis_leaf, dim3((2 * k + 255) / 256), dim3(256), 0, s, cells, k, axis, w.a);
  return reduce_tree(w, 2 * k, root, s);
}

hipError_t launch_nmt_root(const uint8_t* leaves, uint32_t n, uint32_t len, uint8_t* root, void* work,
                           hipStream_t s) {
  const PairWork w = nmt_root_work(work, n);
  if (n) hipLaunchKernelGGL(k_generic_leaf, dim3((n + 255) / 256), dim3(256), 0, s, leaves, n, len, w.a);
  return reduce_tree(w, n, root, s);
}

// ----------------------------------------------------- roots of gathered axes (repair)

// Leaves of `naxes` erasured axes held densely as cells[a][2k][512]; axis_idx[a] is the
// row/column index that decides the Q0 namespace rule.
__global__ __launch_bounds__(256) void k_axes_leaf(const uint8_t* __restrict__ cells, uint32_t k,
                                                   const int32_t* __restrict__ axis_idx, uint32_t naxes,
                                                   uint32_t* __restrict__ out) {
  const uint32_t W = 2 * k;
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= naxes * W) return;
  const bool q0 = (g % W < k) && ((uint32_t)axis_idx[g / W] < k);
  uint32_t nd[kNodeWords];
  make_leaf_node<true>(reinterpret_cast<const uint32_t*>(cells + (uint64_t)g * kShare), q0, nd);
  store_node(out + (uint64_t)g * kNodeWords, nd);
}

// Workspace: leaves [naxes][2k] | ping [naxes][k] | pong [naxes][k/2]
struct AxesWork {
  uint32_t *leaves, *ping, *pong;
  size_t size;
};
static AxesWork axes_work(void* work, uint32_t k, uint32_t naxes) {
  const size_t W = 2 * (size_t)k, nb = kNodeWords * 4;
  Carver c(work);
  AxesWork w;
  w.leaves = c.take<uint32_t>(naxes * W * nb);
  w.ping = c.take<uint32_t>(naxes * (W / 2 + 1) * nb);
  w.pong = c.take<uint32_t>(naxes * (W / 4 + 1) * nb);
  w.size = c.size();
  return w;
}

size_t axes_roots_workspace_size(uint32_t k, uint32_t naxes) { return axes_work(nullptr, k, naxes).size; }

// roots: [naxes] 96-byte records.
hipError_t launch_axes_roots(const uint8_t* cells, uint32_t k, const int32_t* axis_idx, uint32_t naxes,
                             uint32_t* roots, void* work, hipStream_t s) {
  const uint32_t W = 2 * k;
  const AxesWork w = axes_work(work, k, naxes);
  hipLaunchKernelGGL(k_axes_leaf, dim3((naxes * W + 255) / 256), dim3(256), 0, s, cells, k, axis_idx, naxes, w.leaves);
  reduce_trees(LevelJob{w.leaves, nullptr, W, naxes, W, 1}, w.ping, w.pong, roots, s);
  return hipGetLastError();
}

// ------------------------------------------------------------ RFC-6962 over items

// One region, the padded items: launch_merkle_root and launch_rfc_tree use `work` as it is.
size_t merkle_workspace_size(uint32_t n) { return align256((size_t)(n ? n : 1) * kNodeWords * 4); }

__global__ void k_pad_items(const uint8_t* __restrict__ items, uint32_t n, uint32_t len, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t* o = reinterpret_cast<uint8_t*>(out + (uint64_t)i * kNodeWords);
  for (uint32_t j = 0; j < kNodeWords * 4; j++) o[j] = j < len ? items[(uint64_t)i * len + j] : 0;
}

hipError_t launch_merkle_root(const uint8_t* items, uint32_t n, uint32_t item_len, uint8_t* out, void* work,
                              hipStream_t s) {
  if (item_len != kNode) return hipErrorInvalidValue;  // DAH items are NMT roots
  uint32_t* pad = static_cast<uint32_t*>(work);
  if (n) hipLaunchKernelGGL(k_pad_items, dim3((n + 255) / 256), dim3(256), 0, s, items, n, item_len, pad);
  if ((size_t)n * 8 * 4 > 64 * 1024) return hipErrorInvalidValue;  // the digests must fit LDS
  launch_merkle(pad, nullptr, n, 1, out, nullptr, nullptr, s);
  return hipGetLastError();
}

// ---------------------------------------------------- exported trees (proofs, §8f)
//
// Every node of the NMT trees of `naxes` gathered axes (cells[a][2k][512], axis_idx[a]
// = the row/column index that decides the Q0 namespace rule), level-major:
//   nodes = level 0 [naxes][2k] | level 1 [naxes][k] | ... | level log2(2k) [naxes][1]
// 96-byte records. This is what nmt ProveRange / the subtree-root cacher read instead
// of rebuilding the trees on the CPU (pkg/proof/proof.go:151-201,
// pkg/inclusion/nmt_caching.go:96-124).
size_t axes_trees_nodes(uint32_t k, uint32_t naxes) { return (size_t)naxes * (4 * (size_t)k - 1); }

hipError_t launch_axes_trees(const uint8_t* cells, uint32_t k, const int32_t* axis_idx, uint32_t naxes,
                             uint32_t* nodes, hipStream_t s) {
  const uint32_t W = 2 * k;
  hipLaunchKernelGGL(k_axes_leaf, dim3((naxes * W + 255) / 256), dim3(256), 0, s, cells, k, axis_idx, naxes, nodes);
  // every level is kept: level by level through the output itself, no ping / pong
  uint32_t* src = nodes;
  for (uint32_t nin = W; nin > 1; nin /= 2) {
    uint32_t* out = src + (size_t)naxes * nin * kNodeWords;
    launch_level_pair(LevelJob{src, out, nin, naxes, nin, 1}, LevelJob{}, s);
    src = out;
  }
  return hipGetLastError();
}

// RFC-6962 tree of n = 2^m items of 90 bytes (DataAvailabilityHeader.Hash over
// rowRoots || colRoots), every level: level 0 = the n leaf hashes SHA256(0x00 || item),
// then n/2 inner hashes SHA256(0x01 || l || r), ..., the root. 8 big-endian words per
// node. (merkle.ProofsFromByteSlices reads its aunts from these levels.)
__global__ void k_rfc_leaves(const uint32_t* __restrict__ items, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t R[kNodeWords], st[8];
  load_node(items + (uint64_t)i * kNodeWords, R);
  rfc_leaf90(R, st);
  for (int j = 0; j < 8; j++) out[(uint64_t)i * 8 + j] = st[j];
}

__global__ void k_rfc_level(const uint32_t* __restrict__ in, uint32_t nout, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nout) return;
  uint32_t st[8];
  rfc_inner(in + (uint64_t)(2 * i) * 8, in + (uint64_t)(2 * i + 1) * 8, st);
  for (int j = 0; j < 8; j++) out[(uint64_t)i * 8 + j] = st[j];
}

hipError_t launch_rfc_tree(const uint8_t* items90, uint32_t n, uint32_t* levels, void* work, hipStream_t s) {
  if (!n || (n & (n - 1))) return hipErrorInvalidValue;
  uint32_t* pad = static_cast<uint32_t*>(work);
  hipLaunchKernelGGL(k_pad_items, dim3((n + 255) / 256), dim3(256), 0, s, items90, n, kNode, pad);
  hipLaunchKernelGGL(k_rfc_leaves, dim3((n + 255) / 256), dim3(256), 0, s, pad, n, levels);
  uint32_t* src = levels;
  for (uint32_t m = n; m > 1; m /= 2) {
    uint32_t* out = src + (size_t)m * 8;
    hipLaunchKernelGGL(k_rfc_level, dim3((m / 2 + 255) / 256), dim3(256), 0, s, src, m / 2, out);
    src = out;
  }
  return hipGetLastError();
}

// Pack selected 96-byte node records into 90-byte items: out[i] = nodes[rec[i]].
__global__ void k_gather_nodes(const uint32_t* __restrict__ nodes, const int32_t* __restrict__ rec, uint32_t n,
                               uint8_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kNode) return;
  const uint32_t i = t / kNode, b = t % kNode;
  out[t] = reinterpret_cast<const uint8_t*>(nodes + (uint64_t)rec[i] * kNodeWords)[b];
}

hipError_t launch_gather_nodes(const uint32_t* nodes, const int32_t* rec, uint32_t n, uint8_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_gather_nodes, dim3((n * kNode + 255) / 256), dim3(256), 0, s, nodes, rec, n, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ byte slices

// merkle.HashFromByteSlices (tendermint crypto/merkle, RFC-6962) over n byte slices of any
// length: the DAH hash when the roots are not all 90-byte NMT roots
// (data_availability_header.go:92-108 hashes whatever RowRoots / ColumnRoots hold). Leaf
// i = SHA256(0x00 || slice i), one lane each; then one workgroup pairs adjacent nodes
// level by level, carrying an odd last node up unchanged, which is the same tree as the
// reference's split at the largest power of two below n. n == 0: SHA256("").
__global__ void k_slice_leaves(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off, uint32_t n,
                               uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t st[8];
  sha_bytes(data + off[i], (uint32_t)(off[i + 1] - off[i]), 0x00, st);
  for (int j = 0; j < 8; j++) out[(uint64_t)i * 8 + j] = st[j];
}

__global__ __launch_bounds__(256) void k_slice_tree(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint32_t n,
                                                    uint8_t* __restrict__ out) {
  if (n == 0) {
    if (threadIdx.x == 0) {
      uint32_t st[8];
      sha_empty(st);
      for (int j = 0; j < 32; j++) out[j] = (uint8_t)(st[j / 4] >> (24 - 8 * (j % 4)));
    }
    return;
  }
  uint32_t* src = a;
  uint32_t* dst = b;
  for (uint32_t m = n; m > 1; m = (m + 1) / 2) {  // ping-pong: a level reads src, writes dst
    for (uint32_t i = threadIdx.x; i < m / 2; i += blockDim.x) {
      uint32_t st[8];
      rfc_inner(src + (uint64_t)(2 * i) * 8, src + (uint64_t)(2 * i + 1) * 8, st);
      for (int j = 0; j < 8; j++) dst[(uint64_t)i * 8 + j] = st[j];
    }
    if ((m & 1) && threadIdx.x == 0)
      for (int j = 0; j < 8; j++) dst[(uint64_t)(m / 2) * 8 + j] = src[(uint64_t)(m - 1) * 8 + j];
    __syncthreads();
    uint32_t* t = src;
    src = dst;
    dst = t;
  }
  if (threadIdx.x < 32) out[threadIdx.x] = (uint8_t)(src[threadIdx.x / 4] >> (24 - 8 * (threadIdx.x % 4)));
}

hipError_t launch_hash_slices(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out, void* work,
                              hipStream_t s) {
  const PairWork w = slices_work(work, n);
  if (n) hipLaunchKernelGGL(k_slice_leaves, dim3((n + 255) / 256), dim3(256), 0, s, data, off, n, w.a);
  hipLaunchKernelGGL(k_slice_tree, dim3(1), dim3(256), 0, s, w.a, w.b, n, out);
  return hipGetLastError();
}

}  // namespace cel
