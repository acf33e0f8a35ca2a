// nmt Proof.VerifyNamespace for a batch of proofs: the inclusion verifier (nmt_verify.hip) with
// the completeness rule, absence proofs and the empty proof. celestia_eds/proof.py
// (NMTProof.VerifyNamespace) states the rules; this file follows it rule by rule.
//
//   k_verify_ns_leaves  k_verify_leaves, and one byte per leaf: do the share's first 29 bytes
//                       equal the proof's namespace? (celestia-node hands nmt share[:29] ||
//                       share, and nmt checks that prefix against the queried namespace)
//   k_verify_ns_fold    one lane per proof. The fold is k_verify_fold's, pair for pair. Before
//                       it the lane checks the proof's shape by kind, ANDs its leaves' bytes,
//                       and checks completeness: of the proof's nodes the first popcount(start)
//                       are the left siblings (each must end below the namespace), all others
//                       right siblings (each must begin above it); the fold uses every one of
//                       them on that side. An absence proof's last node is its leaf hash: it is
//                       copied into the proof's own record behind the leaf records and folded
//                       as the single leaf.
//
// Every input is untrusted, as in nmt_verify.hip: a lane touches its own proof's leaf records
// [leaf0, leaf0 + nleaves), its own record total_leaves + i, its node records [node0, node0 +
// nnodes) and its root record only, ranges the host derives from checked offsets; a malformed
// proof leaves before it touches any of them but the root.
#include <hip/hip_runtime.h>

#define CEL_VERIFY_DEVICE
#include "cel_internal.hpp"
#include "nmt_verify.hpp"

namespace cel {
namespace {

__global__ __launch_bounds__(256) void k_verify_ns_leaves(const uint32_t* __restrict__ leaves,
                                                          const uint32_t* __restrict__ leaf_proof,
                                                          const uint32_t* __restrict__ ns, uint32_t total,
                                                          uint32_t* __restrict__ rec, uint8_t* __restrict__ leaf_ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t* np = ns + (uint64_t)leaf_proof[i] * 8;
  uint32_t n[8];
  const uint4 a = reinterpret_cast<const uint4*>(np)[0], b = reinterpret_cast<const uint4*>(np)[1];
  n[0] = a.x; n[1] = a.y; n[2] = a.z; n[3] = a.w; n[4] = b.x; n[5] = b.y; n[6] = b.z; n[7] = b.w & 0xFFu;
  bool par = n[7] == 0xFFu;
#pragma unroll
  for (int q = 0; q < 7; q++) par = par && (n[q] == 0xFFFFFFFFu);
  const uint32_t* sh = leaves + (uint64_t)i * (kShare / 4);
  {  // the share's own namespace against the proof's
    const uint4 s0 = reinterpret_cast<const uint4*>(sh)[0], s1 = reinterpret_cast<const uint4*>(sh)[1];
    const bool same = s0.x == n[0] && s0.y == n[1] && s0.z == n[2] && s0.w == n[3] && s1.x == n[4] && s1.y == n[5] &&
                      s1.z == n[6] && (s1.w & 0xFFu) == n[7];
    leaf_ok[i] = same ? 1 : 0;
  }
  uint32_t st[8];
  leaf_hash_ns(st, sh, n, par);
  uint32_t nd[kNodeWords];
#pragma unroll
  for (int q = 0; q < 7; q++) nd[q] = n[q];
  nd[7] = n[7] | (n[0] << 8);
#pragma unroll
  for (int q = 0; q < 6; q++) nd[8 + q] = __builtin_amdgcn_alignbyte(n[q + 1], n[q], 3);
  nd[14] = (n[6] >> 24) | (n[7] << 8);
  put_digest(nd, st);
  store_node(rec + (uint64_t)i * kNodeWords, nd);
}

// The big-endian compare words of a namespace given as 8 little-endian dwords (bytes 29..31 zero).
__device__ __forceinline__ void ns_be(const uint32_t* __restrict__ p, uint32_t (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = bswap32(p[i]);
  o[7] = p[7] << 24;
}

__global__ __launch_bounds__(256) void k_verify_ns_fold(const VerifyProof* __restrict__ proofs, uint32_t n,
                                                        const uint32_t* __restrict__ ns,
                                                        const uint8_t* __restrict__ leaf_ok,
                                                        uint32_t* __restrict__ leaf_rec, uint64_t total_leaves,
                                                        const uint32_t* __restrict__ node_rec,
                                                        const uint32_t* __restrict__ root_rec,
                                                        uint8_t* __restrict__ ok_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const VerifyProof pr = proofs[i];
  const int64_t start = pr.start, end = pr.end;
  const uint32_t kind = pr.pad;
  uint32_t nid[8];
  ns_be(ns + (uint64_t)i * 8, nid);
  uint32_t want[kNodeWords];
  load_node(root_rec + (uint64_t)i * kNodeWords, want);
  if (start == end) {
    // the empty proof: a namespace outside the root's range has no leaves in the tree
    bool good = kind == 0 && pr.nleaves == 0 && pr.nnodes == 0;
    uint32_t rmin[8], rmax[8];
    ns_min_be(want, rmin);
    ns_max_be(want, rmax);
    good = good && (ns_greater(rmin, nid) || ns_greater(nid, rmax));
    ok_out[i] = good ? 1 : 0;
    return;
  }
  const uint32_t nl = (uint32_t)__popc((uint32_t)pr.start);
  bool good = kind <= 1 && start >= 0 && end > start;
  if (kind == 0) good = good && (uint64_t)(end - start) == pr.nleaves && pr.nnodes >= nl;
  else good = good && end == start + 1 && pr.nleaves == 0 && pr.nnodes >= nl + 1;
  if (!good) {
    ok_out[i] = 0;
    return;
  }
  const uint32_t* nodes = node_rec + pr.node0 * kNodeWords;
  const uint32_t nnodes = pr.nnodes - kind;  // without the leaf hash
  uint32_t* rec;
  uint32_t cnt;
  if (kind == 0) {
    rec = leaf_rec + pr.leaf0 * kNodeWords;
    cnt = pr.nleaves;
    for (uint32_t j = 0; j < cnt; j++) good = good && leaf_ok[pr.leaf0 + j] != 0;
  } else {
    // the leaf hash: min <= max, and the namespace lies below it
    rec = leaf_rec + (total_leaves + i) * kNodeWords;
    cnt = 1;
    uint32_t lh[kNodeWords], lmin[8], lmax[8];
    load_node(nodes + (uint64_t)nnodes * kNodeWords, lh);
    ns_min_be(lh, lmin);
    ns_max_be(lh, lmax);
    good = good && !ns_greater(lmin, lmax) && ns_greater(lmin, nid);
    store_node(rec, lh);
  }
  // completeness: nothing of the namespace lies under a sibling
  for (uint32_t j = 0; j < nnodes; j++) {
    uint32_t t[kNodeWords], b[8];
    load_node(nodes + (uint64_t)j * kNodeWords, t);
    if (j < nl) {
      ns_max_be(t, b);
      good = good && ns_greater(nid, b);
    } else {
      ns_min_be(t, b);
      good = good && ns_greater(b, nid);
    }
  }
  uint32_t levels = 0;  // est = 2^levels >= end
  while (((uint64_t)1 << levels) < (uint64_t)end) levels++;
  uint32_t lo = (uint32_t)start;
  uint32_t li = nl;           // left nodes not yet used: nodes[0 .. li), taken from the back
  uint32_t ri = nl;           // next right node: nodes[ri .. nnodes)
  uint32_t level = 0, j = 0, np = 0, m = 0;
  bool pre = false, app = false, open = false;  // open: the level's pairs are set up
  const uint32_t *lp = nullptr, *rp = nullptr;
  for (;;) {
    // the lane's next pair: (a, b) -> rec[j]
    const uint32_t *a = nullptr, *b = nullptr;
    uint32_t* o = nullptr;
    for (;;) {
      if (level == levels) {  // at the top: every remaining node is a right sibling
        if (ri < nnodes) {
          a = rec;
          b = nodes + (uint64_t)ri * kNodeWords;
          o = rec;
          ri++;
        }
        break;
      }
      if (!open) {
        pre = lo & 1u;
        if (pre) lp = nodes + (uint64_t)(--li) * kNodeWords;
        m = cnt + (pre ? 1u : 0u);
        app = (m & 1u) && ri < nnodes;
        if (app) rp = nodes + (uint64_t)(ri++) * kNodeWords;
        m += app ? 1u : 0u;
        np = m >> 1;
        j = 0;
        open = true;
      }
      if (j < np) {
        const uint32_t ea = 2 * j, eb = 2 * j + 1;  // elements of the level: [left] records [right]
        a = (pre && ea == 0) ? lp : rec + (uint64_t)(ea - (pre ? 1u : 0u)) * kNodeWords;
        b = (app && eb == m - 1) ? rp : rec + (uint64_t)(eb - (pre ? 1u : 0u)) * kNodeWords;
        o = rec + (uint64_t)j * kNodeWords;
        j++;
        break;
      }
      // level done: an odd last element (never an appended one) moves up unchanged
      if (m & 1u) {
        const uint32_t src = m - 1 - (pre ? 1u : 0u);
        if (src != np) {
          uint32_t t[kNodeWords];
          load_node(rec + (uint64_t)src * kNodeWords, t);
          store_node(rec + (uint64_t)np * kNodeWords, t);
        }
      }
      cnt = np + (m & 1u);
      lo >>= 1;
      level++;
      open = false;
    }
    if (!o) break;
    uint32_t L[kNodeWords], R[kNodeWords], out[kNodeWords];
    load_node(a, L);
    load_node(b, R);
    good = verify_hash_node(L, R, out) && good;
    store_node(o, out);
  }
  uint32_t got[kNodeWords];
  load_node(rec, got);
#pragma unroll
  for (int q = 0; q < 22; q++) good = good && got[q] == want[q];
  good = good && ((got[22] ^ want[22]) & 0xFFFFu) == 0;
  ok_out[i] = good ? 1 : 0;
}

}  // namespace

VerifyNsWork verify_ns_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n) {
  VerifyNsWork w;
  w.v = verify_carve(work, total_leaves + n, total_nodes, n);
  w.leaf_ok = work ? static_cast<uint8_t*>(work) + w.v.bytes : nullptr;
  w.bytes = w.v.bytes + align256((size_t)(total_leaves ? total_leaves : 1));
  return w;
}

hipError_t launch_verify_ns(const VerifyNsWork& w, const uint8_t* d_leaves, uint64_t total_leaves,
                            const uint8_t* d_nodes, uint64_t total_nodes, const uint8_t* d_roots, uint32_t n,
                            uint8_t* d_ok, int stages, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (stages & kVerifyRepack) {
    const hipError_t e = launch_verify(w.v, d_leaves, total_leaves, d_nodes, total_nodes, d_roots, n, d_ok,
                                       kVerifyRepack, s);
    if (e != hipSuccess) return e;
  }
  if ((stages & kVerifyLeaves) && total_leaves)
    hipLaunchKernelGGL(k_verify_ns_leaves, dim3((uint32_t)((total_leaves + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(d_leaves), w.v.leaf_proof, w.v.ns, (uint32_t)total_leaves,
                       w.v.leaf_rec, w.leaf_ok);
  if (stages & kVerifyFold)
    hipLaunchKernelGGL(k_verify_ns_fold, dim3((n + 255) / 256), dim3(256), 0, s, w.v.proofs, n, w.v.ns, w.leaf_ok,
                       w.v.leaf_rec, total_leaves, w.v.node_rec, w.v.node_rec + total_nodes * kNodeWords, d_ok);
  return hipGetLastError();
}

}  // namespace cel
