// nmt Proof.VerifyInclusion and Proof.VerifyNamespace for a batch of proofs
// (celestia_eds/proof.py states the recursive form and the namespace rules; tests/nmt_ref.py
// the bottom-up fold used here), and the scatter of accepted samples into a resident EDS.
//
//   k_verify_repack     proof nodes and roots arrive packed at 90 bytes (any alignment): into
//                       96-byte records, one lane per dword
//   k_verify_leaves     one lane per leaf of the whole batch (verify_leaf): ns || ns ||
//                       SHA256(0x00 || ns || share) with the proof's namespace (not the share's
//                       prefix) into the proof's leaf records
//   k_verify_ns_leaves  the same, and one byte per leaf: do the share's first 29 bytes equal
//                       the proof's namespace? (celestia-node hands nmt share[:29] || share,
//                       and nmt checks that prefix against the queried namespace)
//   k_verify_fold       one lane per proof (fold_run): the run of nodes covering [start, end)
//                       is folded level by level in place in the proof's own leaf records, left
//                       siblings prepended where the run starts odd, right siblings appended
//                       where it ends odd, the last node moving up unchanged when no right
//                       sibling is left; verdict = folded node == root over 90 bytes
//   k_verify_ns_fold    one lane per proof, the same fold. Before it the lane checks the
//                       proof's shape by kind, ANDs its leaves' bytes, and checks completeness:
//                       of the proof's nodes the first popcount(start) are the left siblings
//                       (each must end below the namespace), all others right siblings (each
//                       must begin above it); the fold uses every one of them on that side. An
//                       absence proof's last node is its leaf hash: it is copied into the
//                       proof's own record behind the leaf records and folded as the single
//                       leaf. The empty proof is decided from the root's range alone.
//
// Every input is untrusted: a malformed proof is verdict 0, never a fault. Each lane touches
// its own proof's leaf records [leaf0, leaf0 + nleaves), node records [node0, node0 + nnodes)
// and root record only (the namespace verifier also its own record total_leaves + i); the host
// (api_verify.cpp) derives those ranges from checked offsets, and a malformed proof leaves
// before it touches any of them but the root.
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "nmt_device.hpp"
#include "nmt_verify.hpp"

namespace cel {
namespace {

// Leaf digest of a 512-byte share under a namespace given apart from it: the message is
// 0x00 || ns(29) || share(512), 9 blocks; n = the namespace's 8 little-endian dwords (bytes
// 29..31 zero). The word shuffling is leaf_hash's (nmt_device.hpp) with the namespace words
// taken from n. Lanes of one wave that all carry the parity namespace start block 0 from
// the parity midstate.
__device__ __forceinline__ void leaf_hash_ns(uint32_t (&st)[8], const uint32_t* __restrict__ sh,
                                             const uint32_t (&n)[8], bool par) {
  sha256_init(st);
  uint32_t w[16];
  uint32_t nx[17];
  {  // block 0: 0x00 || ns || share[0:34]
    uint32_t s[9];
    const uint4* p4 = reinterpret_cast<const uint4*>(sh);
    const uint4 v0 = p4[0], v1 = p4[1];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w; s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
    s[8] = sh[8];
#pragma unroll
    for (int i = 8; i < 16; i++) w[i] = perm(s[i - 8], s[i - 7], 0x06070001u);
    const uint32_t sh01 = perm(0u, s[0], 0x0C0C0001u);  // share bytes 0, 1 = message bytes 30, 31
    if (__all(par)) {
#pragma unroll
      for (int i = 0; i < 7; i++) w[i] = kLeafParPrefix[i];
      w[7] = 0xFFFF0000u | sh01;
      sha256_compress_from<7>(st, mid_regs(kLeafParMid), w);
    } else {
      w[0] = perm(0u, n[0], 0x0C000102u);
#pragma unroll
      for (int i = 1; i < 7; i++) w[i] = perm(n[i - 1], n[i], 0x07000102u);
      w[7] = perm(n[6], n[7], 0x07000C0Cu) | sh01;
      sha256_compress(st, w);
    }
  }
#pragma unroll 1
  for (int b = 1; b < 8; b++) {  // blocks 1..7: share bytes [64b-30, 64b+34)
    const uint32_t* base = sh + 16 * b - 8;
    const uint4* p4 = reinterpret_cast<const uint4*>(base);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint4 v = p4[i];
      nx[4 * i] = v.x; nx[4 * i + 1] = v.y; nx[4 * i + 2] = v.z; nx[4 * i + 3] = v.w;
    }
    nx[16] = base[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = perm(nx[i], nx[i + 1], 0x06070001u);
    sha256_compress(st, w);
  }
  {  // block 8: share[482:512] || 0x80 || 0... || len
    const uint4* p4 = reinterpret_cast<const uint4*>(sh + 120);
    const uint4 v0 = p4[0], v1 = p4[1];
    nx[0] = v0.x; nx[1] = v0.y; nx[2] = v0.z; nx[3] = v0.w; nx[4] = v1.x; nx[5] = v1.y; nx[6] = v1.z; nx[7] = v1.w;
#pragma unroll
    for (int i = 0; i < 7; i++) w[i] = perm(nx[i], nx[i + 1], 0x06070001u);
    w[7] = perm(nx[7], 0x80u, 0x0607000Cu);
#pragma unroll
    for (int i = 8; i < 15; i++) w[i] = 0u;
    w[15] = 542u * 8u;
    sha256_compress(st, w);
  }
}

// Big-endian words of a record's min namespace (bytes 0..28) and max namespace (29..57);
// word 7 holds the last byte in its top byte. Comparing the 8 words in order is the
// 29-byte lexicographic compare.
__device__ __forceinline__ void ns_min_be(const uint32_t (&r)[kNodeWords], uint32_t (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = bswap32(r[i]);
  o[7] = r[7] << 24;
}
__device__ __forceinline__ void ns_max_be(const uint32_t (&r)[kNodeWords], uint32_t (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = bswap32(__builtin_amdgcn_alignbyte(r[8 + i], r[7 + i], 1));
  o[7] = (r[14] >> 8) << 24;
}
// The same words of a namespace given as 8 little-endian dwords (bytes 29..31 zero).
__device__ __forceinline__ void ns_be(const uint32_t* __restrict__ p, uint32_t (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = bswap32(p[i]);
  o[7] = p[7] << 24;
}
// a > b?
__device__ __forceinline__ bool ns_greater(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  int res = 0;
#pragma unroll
  for (int i = 0; i < 8; i++)
    if (res == 0 && a[i] != b[i]) res = a[i] > b[i] ? 1 : -1;
  return res > 0;
}

// nmt HashNode with IgnoreMaxNamespace on untrusted children, as proof.py's _nmt_node: false
// (nothing hashed into out that matters) when L.max > R.min; minNs = L.min; maxNs = L.max if
// R.min is the parity namespace, else the larger of L.max and R.max.
__device__ __forceinline__ bool verify_hash_node(const uint32_t (&L)[kNodeWords], const uint32_t (&R)[kNodeWords],
                                                 uint32_t (&out)[kNodeWords]) {
  uint32_t lmax[8], rmin[8], rmax[8];
  ns_max_be(L, lmax);
  ns_min_be(R, rmin);
  ns_max_be(R, rmax);
  const bool ordered = !ns_greater(lmax, rmin);
  bool rpar = rmin[7] == 0xFF000000u;
#pragma unroll
  for (int i = 0; i < 7; i++) rpar = rpar && (rmin[i] == 0xFFFFFFFFu);
  const bool from_l = rpar || !ns_greater(rmax, lmax);
  uint32_t st[8];
  sha256_init(st);
#pragma unroll 1
  for (int b = 0; b < 3; b++) {
    uint32_t w[16];
    // node_word with a run-time block index: three unrolled copies of the compression would
    // triple the loop body every lane of the fold iterates over
    if (b == 0) {
#pragma unroll
      for (int wi = 0; wi < 16; wi++) w[wi] = node_word(L, R, wi);
    } else if (b == 1) {
#pragma unroll
      for (int wi = 0; wi < 16; wi++) w[wi] = node_word(L, R, 16 + wi);
    } else {
#pragma unroll
      for (int wi = 0; wi < 16; wi++) w[wi] = node_word(L, R, 32 + wi);
    }
    sha256_compress(st, w);
  }
#pragma unroll
  for (int i = 0; i < 7; i++) out[i] = L[i];
  out[7] = (L[7] & 0xFFu) | ((from_l ? L[7] : R[7]) & 0xFFFFFF00u);
#pragma unroll
  for (int i = 8; i < 14; i++) out[i] = from_l ? L[i] : R[i];
  out[14] = (from_l ? L[14] : R[14]) & 0xFFFFu;
  put_digest(out, st);
  return ordered;
}

// ------------------------------------------------------------------- repack

// Record dword w of packed node j: bytes [90j + 4w, 90j + 4w + 4) of src, zero past byte 89.
// Only aligned dwords that hold at least one byte of the node are loaded, so no load leaves
// the page of a byte the caller owns.
__global__ __launch_bounds__(256) void k_verify_repack(const uint8_t* __restrict__ nodes, uint64_t nnodes,
                                                       const uint8_t* __restrict__ roots,
                                                       const VerifyProof* __restrict__ proofs, uint32_t n,
                                                       uint32_t* __restrict__ rec) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (nnodes + n) * kNodeWords) return;
  const uint64_t j = t / kNodeWords;
  const uint32_t w = (uint32_t)(t % kNodeWords);
  uint32_t v = 0;
  if (w < 23) {
    // record nnodes + i = the root of proof i
    const uint8_t* src = j < nnodes ? nodes + j * kNode : roots + (uint64_t)proofs[j - nnodes].root * kNode;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) + 4 * w;  // first byte wanted
    const uintptr_t end = reinterpret_cast<uintptr_t>(src) + kNode;
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - sh);
    const uint32_t lo = p[0];  // holds byte a
    const uint32_t hi = (sh != 0 && a - sh + 4 < end) ? p[1] : 0u;
    v = __builtin_amdgcn_alignbyte(hi, lo, sh);
    if (w == 22) v &= 0xFFFFu;
  }
  rec[t] = v;
}

// ------------------------------------------------------------------- leaves

// Leaf i of the batch. leaves: shares of 512 bytes (16-byte aligned); leaf_proof[i] = the
// proof of leaf i; ns: 8 dwords per proof; rec: the leaf records, leaf i at record i. With
// kPrefix, leaf_ok[i] = does the share start with the proof's namespace?
template <bool kPrefix>
__device__ __forceinline__ void verify_leaf(uint32_t i, const uint32_t* __restrict__ leaves,
                                            const uint32_t* __restrict__ leaf_proof, const uint32_t* __restrict__ ns,
                                            uint32_t* __restrict__ rec, uint8_t* __restrict__ leaf_ok) {
  const uint32_t* np = ns + (uint64_t)leaf_proof[i] * 8;
  uint32_t n[8];
  const uint4 a = reinterpret_cast<const uint4*>(np)[0], b = reinterpret_cast<const uint4*>(np)[1];
  n[0] = a.x; n[1] = a.y; n[2] = a.z; n[3] = a.w; n[4] = b.x; n[5] = b.y; n[6] = b.z; n[7] = b.w & 0xFFu;
  bool par = n[7] == 0xFFu;
#pragma unroll
  for (int q = 0; q < 7; q++) par = par && (n[q] == 0xFFFFFFFFu);
  const uint32_t* sh = leaves + (uint64_t)i * (kShare / 4);
  if (kPrefix) {  // the share's own namespace against the proof's
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

__global__ __launch_bounds__(256) void k_verify_leaves(const uint32_t* __restrict__ leaves,
                                                       const uint32_t* __restrict__ leaf_proof,
                                                       const uint32_t* __restrict__ ns, uint32_t total,
                                                       uint32_t* __restrict__ rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) verify_leaf<false>(i, leaves, leaf_proof, ns, rec, nullptr);
}

__global__ __launch_bounds__(256) void k_verify_ns_leaves(const uint32_t* __restrict__ leaves,
                                                          const uint32_t* __restrict__ leaf_proof,
                                                          const uint32_t* __restrict__ ns, uint32_t total,
                                                          uint32_t* __restrict__ rec, uint8_t* __restrict__ leaf_ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) verify_leaf<true>(i, leaves, leaf_proof, ns, rec, leaf_ok);
}

// --------------------------------------------------------------------- fold

// Folds the cnt records at rec, which cover leaves [start, end) of a tree, up to the root with
// the proof's nodes: nodes[0 .. nl) are the left siblings, nodes[nl .. nnodes) the right ones.
// The folded node is left in rec[0]; false if a HashNode met children out of order. The
// caller has checked 0 <= start < end, cnt == end - start (a lane reads nothing past its cnt
// records) and nl == popcount(start) <= nnodes (the left cursor never passes nodes[0]).
//
// The lane's state is the level, the count of records its run holds, and the cursors into its
// left and right nodes; each turn of the outer loop finds the lane's next pair and hashes it,
// so lanes of different depth and length meet on the one HashNode in the loop.
__device__ __forceinline__ bool fold_run(uint32_t* rec, uint32_t cnt, uint32_t start, uint32_t end,
                                         const uint32_t* nodes, uint32_t nl, uint32_t nnodes) {
  uint32_t levels = 0;  // est = 2^levels >= end
  while (((uint64_t)1 << levels) < (uint64_t)end) levels++;
  bool ordered = true;
  uint32_t lo = start;
  uint32_t li = nl;  // left nodes not yet used: nodes[0 .. li), taken from the back
  uint32_t ri = nl;  // next right node: nodes[ri .. nnodes)
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
    ordered = verify_hash_node(L, R, out) && ordered;
    store_node(o, out);
  }
  return ordered;
}

// Does the record at rec equal the root `want` over its 90 bytes?
__device__ __forceinline__ bool root_equal(const uint32_t* rec, const uint32_t (&want)[kNodeWords]) {
  uint32_t got[kNodeWords];
  load_node(rec, got);
  bool same = true;
#pragma unroll
  for (int q = 0; q < 22; q++) same = same && got[q] == want[q];
  return same && ((got[22] ^ want[22]) & 0xFFFFu) == 0;
}

__global__ __launch_bounds__(256) void k_verify_fold(const VerifyProof* __restrict__ proofs, uint32_t n,
                                                     uint32_t* __restrict__ leaf_rec,
                                                     const uint32_t* __restrict__ node_rec,
                                                     const uint32_t* __restrict__ root_rec,
                                                     uint8_t* __restrict__ ok_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const VerifyProof pr = proofs[i];
  const int64_t start = pr.start, end = pr.end;
  const uint32_t nl = (uint32_t)__popc((uint32_t)pr.start);
  bool good = start >= 0 && end > start && (uint64_t)(end - start) == pr.nleaves && pr.nnodes >= nl;
  if (!good) {
    ok_out[i] = 0;
    return;
  }
  uint32_t* rec = leaf_rec + pr.leaf0 * kNodeWords;
  good = fold_run(rec, pr.nleaves, (uint32_t)start, (uint32_t)end, node_rec + pr.node0 * kNodeWords, nl, pr.nnodes);
  uint32_t want[kNodeWords];
  load_node(root_rec + (uint64_t)i * kNodeWords, want);
  const bool same = root_equal(rec, want);  // unconditional: no branch around the loads
  ok_out[i] = good && same ? 1 : 0;
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
  good = fold_run(rec, cnt, (uint32_t)start, (uint32_t)end, nodes, nl, nnodes) && good;
  const bool same = root_equal(rec, want);  // unconditional: no branch around the loads
  ok_out[i] = good && same ? 1 : 0;
}

// ------------------------------------------------------------------ scatter

// Share src[t] of `shares` into cell dst[t] of the EDS, 32 lanes of 16 bytes per share.
__global__ __launch_bounds__(256) void k_place_shares(const uint4* __restrict__ shares, const uint32_t* __restrict__ src,
                                                      const uint32_t* __restrict__ dst, uint32_t n,
                                                      uint4* __restrict__ eds) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t s = (uint32_t)(t >> 5), q = (uint32_t)(t & 31);
  if (s >= n) return;
  eds[(uint64_t)dst[s] * 32 + q] = shares[(uint64_t)src[s] * 32 + q];
}

}  // namespace

VerifyWork verify_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n) {
  Carver c(work);
  VerifyWork w;
  w.proofs = c.take<VerifyProof>((size_t)n * sizeof(VerifyProof));
  w.ns = c.take<uint32_t>((size_t)n * 32);
  w.leaf_proof = c.take<uint32_t>((size_t)total_leaves * 4);
  w.head_bytes = c.size();
  w.leaf_rec = c.take<uint32_t>((size_t)total_leaves * kNodeWords * 4);
  w.node_rec = c.take<uint32_t>((size_t)(total_nodes + n) * kNodeWords * 4);
  w.bytes = c.size();
  return w;
}

VerifyNsWork verify_ns_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n) {
  VerifyNsWork w;
  w.v = verify_carve(work, total_leaves + n, total_nodes, n);
  w.leaf_ok = work ? static_cast<uint8_t*>(work) + w.v.bytes : nullptr;
  w.bytes = w.v.bytes + align256((size_t)(total_leaves ? total_leaves : 1));
  return w;
}

hipError_t launch_verify(const VerifyWork& w, const uint8_t* d_leaves, uint64_t total_leaves, const uint8_t* d_nodes,
                         uint64_t total_nodes, const uint8_t* d_roots, uint32_t n, uint8_t* d_ok, int stages,
                         hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (stages & kVerifyRepack) {
    const uint64_t lanes = (total_nodes + n) * kNodeWords;
    hipLaunchKernelGGL(k_verify_repack, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, s, d_nodes, total_nodes,
                       d_roots, w.proofs, n, w.node_rec);
  }
  if ((stages & kVerifyLeaves) && total_leaves)
    hipLaunchKernelGGL(k_verify_leaves, dim3((uint32_t)((total_leaves + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(d_leaves), w.leaf_proof, w.ns, (uint32_t)total_leaves,
                       w.leaf_rec);
  if (stages & kVerifyFold)
    hipLaunchKernelGGL(k_verify_fold, dim3((n + 255) / 256), dim3(256), 0, s, w.proofs, n, w.leaf_rec, w.node_rec,
                       w.node_rec + total_nodes * kNodeWords, d_ok);
  return hipGetLastError();
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

hipError_t launch_place_shares(const uint8_t* d_shares, const uint32_t* d_src, const uint32_t* d_dst, uint32_t n,
                               uint8_t* d_eds, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(k_place_shares, dim3((uint32_t)(((uint64_t)n * 32 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(d_shares), d_src, d_dst, n, reinterpret_cast<uint4*>(d_eds));
  return hipGetLastError();
}

}  // namespace cel
