// nmt Proof.VerifyInclusion for a batch of range proofs (celestia_eds/proof.py states the
// recursive form; tests/nmt_ref.py the bottom-up one used here), and the scatter of accepted
// samples into a resident EDS.
//
//   k_verify_repack  proof nodes and roots arrive packed at 90 bytes (any alignment): into
//                    96-byte records, one lane per dword
//   k_verify_leaves  one lane per leaf of the whole batch: ns || ns || SHA256(0x00 || ns ||
//                    share) with the proof's namespace (not the share's prefix) into the
//                    proof's leaf records
//   k_verify_fold    one lane per proof: the run of nodes covering [start, end) is folded
//                    level by level in place in the proof's own leaf records, left siblings
//                    prepended where the run starts odd, right siblings appended where it
//                    ends odd, the last node moving up unchanged when no right sibling is
//                    left; verdict = folded node == root over 90 bytes
//
// Every input is untrusted: a malformed proof is verdict 0, never a fault. Each lane touches
// its own proof's leaf records [leaf0, leaf0 + nleaves), node records [node0, node0 + nnodes)
// and root record only; the host (api_verify.cpp) derives those ranges from checked offsets.
#include <hip/hip_runtime.h>

#define CEL_VERIFY_DEVICE
#include "cel_internal.hpp"
#include "nmt_verify.hpp"

namespace cel {
namespace {

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

// leaves: total shares of 512 bytes (16-byte aligned); leaf_proof[i] = the proof of leaf i;
// ns: 8 dwords per proof; rec: the leaf records, leaf i at record i.
__global__ __launch_bounds__(256) void k_verify_leaves(const uint32_t* __restrict__ leaves,
                                                       const uint32_t* __restrict__ leaf_proof,
                                                       const uint32_t* __restrict__ ns, uint32_t total,
                                                       uint32_t* __restrict__ rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t* np = ns + (uint64_t)leaf_proof[i] * 8;
  uint32_t n[8];
  const uint4 a = reinterpret_cast<const uint4*>(np)[0], b = reinterpret_cast<const uint4*>(np)[1];
  n[0] = a.x; n[1] = a.y; n[2] = a.z; n[3] = a.w; n[4] = b.x; n[5] = b.y; n[6] = b.z; n[7] = b.w & 0xFFu;
  bool par = n[7] == 0xFFu;
#pragma unroll
  for (int q = 0; q < 7; q++) par = par && (n[q] == 0xFFFFFFFFu);
  uint32_t st[8];
  leaf_hash_ns(st, leaves + (uint64_t)i * (kShare / 4), n, par);
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

// --------------------------------------------------------------------- fold

// One lane per proof. The lane's state is the level, the count of records its run holds
// in rec[leaf0 ..], and the cursors into its left and right proof nodes; each turn of the
// outer loop finds the lane's next pair and hashes it, so lanes of different depth and
// length meet on the one HashNode in the loop.
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
  uint32_t levels = 0;  // est = 2^levels >= end
  while (((uint64_t)1 << levels) < (uint64_t)end) levels++;
  uint32_t* rec = leaf_rec + pr.leaf0 * kNodeWords;
  const uint32_t* nodes = node_rec + pr.node0 * kNodeWords;
  uint32_t cnt = pr.nleaves;  // records of the run at this level
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
        if (ri < pr.nnodes) {
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
        app = (m & 1u) && ri < pr.nnodes;
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
  uint32_t got[kNodeWords], want[kNodeWords];
  load_node(rec, got);
  load_node(root_rec + (uint64_t)i * kNodeWords, want);
#pragma unroll
  for (int q = 0; q < 22; q++) good = good && got[q] == want[q];
  good = good && ((got[22] ^ want[22]) & 0xFFFFu) == 0;
  ok_out[i] = good ? 1 : 0;
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

hipError_t launch_place_shares(const uint8_t* d_shares, const uint32_t* d_src, const uint32_t* d_dst, uint32_t n,
                               uint8_t* d_eds, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(k_place_shares, dim3((uint32_t)(((uint64_t)n * 32 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(d_shares), d_src, d_dst, n, reinterpret_cast<uint4*>(d_eds));
  return hipGetLastError();
}

}  // namespace cel
