// The batched NMT proof verifier's device interface (nmt_verify.hip), used by api_verify.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cel {

// One proof of a batch, as the fold kernel reads it. Ranges are in records: the proof's
// leaves are leaf records [leaf0, leaf0 + nleaves), its nodes node records [node0, node0 +
// nnodes), its root is packed root `root` of the caller's roots (repacked into root record i).
// pad: 0 for the inclusion verifier; the namespace verifier keeps the proof's kind there.
struct VerifyProof {
  int32_t start, end;
  uint32_t nleaves, nnodes;
  uint64_t leaf0, node0;
  uint32_t root, pad;
};
static_assert(sizeof(VerifyProof) == 40, "VerifyProof layout");

// The workspace of one batch. The head [0, head_bytes) is filled by the host and uploaded
// in one copy: the proofs, a 32-byte namespace per proof (29 bytes, zero padded), and the
// proof index of every leaf. Behind it the 96-byte records of the leaves and of the nodes
// followed by one root per proof.
struct VerifyWork {
  VerifyProof* proofs;
  uint32_t* ns;
  uint32_t* leaf_proof;
  size_t head_bytes;
  uint32_t* leaf_rec;
  uint32_t* node_rec;
  size_t bytes;
};
// On a null `work` every pointer is null and `bytes` is the workspace's size.
VerifyWork verify_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n);

enum { kVerifyRepack = 1, kVerifyLeaves = 2, kVerifyFold = 4, kVerifyAll = 7 };
// The stages of a batch whose head is in place (stages: a measurement runs them apart).
// d_leaves: 16-byte aligned shares; d_nodes, d_roots: packed 90-byte nodes, any alignment.
hipError_t launch_verify(const VerifyWork& w, const uint8_t* d_leaves, uint64_t total_leaves, const uint8_t* d_nodes,
                         uint64_t total_nodes, const uint8_t* d_roots, uint32_t n, uint8_t* d_ok, int stages,
                         hipStream_t s);
// Share d_src[t] of d_shares into cell d_dst[t] (row-major index) of d_eds, t < n.
hipError_t launch_place_shares(const uint8_t* d_shares, const uint32_t* d_src, const uint32_t* d_dst, uint32_t n,
                               uint8_t* d_eds, hipStream_t s);

// nmt Proof.VerifyNamespace for a batch (nmt_verify_ns.hip). The table is the inclusion
// verifier's, with the proof's kind (CEL_NS_INCLUSION / CEL_NS_ABSENCE) in VerifyProof::pad.
// Behind the total_leaves leaf records lies one more record per proof, record total_leaves + i,
// where an absence proof's fold starts from its leaf hash; leaf_ok holds one byte per leaf:
// does the share start with its proof's namespace?
struct VerifyNsWork {
  VerifyWork v;
  uint8_t* leaf_ok;
  size_t bytes;
};
VerifyNsWork verify_ns_carve(void* work, uint64_t total_leaves, uint64_t total_nodes, uint32_t n);
// The stages as in launch_verify: repack (the inclusion verifier's kernel), leaves, fold.
hipError_t launch_verify_ns(const VerifyNsWork& w, const uint8_t* d_leaves, uint64_t total_leaves,
                            const uint8_t* d_nodes, uint64_t total_nodes, const uint8_t* d_roots, uint32_t n,
                            uint8_t* d_ok, int stages, hipStream_t s);

}  // namespace cel

// Device code that nmt_verify.hip and nmt_verify_ns.hip share; a file that wants it defines
// CEL_VERIFY_DEVICE before the include.
#ifdef CEL_VERIFY_DEVICE
#include "nmt_device.hpp"

namespace cel {

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

}  // namespace cel
#endif
