// Device building blocks of the NMT and RFC-6962 hashing shared by nmt_kernels.hip (the EDS
// commit), nmt_slab.hip (the row-sharded mode), nmt_trees.hip (single trees, axes roots,
// exported trees) and blob_commit.hip (blob share commitments): 96-byte node records, the
// leaf hash of a 512-byte share, the namespace compares, HashNode with IgnoreMaxNamespace,
// the inner-node step of a tree level (hash_pair), the digest-only hash of a node outside Q0
// (hash_parity_node), and the RFC-6962 leaf / inner hashes.
// One message per lane.
#pragma once
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "sha256_device.hpp"

namespace cel {

__device__ __forceinline__ void load_node(const uint32_t* p, uint32_t (&n)[kNodeWords]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const uint4 v = q[i];
    n[4 * i] = v.x; n[4 * i + 1] = v.y; n[4 * i + 2] = v.z; n[4 * i + 3] = v.w;
  }
}

__device__ __forceinline__ void store_node(uint32_t* p, const uint32_t (&n)[kNodeWords]) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < 6; i++) q[i] = make_uint4(n[4 * i], n[4 * i + 1], n[4 * i + 2], n[4 * i + 3]);
}

// Node dwords 14..23 from the 8 big-endian digest words (digest = node bytes 58..89).
// nd14 keeps its low 16 bits (the last two max-namespace bytes).
__device__ __forceinline__ void put_digest(uint32_t (&nd)[kNodeWords], const uint32_t (&st)[8]) {
  uint32_t sw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) sw[i] = bswap32(st[i]);
  nd[14] = (nd[14] & 0xFFFFu) | (sw[0] << 16);
#pragma unroll
  for (int i = 15; i <= 21; i++) nd[i] = __builtin_amdgcn_alignbyte(sw[i - 14], sw[i - 15], 2);
  nd[22] = sw[7] >> 16;
  nd[23] = 0;
}

// --------------------------------------------------------------------- leaves

// Leaf message: 0x00 || ns(29) || share(512) = 542 B -> 9 blocks.
// sh = the share's little-endian dwords; ns = share[0:29] for Q0 cells, 0xFF*29 else.
// Message word at byte p >= 32 is share bytes q..q+3 with q = p - 30 (q = 2 mod 4):
// bytes 2,3 of dword (q-2)/4 and bytes 0,1 of the next -> one v_perm_b32 (and the
// byte swap to big-endian comes for free in the same select).
// Parity cells: message bytes 0..27 are 0x00 || 0xFF*27 (ns = 0xFF*29 continues into w7).
constexpr uint32_t kLeafParPrefix[7] = {0x00FFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                        0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
constexpr ShaMid kLeafParMid = sha_midstate(kLeafParPrefix, 7);

// PF (prefetch): the next block's words are loaded while the current block is compressed.
// At one or two waves per SIMD (a single square's commit, a rank's slab) nothing else
// covers a block's load latency, which the plain form exposes nine times per leaf; at
// batch occupancy other waves cover it and the 17 extra VGPRs cost 1.5-3 %
// (profiles/r2_nmt_leaf_prefetch_ab.txt), so the batch keeps PF = false.
// What a call site knows about its cells at compile time. kAny: the class is q0, per lane,
// with the wave-uniform shortcut below. kQ0 / kParity: every lane of every wave is of that
// class (the batch's kernels per tile class, nmt_kernels.hip); q0 is not read, and block 0
// has one form.
enum class Cells { kAny, kQ0, kParity };

template <bool PF, Cells C = Cells::kAny>
__device__ __forceinline__ void leaf_hash(uint32_t (&st)[8], const uint32_t* __restrict__ sh, bool q0) {
  if (C != Cells::kAny) q0 = C == Cells::kQ0;
  sha256_init(st);
  uint32_t w[16];
  uint32_t nx[17];  // PF: the next block's share dwords
  auto load17 = [&](int b) {  // share bytes [64b-30, 64b+34) for block b = 1..7
    const uint32_t* base = sh + 16 * b - 8;
    const uint4* p4 = reinterpret_cast<const uint4*>(base);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint4 v = p4[i];
      nx[4 * i] = v.x; nx[4 * i + 1] = v.y; nx[4 * i + 2] = v.z; nx[4 * i + 3] = v.w;
    }
    nx[16] = base[16];
  };
  {  // block 0: 0x00 || ns || share[0:34]
    uint32_t s[9];
    const uint4* p4 = reinterpret_cast<const uint4*>(sh);
    const uint4 v0 = p4[0], v1 = p4[1];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w; s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
    s[8] = sh[8];
    if (PF) load17(1);
#pragma unroll
    for (int i = 8; i < 16; i++) w[i] = perm(s[i - 8], s[i - 7], 0x06070001u);
    // wave-uniform parity cells: rounds 0..6 are one constant
    if (C == Cells::kParity || (C == Cells::kAny && __all(!q0))) {
#pragma unroll
      for (int i = 0; i < 7; i++) w[i] = kLeafParPrefix[i];
      w[7] = 0xFFFF0000u | perm(0u, s[0], 0x0C0C0001u);
      sha256_compress_from<7>(st, mid_regs(kLeafParMid), w);
    } else {
      if (q0) {
        w[0] = perm(0u, s[0], 0x0C000102u);
#pragma unroll
        for (int i = 1; i < 7; i++) w[i] = perm(s[i - 1], s[i], 0x07000102u);
        w[7] = perm(s[6], s[7], 0x07000C0Cu) | perm(0u, s[0], 0x0C0C0001u);
      } else {
#pragma unroll
        for (int i = 0; i < 7; i++) w[i] = kLeafParPrefix[i];
        w[7] = 0xFFFF0000u | perm(0u, s[0], 0x0C0C0001u);
      }
      sha256_compress(st, w);
    }
  }
#pragma unroll 1
  for (int b = 1; b < 8; b++) {  // blocks 1..7: share bytes [64b-30, 64b+34)
    if (!PF) load17(b);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = perm(nx[i], nx[i + 1], 0x06070001u);
    if (PF) {
      if (b < 7) {
        load17(b + 1);
      } else {  // the last block's 8 dwords
        const uint4* p4 = reinterpret_cast<const uint4*>(sh + 120);
        const uint4 v0 = p4[0], v1 = p4[1];
        nx[0] = v0.x; nx[1] = v0.y; nx[2] = v0.z; nx[3] = v0.w; nx[4] = v1.x; nx[5] = v1.y; nx[6] = v1.z; nx[7] = v1.w;
      }
    }
    sha256_compress(st, w);
  }
  {  // block 8: share[482:512] || 0x80 || 0... || len
    if (!PF) {
      const uint4* p4 = reinterpret_cast<const uint4*>(sh + 120);
      const uint4 v0 = p4[0], v1 = p4[1];
      nx[0] = v0.x; nx[1] = v0.y; nx[2] = v0.z; nx[3] = v0.w; nx[4] = v1.x; nx[5] = v1.y; nx[6] = v1.z; nx[7] = v1.w;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) w[i] = perm(nx[i], nx[i + 1], 0x06070001u);
    w[7] = perm(nx[7], 0x80u, 0x0607000Cu);
#pragma unroll
    for (int i = 8; i < 15; i++) w[i] = 0u;
    w[15] = 542u * 8u;
    sha256_compress(st, w);
  }
}

// The leaf record of one EDS cell from its leaf digest st: ns || ns || digest. The
// namespaces come from the share again (32 bytes), so a caller that keeps a leaf across
// other hashes holds its 8 digest words and not the 24-word record.
__device__ __forceinline__ void leaf_record(const uint32_t* __restrict__ sh, bool q0, const uint32_t (&st)[8],
                                            uint32_t (&nd)[kNodeWords]) {
  if (q0) {
    const uint4* p4 = reinterpret_cast<const uint4*>(sh);
    uint32_t s[8];
    const uint4 v0 = p4[0], v1 = p4[1];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w; s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
#pragma unroll
    for (int i = 0; i < 7; i++) nd[i] = s[i];
    nd[7] = (s[7] & 0xFFu) | (s[0] << 8);
#pragma unroll
    for (int i = 0; i < 6; i++) nd[8 + i] = __builtin_amdgcn_alignbyte(s[i + 1], s[i], 3);
    nd[14] = (s[6] >> 24) | ((s[7] & 0xFFu) << 8);
  } else {
#pragma unroll
    for (int i = 0; i < 14; i++) nd[i] = 0xFFFFFFFFu;
    nd[14] = 0xFFFFu;
  }
  put_digest(nd, st);
}

// Leaf node of one EDS cell: ns || ns || SHA256(0x00 || ns || share), ns = share[0:29]
// for Q0 cells and 0xFF*29 (parity namespace) otherwise.
template <bool PF>
__device__ __forceinline__ void make_leaf_node(const uint32_t* __restrict__ sh, bool q0, uint32_t (&nd)[kNodeWords]) {
  uint32_t st[8];
  leaf_hash<PF>(st, sh, q0);
  leaf_record(sh, q0, st, nd);
}

// Namespace order: is ns(a) < ns(b)? (29-byte lexicographic compare of share prefixes)
__device__ __forceinline__ bool ns_less(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {
  const uint4* pa = reinterpret_cast<const uint4*>(a);
  const uint4* pb = reinterpret_cast<const uint4*>(b);
  uint32_t x[8], y[8];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const uint4 u = pa[i], v = pb[i];
    x[4 * i] = u.x; x[4 * i + 1] = u.y; x[4 * i + 2] = u.z; x[4 * i + 3] = u.w;
    y[4 * i] = v.x; y[4 * i + 1] = v.y; y[4 * i + 2] = v.z; y[4 * i + 3] = v.w;
  }
  int res = 0;  // -1 a<b, 1 a>b
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t xa = bswap32(x[i]), yb = bswap32(y[i]);
    if (i == 7) { xa &= 0xFF000000u; yb &= 0xFF000000u; }
    if (res == 0 && xa != yb) res = xa < yb ? -1 : 1;
  }
  return res < 0;
}

// Is the record's minNs (bytes 0..28) the parity namespace 0xFF*29?
__device__ __forceinline__ bool min_is_parity(const uint32_t* __restrict__ R) {
  bool par = (R[7] & 0xFFu) == 0xFFu;
#pragma unroll
  for (int q = 0; q < 7; q++) par = par && (R[q] == 0xFFFFFFFFu);
  return par;
}

// ---------------------------------------------------------------- inner nodes

// HashNode(L, R): message 0x01 || L(90) || R(90) = 181 B -> 3 blocks.
// minNs = L.min; maxNs = (R.min == 0xFF*29) ? L.max : R.max  (IgnoreMaxNamespace).
// Parity left child (min = max = 0xFF*29, nodes of Q1-Q3): message bytes 0..55 are
// 0x01 || 0xFF*55 for every such node, so rounds 0..13 of block 0 are one constant.
constexpr uint32_t kNodeParPrefix[14] = {0x01FFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                         0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                         0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
constexpr ShaMid kNodeParMid = sha_midstate(kNodeParPrefix, 14);

__device__ __forceinline__ uint32_t node_word(const uint32_t (&L)[kNodeWords], const uint32_t (&R)[kNodeWords], int q) {
  if (q == 0) return perm(1u, L[0], 0x04000102u);
  if (q <= 21) return perm(L[q - 1], L[q], 0x07000102u);
  if (q == 22) return perm(L[21], L[22], 0x0700010Cu) | (R[0] & 0xFFu);
  if (q <= 44) return perm(R[q - 23], R[q - 22], 0x05060700u);
  if (q == 45) return perm(R[22], 0x80u, 0x05000C0Cu);
  if (q == 47) return 181u * 8u;
  return 0u;
}

// PAR_START = false leaves the wave-uniform start out: the same bytes from one form of
// block 0, for a kernel whose nodes all lie inside Q0 (a parity left child there is a Q0
// share that carries 0xFF*29 itself) and whose code size counts.
template <bool PAR_START = true>
__device__ __forceinline__ void hash_node(const uint32_t (&L)[kNodeWords], const uint32_t (&R)[kNodeWords],
                                          uint32_t (&out)[kNodeWords]) {
  uint32_t st[8];
  sha256_init(st);
  bool lpar = PAR_START && (L[14] & 0xFFFFu) == 0xFFFFu;
#pragma unroll
  for (int i = 0; i < 14; i++) lpar = lpar && (L[i] == 0xFFFFFFFFu);
  {
    uint32_t w[16];
    if (PAR_START && __all(lpar)) {  // wave-uniform: the whole wave starts block 0 at round 14
#pragma unroll
      for (int wi = 0; wi < 14; wi++) w[wi] = kNodeParPrefix[wi];
      w[14] = node_word(L, R, 14);
      w[15] = node_word(L, R, 15);
      sha256_compress_from<14>(st, mid_regs(kNodeParMid), w);
    } else {
#pragma unroll
      for (int wi = 0; wi < 16; wi++) w[wi] = node_word(L, R, wi);
      sha256_compress(st, w);
    }
  }
#pragma unroll
  for (int b = 1; b < 3; b++) {
    uint32_t w[16];
#pragma unroll
    for (int wi = 0; wi < 16; wi++) w[wi] = node_word(L, R, 16 * b + wi);
    sha256_compress(st, w);
  }
  bool rpar = (R[7] & 0xFFu) == 0xFFu;
#pragma unroll
  for (int i = 0; i < 7; i++) rpar = rpar && (R[i] == 0xFFFFFFFFu);
  // out: min from L (bytes 0..28), max from L or R (bytes 29..57)
#pragma unroll
  for (int i = 0; i < 7; i++) out[i] = L[i];
  const uint32_t X7 = rpar ? L[7] : R[7];
  out[7] = (L[7] & 0xFFu) | (X7 & 0xFFFFFF00u);
#pragma unroll
  for (int i = 8; i < 14; i++) out[i] = rpar ? L[i] : R[i];
  out[14] = (rpar ? L[14] : R[14]) & 0xFFFFu;
  put_digest(out, st);
}

// The inner-node step of every tree level: o = HashNode(in[li], in[ri]), li / ri in records.
__device__ __forceinline__ void hash_pair(const uint32_t* in, uint64_t li, uint64_t ri, uint32_t (&o)[kNodeWords]) {
  uint32_t L[kNodeWords], R[kNodeWords];
  load_node(in + li * kNodeWords, L);
  load_node(in + ri * kNodeWords, R);
  hash_node(L, R, o);
}

// ------------------------------------------- parity nodes, kept as their digests

// A node whose subtree lies outside Q0 has min = max = 0xFF*29, and so have both its
// children: the batch commit (nmt_kernels.hip) knows such a node from its position and
// keeps only its digest, the 8 big-endian SHA state words. Its message is
// 0x01 || 0xFF*58 || dl || 0xFF*58 || dr: the 48 words below with the digest bytes zero
// (tests/test_gpu_parity_records.py restates the layout). Digest bytes fall into 18 of them:
// 14, 15 (block 0), 16..22 (block 1), 37..45 (block 2).
constexpr uint32_t kParNodeWords[48] = {
    0x01FFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
    0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFF00u, 0x00000000u,
    0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x000000FFu, 0xFFFFFFFFu,
    0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu,
    0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFF000000u, 0x00000000u, 0x00000000u,
    0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00800000u, 0x00000000u, 181u * 8u};

// out = SHA256(0x01 || 0xFF*58 || dl || 0xFF*58 || dr), digests as state words. Block 0
// starts at round 14 from kNodeParMid; each of the 18 digest-carrying words is one alignbit
// of two adjacent state words (or one shift and or); the other 30 are literals, which fold
// into the schedule of rounds 16..31 (sha256_rounds_folded). No records, no namespace tests.
// COMPACT: rounds 32..63 of each block rolled (the mixed k_leaf_quad, which carries hash_node
// beside it and must stay inside the instruction cache); otherwise unrolled (k_leaf_quad_par,
// the level kernel).
template <bool COMPACT>
__device__ __forceinline__ void hash_parity_node(const uint32_t (&dl)[8], const uint32_t (&dr)[8],
                                                 uint32_t (&out)[8]) {
  constexpr int kEnd = COMPACT ? 32 : 64;
  uint32_t st[8], w[16];
  sha256_init(st);
  auto finish = [&](ShaRegs& r) {
    if (COMPACT) sha256_rounds_tail(r, w);
    sha256_add(st, r);
  };
  {
#pragma unroll
    for (int i = 0; i < 14; i++) w[i] = kParNodeWords[i];
    w[14] = kParNodeWords[14] | (dl[0] >> 24);
    w[15] = __builtin_amdgcn_alignbit(dl[0], dl[1], 24);
    ShaRegs r = mid_regs(kNodeParMid);
    sha256_rounds_folded<14, kEnd>(r, w);
    finish(r);
  }
  {
#pragma unroll
    for (int i = 0; i < 6; i++) w[i] = __builtin_amdgcn_alignbit(dl[i + 1], dl[i + 2], 24);
    w[6] = kParNodeWords[22] | (dl[7] << 8);
#pragma unroll
    for (int i = 7; i < 16; i++) w[i] = kParNodeWords[16 + i];
    ShaRegs r{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
    sha256_rounds_folded<0, kEnd>(r, w);
    finish(r);
  }
  {
#pragma unroll
    for (int i = 0; i < 5; i++) w[i] = kParNodeWords[32 + i];
    w[5] = kParNodeWords[37] | (dr[0] >> 8);
#pragma unroll
    for (int i = 6; i < 13; i++) w[i] = __builtin_amdgcn_alignbit(dr[i - 6], dr[i - 5], 8);
    w[13] = kParNodeWords[45] | (dr[7] << 24);
    w[14] = kParNodeWords[46];
    w[15] = kParNodeWords[47];
    ShaRegs r{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
    sha256_rounds_folded<0, kEnd>(r, w);
    finish(r);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[i];
}

// The 96-byte record of a parity node from its digest: 0xFF*58 || digest bytes.
__device__ __forceinline__ void parity_record(const uint32_t (&d)[8], uint32_t (&nd)[kNodeWords]) {
#pragma unroll
  for (int i = 0; i < 14; i++) nd[i] = 0xFFFFFFFFu;
  nd[14] = 0xFFFFu;
  put_digest(nd, d);
}

__device__ __forceinline__ void load_digest(const uint32_t* p, uint32_t (&d)[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

__device__ __forceinline__ void store_digest(uint32_t* p, const uint32_t (&d)[8]) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(d[0], d[1], d[2], d[3]);
  q[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

// ------------------------------------------------------------------ RFC-6962

// SHA256 of the empty string (RFC-6962 empty tree).
__device__ __forceinline__ void sha_empty(uint32_t (&st)[8]) {
  uint32_t w[16];
  w[0] = 0x80000000u;
#pragma unroll
  for (int i = 1; i < 16; i++) w[i] = 0;
  sha256_init(st);
  sha256_compress(st, w);
}

// leafHash = SHA256(0x00 || item) for a 90-byte item (2 blocks).
__device__ __forceinline__ void rfc_leaf90(const uint32_t (&R)[kNodeWords], uint32_t (&st)[8]) {
  sha256_init(st);
#pragma unroll
  for (int b = 0; b < 2; b++) {
    uint32_t w[16];
#pragma unroll
    for (int wi = 0; wi < 16; wi++) {
      const int q = 16 * b + wi;
      uint32_t x;
      if (q == 0) x = perm(0u, R[0], 0x0C000102u);
      else if (q <= 21) x = perm(R[q - 1], R[q], 0x07000102u);
      else if (q == 22) x = perm(R[21], R[22], 0x0700010Cu) | 0x80u;
      else if (q == 31) x = 91u * 8u;
      else x = 0u;
      w[wi] = x;
    }
    sha256_compress(st, w);
  }
}

// innerHash = SHA256(0x01 || l(32) || r(32)) (2 blocks). The DAH tree hashes its levels
// one after the other in one workgroup (a latency chain), so both compressions are
// unrolled; the second block's 15 constant words fold into its schedule.
__device__ __forceinline__ void rfc_inner(const uint32_t* l, const uint32_t* r, uint32_t (&st)[8]) {
  uint32_t w[16];
  w[0] = 0x01000000u | (l[0] >> 8);
#pragma unroll
  for (int i = 1; i < 8; i++) w[i] = __builtin_amdgcn_alignbit(l[i - 1], l[i], 8);
  w[8] = __builtin_amdgcn_alignbit(l[7], r[0], 8);
#pragma unroll
  for (int i = 9; i < 16; i++) w[i] = __builtin_amdgcn_alignbit(r[i - 9], r[i - 8], 8);
  sha256_init(st);
  uint32_t w2[16];
  w2[0] = (r[7] << 24) | 0x00800000u;
#pragma unroll
  for (int i = 1; i < 15; i++) w2[i] = 0;
  w2[15] = 65u * 8u;
  sha256_compress(st, w);
  sha256_compress(st, w2);
}

}  // namespace cel
