// Blob share commitments (go-square v1.1.0 inclusion.CreateCommitment) for a batch of blobs
// on gfx950, from the raw blob bytes: the shares are never written out (except by the leaf
// stage's A/B partner, k_blob_expand, a measurement aid).
//
//   commitment = merkle.HashFromByteSlices(subtree roots)
//   subtree roots = NMT roots over the merkle mountain range of the blob's shares at
//                   SubTreeWidth(n, threshold) (blob_plan.hpp has the slot layout)
//
//   k_blob_tile   one workgroup per 256 leaf slots: each lane hashes its share's leaf
//                 (9 compressions) straight from the blob bytes, then the workgroup reduces
//                 levels 1..8 in place in LDS (24 KiB of node records) and writes every
//                 subtree root of <= 256 leaves into the blob's slot of the roots array.
//   k_blob_top_*  subtree widths 512 and 1024: levels 9 and 10 over the tiles' level-8
//                 nodes, then their roots.
//   k_blob_commit one workgroup per blob: RFC-6962 over its roots. Bottom-up pairing in
//                 which an unpaired last node moves up unchanged gives the same root as
//                 the recursive split at the largest power of two below the count.
//
// Bounds: a lane reads only dwords that hold at least one byte of its own blob (clamped
// index, bytes past the blob masked to the share's zero padding), slot tables hold
// `slots` entries (a multiple of 256 = the grid), roots go to root0 + index < roots.
#include <hip/hip_runtime.h>

#include "blob_plan.hpp"
#include "cel_internal.hpp"
#include "nmt_device.hpp"
#include "sha256_device.hpp"

namespace cel {

using blob::kNoBlob;
using blob::Rec;

namespace {

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-byte load

// Leaf node ns || ns || SHA256(0x00 || ns || share j) of a blob whose data starts at `data`
// (any byte alignment), share version 0.
//
// Share j is ns || info || [len, j = 0] || data slice || zeros, so in the 542-byte leaf
// message 0x00 || ns || share the data always starts on a message word: byte 64 for
// share 0 (after the 4-byte sequence length) and byte 60 for the others. With P the blob
// offset that message byte 60 maps to (-4 for share 0, 478 + 482 (j - 1) otherwise),
// message word m >= 15 is the big-endian read of blob bytes P + 4 (m - 15) .. + 3: one
// v_perm_b32 over two neighbouring dwords with a per-lane selector for the address's
// alignment a = (data + P) mod 4. `vend` counts the bytes from P that belong to the blob;
// what lies beyond is the share's zero padding.
__device__ __forceinline__ void blob_leaf_node(const uint32_t (&ns)[8], const uint8_t* __restrict__ data, uint32_t len,
                                               uint32_t j, uint32_t (&nd)[kNodeWords]) {
  const int64_t P = j == 0 ? -4 : (int64_t)blob::kSparseFirst + (int64_t)blob::kSparseCont * (j - 1);
  const uint32_t left = j == 0 ? len : len - (uint32_t)P;
  const int32_t vend = j == 0 ? 4 + (int32_t)(left < blob::kSparseFirst ? left : blob::kSparseFirst)
                              : (int32_t)(left < blob::kSparseCont ? left : blob::kSparseCont);
  const uintptr_t pa = (uintptr_t)data + (uintptr_t)P;
  const uint32_t a = (uint32_t)pa & 3u;
  const uint32_t* __restrict__ Q = reinterpret_cast<const uint32_t*>(pa - a);
  const uint32_t sel = 0x00010203u + a * 0x01010101u;
  const int32_t imax = (vend + (int32_t)a - 1) >> 2;  // last dword of Q that holds a blob byte
  // dword i of Q, clamped into the blob; share 0 never reads dword 0 (the length's place)
  auto ld = [&](int32_t i) { return Q[i < imax ? i : imax]; };
  // message word 15 + i from dwords i, i + 1, bytes past the blob zeroed
  auto word = [&](uint32_t lo, uint32_t hi, int32_t i) {
    const int32_t v = vend - 4 * i;  // blob bytes in this word
    const uint32_t x = perm(hi, lo, sel);
    return v >= 4 ? x : (v <= 0 ? 0u : x & (0xFFFFFFFFu << (32 - 8 * v)));
  };

  uint32_t st[8], w[16], nx[17];
  sha256_init(st);
  {  // block 0: 0x00 || ns || ns || info || first data word (or the sequence length)
    const uint32_t s7 = (ns[7] & 0xFFu) | (j == 0 ? 0x100u : 0u);  // share bytes 28..29: ns[28], info
    w[0] = perm(0u, ns[0], 0x0C000102u);
#pragma unroll
    for (int i = 1; i < 7; i++) w[i] = perm(ns[i - 1], ns[i], 0x07000102u);
    w[7] = perm(ns[6], ns[7], 0x07000C0Cu) | perm(0u, ns[0], 0x0C0C0001u);
#pragma unroll
    for (int i = 8; i < 15; i++) w[i] = perm(ns[i - 8], i == 14 ? s7 : ns[i - 7], 0x06070001u);
    if (j == 0) {
      w[15] = len;
    } else {
      const uint32_t d0 = ld(0), d1 = ld(1);
      w[15] = word(d0, d1, 0);
    }
    sha256_compress(st, w);
  }
#pragma unroll 1
  for (int b = 1; b < 8; b++) {  // blocks 1..7: message words 16b .. 16b + 15 = dwords 16b - 15 .. 16b + 1
    const int32_t i0 = 16 * b - 15;
    if (__all(64 * b + 8 <= vend)) {  // the whole wave is inside its blobs: plain loads, no masks
      const uint32_t* base = Q + i0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u32x4u v = *reinterpret_cast<const u32x4u*>(base + 4 * i);
        nx[4 * i] = v.x; nx[4 * i + 1] = v.y; nx[4 * i + 2] = v.z; nx[4 * i + 3] = v.w;
      }
      nx[16] = base[16];
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = perm(nx[i + 1], nx[i], sel);
    } else {
#pragma unroll
      for (int i = 0; i < 17; i++) nx[i] = ld(i0 + i);
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = word(nx[i], nx[i + 1], i0 + i);
    }
    sha256_compress(st, w);
  }
  {  // block 8: message words 128..135 (the last holds two share bytes), 0x80, zeros, length
#pragma unroll
    for (int i = 0; i < 9; i++) nx[i] = ld(113 + i);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = word(nx[i], nx[i + 1], 113 + i);
    w[7] = (w[7] & 0xFFFF0000u) | 0x00008000u;
#pragma unroll
    for (int i = 8; i < 15; i++) w[i] = 0u;
    w[15] = 542u * 8u;
    sha256_compress(st, w);
  }
#pragma unroll
  for (int i = 0; i < 7; i++) nd[i] = ns[i];
  nd[7] = (ns[7] & 0xFFu) | (ns[0] << 8);
#pragma unroll
  for (int i = 0; i < 6; i++) nd[8 + i] = __builtin_amdgcn_alignbyte(ns[i + 1], ns[i], 3);
  nd[14] = (ns[6] >> 24) | ((ns[7] & 0xFFu) << 8);
  put_digest(nd, st);
}

__device__ __forceinline__ void load_ns(const Rec* __restrict__ r, uint32_t (&ns)[8]) {
  const uint4* p = reinterpret_cast<const uint4*>(r->ns);
  const uint4 v0 = p[0], v1 = p[1];
  ns[0] = v0.x; ns[1] = v0.y; ns[2] = v0.z; ns[3] = v0.w; ns[4] = v1.x; ns[5] = v1.y; ns[6] = v1.z; ns[7] = v1.w;
}

// The A/B partner of the direct read (profiles/commitments_leaf_ab.txt): every share written
// out to device memory, [slot][512], one lane per share dword (bytes gathered one by one;
// gap slots are left alone, no lane reads them), then k_blob_tile<true> hashes the shares with
// the EDS commit's leaf_hash.
__global__ __launch_bounds__(256) void k_blob_expand(const uint8_t* __restrict__ data, const Rec* __restrict__ recs,
                                                     const uint32_t* __restrict__ slot_blob, uint32_t* __restrict__ shares) {
  const uint32_t slot = blockIdx.x * 2u + (threadIdx.x >> 7), d = threadIdx.x & 127u;
  const uint32_t b = slot_blob[slot];
  if (b == kNoBlob) return;
  const Rec* r = recs + b;
  const uint32_t j = slot - r->first, len = r->len;
  const uint8_t* __restrict__ src = data + r->off;
  const uint8_t* __restrict__ ns = reinterpret_cast<const uint8_t*>(r->ns);
  uint32_t v = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t p = 4 * d + q;  // byte of the share
    uint32_t x;
    if (p < kNs) {
      x = ns[p];
    } else if (p == kNs) {
      x = j == 0;
    } else if (j == 0 && p < kNs + 5) {
      x = (len >> (8 * (kNs + 4 - p))) & 0xFFu;
    } else {
      const uint64_t at = j == 0 ? p - (kNs + 5) : (uint64_t)blob::kSparseFirst + (uint64_t)blob::kSparseCont * (j - 1) + (p - (kNs + 1));
      x = at < len ? src[at] : 0u;
    }
    v |= x << (8 * q);
  }
  shares[(uint64_t)slot * (kShare / 4) + d] = v;
}

// grid: slots / 256 workgroups of 256. roots: [total roots][24]; tops: [tiles][24], the
// tile's level-8 node for blobs wider than 256. EXPANDED: leaves from shares ([slot][512],
// k_blob_expand) instead of the blob bytes.
template <bool EXPANDED>
__global__ __launch_bounds__(256) void k_blob_tile(const uint8_t* __restrict__ data, const Rec* __restrict__ recs,
                                                   const uint32_t* __restrict__ slot_blob, uint32_t* __restrict__ roots,
                                                   uint32_t* __restrict__ tops, const uint32_t* __restrict__ shares) {
  __shared__ __attribute__((aligned(16))) uint32_t nodes[256 * kNodeWords];
  __shared__ uint32_t meta[256];  // shares from this slot to the blob's end | wlog << 24; 0 = empty slot
  __shared__ uint32_t top_level;  // highest level any blob of the tile needs here
  const uint32_t tid = threadIdx.x;
  const uint32_t slot = blockIdx.x * 256u + tid;
  const uint32_t b = slot_blob[slot];
  if (tid == 0) top_level = 0;
  __syncthreads();
  uint32_t n = 0, s = 0, wlog = 0, root0 = 0;
  if (b != kNoBlob) {
    const Rec* r = recs + b;
    n = r->n; wlog = r->wlog; root0 = r->root0;
    s = slot - r->first;
    uint32_t nd[kNodeWords];
    if (EXPANDED) {
      make_leaf_node<false>(shares + (uint64_t)slot * (kShare / 4), true, nd);
    } else {
      uint32_t ns[8];
      load_ns(r, ns);
      blob_leaf_node(ns, data + r->off, r->len, s, nd);
    }
    store_node(nodes + tid * kNodeWords, nd);
    meta[tid] = (n - s) | (wlog << 24);
    if (wlog) atomicMax(&top_level, wlog < 8 ? wlog : 8u);
  } else {
    meta[tid] = 0;
  }
  __syncthreads();
  const uint32_t levels = top_level;
  // Level L node at tile slot t = lane << L from the two level L - 1 nodes at t and
  // t + 2^(L-1), in place: no other lane of the level touches either record.
  for (uint32_t L = 1; L <= levels; L++) {
    if (tid < (256u >> L)) {
      const uint32_t t = tid << L, m = meta[t];
      if ((m >> 24) >= L && (m & 0xFFFFFFu) >= (1u << L)) {
        uint32_t o[kNodeWords];
        hash_pair(nodes, t, t + (1u << (L - 1)), o);
        store_node(nodes + t * kNodeWords, o);
      }
    }
    __syncthreads();
  }
  if (b == kNoBlob) return;
  uint32_t index, level;
  if (blob::root_at(n, wlog, s, &index, &level) && level <= 8) {
    const uint4* src = reinterpret_cast<const uint4*>(nodes + tid * kNodeWords);
    uint4* dst = reinterpret_cast<uint4*>(roots + (uint64_t)(root0 + index) * kNodeWords);
#pragma unroll
    for (int i = 0; i < 6; i++) dst[i] = src[i];
  }
  if (tid == 0 && wlog > 8 && n - s >= 256) {
    const uint4* src = reinterpret_cast<const uint4*>(nodes);
    uint4* dst = reinterpret_cast<uint4*>(tops + (uint64_t)blockIdx.x * kNodeWords);
#pragma unroll
    for (int i = 0; i < 6; i++) dst[i] = src[i];
  }
}

// Level L = 9 or 10 over the tiles' level-8 nodes, in place: lane g owns tile g << (L - 8).
__global__ __launch_bounds__(256) void k_blob_top_level(const Rec* __restrict__ recs, const uint32_t* __restrict__ slot_blob,
                                                        uint32_t* __restrict__ tops, uint32_t tiles, uint32_t L) {
  const uint64_t tile = (uint64_t)(blockIdx.x * 256u + threadIdx.x) << (L - 8);
  if (tile >= tiles) return;
  const uint32_t slot = (uint32_t)tile * 256u;
  const uint32_t b = slot_blob[slot];
  if (b == kNoBlob) return;
  const Rec* r = recs + b;
  if (r->wlog < L || r->n - (slot - r->first) < (1u << L)) return;
  uint32_t o[kNodeWords];
  hash_pair(tops, tile, tile + (1u << (L - 9)), o);
  store_node(tops + tile * kNodeWords, o);
}

// Roots of more than 256 leaves, one lane per tile.
__global__ __launch_bounds__(256) void k_blob_top_roots(const Rec* __restrict__ recs, const uint32_t* __restrict__ slot_blob,
                                                        const uint32_t* __restrict__ tops, uint32_t* __restrict__ roots,
                                                        uint32_t tiles) {
  const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
  if (tile >= tiles) return;
  const uint32_t slot = tile * 256u;
  const uint32_t b = slot_blob[slot];
  if (b == kNoBlob) return;
  const Rec* r = recs + b;
  uint32_t index, level;
  if (r->wlog <= 8 || !blob::root_at(r->n, r->wlog, slot - r->first, &index, &level) || level <= 8) return;
  const uint4* src = reinterpret_cast<const uint4*>(tops + (uint64_t)tile * kNodeWords);
  uint4* dst = reinterpret_cast<uint4*>(roots + (uint64_t)(r->root0 + index) * kNodeWords);
#pragma unroll
  for (int i = 0; i < 6; i++) dst[i] = src[i];
}

constexpr uint32_t kCommitLds = 1024;  // digests one workgroup reduces in LDS

// One workgroup per blob: RFC-6962 over its roots. da / db: [total roots][8] scratch, used
// only by blobs with more than kCommitLds roots (levels ping-pong between them in global
// memory until the rest fits LDS).
__global__ __launch_bounds__(256) void k_blob_commit(const Rec* __restrict__ recs, const uint32_t* __restrict__ roots,
                                                     uint32_t* da, uint32_t* db, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t hs[kCommitLds * 8];
  const Rec* r = recs + blockIdx.x;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  uint32_t cnt = r->nroots;
  const uint64_t r0 = r->root0;
  const bool big = cnt > kCommitLds;
  uint32_t* in = da + r0 * 8;
  uint32_t* nxt = db + r0 * 8;
  for (uint32_t i = tid; i < cnt; i += nt) {
    uint32_t R[kNodeWords], st[8];
    load_node(roots + (r0 + i) * kNodeWords, R);
    rfc_leaf90(R, st);
    uint32_t* d = big ? in + (uint64_t)i * 8 : hs + i * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) d[q] = st[q];
  }
  __syncthreads();
  while (cnt > kCommitLds) {  // out[j] = H(in[2j], in[2j+1]), or in[2j] moved up if unpaired
    const uint32_t half = (cnt + 1) / 2;
    for (uint32_t jn = tid; jn < half; jn += nt) {
      uint32_t st[8];
      if (2 * jn + 1 < cnt) {
        rfc_inner(in + (uint64_t)(2 * jn) * 8, in + (uint64_t)(2 * jn + 1) * 8, st);
      } else {
#pragma unroll
        for (int q = 0; q < 8; q++) st[q] = in[(uint64_t)(2 * jn) * 8 + q];
      }
#pragma unroll
      for (int q = 0; q < 8; q++) nxt[(uint64_t)jn * 8 + q] = st[q];
    }
    __threadfence_block();
    __syncthreads();
    uint32_t* t = in; in = nxt; nxt = t;
    cnt = half;
  }
  if (big) {
    for (uint32_t i = tid; i < cnt * 8; i += nt) hs[i] = in[i];
    __syncthreads();
  }
  while (cnt > 1) {
    const uint32_t half = cnt / 2;
    for (uint32_t base = 0; base < half; base += nt) {
      const uint32_t i = base + tid;
      uint32_t st[8];
      if (i < half) rfc_inner(hs + (2 * i) * 8, hs + (2 * i + 1) * 8, st);
      __syncthreads();
      if (i < half) {
#pragma unroll
        for (int q = 0; q < 8; q++) hs[i * 8 + q] = st[q];
      }
      __syncthreads();
    }
    if (cnt & 1) {
      if (tid < 8) hs[half * 8 + tid] = hs[(cnt - 1) * 8 + tid];
      __syncthreads();
    }
    cnt = half + (cnt & 1);
  }
  if (tid < 8) {
    const uint32_t v = hs[tid];
    uint8_t* o = out + (uint64_t)blockIdx.x * 32 + 4 * tid;
    o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v;
  }
}

// Workspace: the plan's tables (nblobs records | slot table [slots], uploaded by the caller) |
//            tile tops [slots / 256] nodes | roots [roots] nodes | da, db [roots][8]
struct BlobWork {
  const Rec* recs;
  const uint32_t* slot_blob;
  uint32_t *tops, *roots, *da, *db;
  size_t size;
};
BlobWork blob_work(void* work, uint64_t slots, uint64_t roots, uint32_t nblobs) {
  Carver c(work);
  BlobWork w;
  w.recs = c.take<const Rec>((size_t)nblobs * sizeof(Rec));
  w.slot_blob = c.take<const uint32_t>(slots * 4);
  w.tops = c.take<uint32_t>(slots / 256 * kNodeWords * 4);
  w.roots = c.take<uint32_t>(roots * kNodeWords * 4);
  w.da = c.take<uint32_t>(roots * 32);
  w.db = c.take<uint32_t>(roots * 32);
  w.size = c.size();
  return w;
}

}  // namespace

size_t blob_commit_workspace_size(uint64_t slots, uint64_t roots, uint32_t nblobs) {
  return blob_work(nullptr, slots, roots, nblobs).size;
}

// tables: nblobs records then, 256-aligned, the slot table (plan.slots entries), already
// in the workspace's first bytes. d_shares != nullptr (plan.slots * 512 bytes) selects the
// expanded-shares leaf stage. Asynchronous on s.
hipError_t launch_blob_commit(const uint8_t* d_data, const blob::Plan& plan, void* d_work, uint8_t* d_out,
                              hipStream_t s, uint32_t* d_shares) {
  const uint32_t nblobs = (uint32_t)plan.recs.size();
  const uint32_t tiles = (uint32_t)(plan.slots / 256);
  const BlobWork w = blob_work(d_work, plan.slots, plan.roots, nblobs);
  if (d_shares) {
    k_blob_expand<<<tiles * 128, 256, 0, s>>>(d_data, w.recs, w.slot_blob, d_shares);
    k_blob_tile<true><<<tiles, 256, 0, s>>>(d_data, w.recs, w.slot_blob, w.roots, w.tops, d_shares);
  } else {
    k_blob_tile<false><<<tiles, 256, 0, s>>>(d_data, w.recs, w.slot_blob, w.roots, w.tops, nullptr);
  }
  for (uint32_t L = 9; L <= plan.max_wlog; L++) {
    const uint32_t lanes = (tiles + (1u << (L - 8)) - 1) >> (L - 8);
    k_blob_top_level<<<(lanes + 255) / 256, 256, 0, s>>>(w.recs, w.slot_blob, w.tops, tiles, L);
  }
  if (plan.max_wlog > 8)
    k_blob_top_roots<<<(tiles + 255) / 256, 256, 0, s>>>(w.recs, w.slot_blob, w.tops, w.roots, tiles);
  // one lane per pair of the widest RFC level where that keeps a wave busy
  const uint32_t block = plan.max_roots <= 128 ? 64u : 256u;
  k_blob_commit<<<nblobs, block, 0, s>>>(w.recs, w.roots, w.da, w.db, d_out);
  return hipGetLastError();
}

}  // namespace cel
