// Blobs out of a resident square (blob_parse.hpp): go-square v1.1.0 parseSparseShares over runs
// of ODS shares, and the blobs' bytes gathered into the layout launch_blob_commit takes. The
// inverse of square_build.hip; it replaces a download of the shares, a parse on the host and an
// upload of the bytes. The scheme is nmt_namespace.hip's: classify, block sums, one workgroup's
// scan, the same blocks again, emit. Every position is a place in a prefix sum, so the results
// do not depend on any schedule.
//
// k_bp_classify  one lane per share of the ranges (flat position p): the 34-byte head of its
//                cell gives the class (padding / start / continuation / bad version) and the
//                declared length.
// k_bp_sums      the three counters (significant shares, starts, bad versions) of each block of
//                256 positions
// k_bp_scan      one workgroup: the exclusive prefix sum of the block sums in place, the totals
// k_bp_compact   the same blocks again: every position's exclusive prefix (pre), the significant
//                shares compacted into the source list (src), the starts into the candidates
//                (cand). Blob b's j-th share is src[first[b] + j], padding in between or not.
// k_bp_cand      one lane per candidate: the shares it found (up to the next start or the end
//                of its range); a candidate that lacks bytes flags its range. The flag is a
//                plain store of 1 into a word cleared before: the lanes that race store the same
//                value, and nothing is ordered by it.
// k_bp_status    one lane per range: its status, bparse::walk_status and the flag.
// k_bp_bsums, k_bp_bscan, k_bp_bcompact  the same scan over the candidates: those of ranges
//                without an error are the blobs; a blob's data offset is the prefix sum of the
//                lengths before it, each rounded up to 16. The records, the head.
// k_bp_gather    destination-driven, the mirror image of k_square_build: a lane owns one
//                16-byte chunk of one blob's output and stores it with one aligned 16-byte
//                store. Its bytes come from one or two shares (the boundary is at blob byte
//                478 + 482 m), each read as five aligned dwords and funnelled with
//                v_alignbyte_b32; the misalignment is constant within a share. Bytes past the
//                blob's length are stored as zero.
//
// Bounds. The host has checked k, the ranges (start <= end <= k * k, fewer than 2^31 shares in
// all: api_blobs.cpp, bparse::ranges_error) and carved the workspace for `total` positions and
// n_ranges ranges (bparse::carve); roff and rstart are the host's. What the cells hold decides
// classes and lengths only, never an address:
//   k_bp_classify  p < total; share = rstart[r] + p - roff[r] < ends[r] <= k * k, so the cell
//                  (share / k, share % k) lies in Q0 and the 36 bytes read lie in it. Writes
//                  cls[p].
//   k_bp_sums, k_bp_scan, k_bp_compact  read cls[p], p < total. The prefix counts are counts of
//                  positions, so sig, starts, bad <= total: src[sig], cand[starts] stay below
//                  total entries, pre has total + 1.
//   k_bp_cand      c < n_cand <= total (the device's count). cand[c + 1] is read only when
//                  c + 1 is below the starts counted up to the range's end, so it is a
//                  candidate. found = a difference of places in src of one range: at most the
//                  range's shares, at most 2^18. A declared length of 0xFFFFFFFF only makes
//                  is_short true (64-bit arithmetic). Writes cand[c].found, range_short[r],
//                  r < n_ranges.
//   k_bp_status    r < n_ranges; src[pre[roff[r]].sig] is read only when the range has a
//                  significant share, which is then that entry.
//   k_bp_b*        c < n_cand. A blob's place is below the number of candidates; doff has
//                  total + 1 entries. The namespace is read from the start share's cell,
//                  an ODS index below k * k that k_bp_compact copied from cls.
//   k_bp_gather    chunk i < doff[nb] / 16 with nb = min(n_blobs passed, head->n_blobs); its
//                  blob b < nb by search over doff[0 .. nb]. o = 16 i - doff[b] < pad16(len).
//                  A blob is a candidate that is not short: found >= the shares its length
//                  needs, so share j of a byte below len has j < found, and src[first + j] is
//                  one of the range's significant shares: an ODS index below k * k, masked to
//                  18 bits besides. Of that cell the dwords (q >> 2) + 0 .. 4 are read, each
//                  only if its index is at most 127: inside the cell. The store covers
//                  [doff[b] + o, + 16) with o + 16 <= pad16(len): inside the blob's own padded
//                  span, below head->total_bytes, which the plan call has given the caller to
//                  size d_data with. Nothing runs when head->k is not the k passed.
// Continuation-only ranges have no candidate; overlapping ranges are separate positions.
#include <hip/hip_runtime.h>

#include "blob_parse.hpp"
#include "cel_internal.hpp"
#include "scan_device.hpp"

namespace cel {

using bparse::BlobSums;
using bparse::Cand;
using bparse::Class;
using bparse::Head;
using bparse::Pre;
using bparse::Work;
using scan::block_scan;
using scan::cell_of;
using scan::kWaves;
using scan::log2_of;
using scan::scan_blocks;

namespace {

__global__ __launch_bounds__(256) void k_bp_classify(const uint8_t* __restrict__ eds, uint32_t klog,
                                                     const uint32_t* __restrict__ roff,
                                                     const uint32_t* __restrict__ rstart, uint32_t n_ranges,
                                                     uint32_t total, Class* __restrict__ cls) {
  const uint32_t p = blockIdx.x * bparse::kScanBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t r = bparse::range_of(roff, n_ranges, p);
  const uint32_t share = rstart[r] + (p - roff[r]);
  const uint4* cell = cell_of(eds, klog, share);
  const uint4 a = cell[0], b = cell[1];
  const uint32_t c = reinterpret_cast<const uint32_t*>(cell)[8];
  const uint32_t info = (b.w >> 8) & 0xFFu;
  const uint32_t len = (((b.w >> 16) & 0xFFu) << 24) | ((b.w >> 24) << 16) | ((c & 0xFFu) << 8) | ((c >> 8) & 0xFFu);
  const uint32_t all = a.x & a.y & a.z & a.w & b.x & b.y & b.z, any = a.x | a.y | a.z | a.w | b.x | b.y | b.z;
  const bool tail = all == 0xFFFFFFFFu && (b.w & 0xFFu) == 0xFEu;
  const bool reserved = any == 0u && (b.w & 0xFFu) == 0xFFu;
  cls[p] = Class{bparse::classify(info, tail, reserved, len), len, share, r};
}

// The counters of position p; zero beyond the ranges.
__device__ __forceinline__ Class share_counts(const Class* __restrict__ cls, uint32_t p, uint32_t total,
                                              uint32_t (&v)[3]) {
  Class c{bparse::kPad, 0, 0, 0};
  if (p < total) c = cls[p];
  v[0] = c.cls != bparse::kPad ? 1u : 0u;
  v[1] = c.cls == bparse::kStart ? 1u : 0u;
  v[2] = c.cls == bparse::kBadVer ? 1u : 0u;
  return c;
}

__global__ __launch_bounds__(256) void k_bp_sums(const Class* __restrict__ cls, uint32_t total,
                                                 uint32_t* __restrict__ sums1) {
  __shared__ uint32_t sh[kWaves * 3];
  uint32_t v[3], tot[3];
  share_counts(cls, blockIdx.x * bparse::kScanBlock + threadIdx.x, total, v);
  block_scan<uint32_t, 3>(v, tot, sh);
  if (threadIdx.x == 0) {
    sums1[blockIdx.x * 3] = tot[0];
    sums1[blockIdx.x * 3 + 1] = tot[1];
    sums1[blockIdx.x * 3 + 2] = tot[2];
  }
}

__global__ __launch_bounds__(256) void k_bp_scan(uint32_t* __restrict__ sums1, uint64_t blocks, uint32_t total,
                                                 uint32_t k, uint32_t n_ranges, Pre* __restrict__ pre,
                                                 Head* __restrict__ head) {
  __shared__ uint32_t part[257 * 3];
  uint32_t tot[3];
  scan_blocks<uint32_t, 3>(sums1, blocks, tot, part);
  if (threadIdx.x == 0) {
    pre[total] = Pre{tot[0], tot[1], tot[2]};
    head->n_sig = tot[0];
    head->n_cand = tot[1];
    head->total = total;
    head->k = k;
    head->n_ranges = n_ranges;
  }
}

__global__ __launch_bounds__(256) void k_bp_compact(const Class* __restrict__ cls, uint32_t total,
                                                    const uint32_t* __restrict__ sums1, Pre* __restrict__ pre,
                                                    uint32_t* __restrict__ src, Cand* __restrict__ cand) {
  __shared__ uint32_t sh[kWaves * 3];
  const uint32_t p = blockIdx.x * bparse::kScanBlock + threadIdx.x;
  uint32_t v[3], tot[3];
  const Class c = share_counts(cls, p, total, v);
  const uint32_t mine[3] = {v[0], v[1], v[2]};
  block_scan<uint32_t, 3>(v, tot, sh);
  if (p >= total) return;
  const uint32_t g = sums1[blockIdx.x * 3] + (v[0] - mine[0]);
  const uint32_t s = sums1[blockIdx.x * 3 + 1] + (v[1] - mine[1]);
  pre[p] = Pre{g, s, sums1[blockIdx.x * 3 + 2] + (v[2] - mine[2])};
  if (mine[0]) src[g] = c.share | (c.cls << bparse::kClassShift);  // g < the significant shares <= total
  if (mine[1]) cand[s] = Cand{c.range, c.share, g, c.len, 0, 0};   // s < the starts <= total
}

__global__ __launch_bounds__(256) void k_bp_cand(const Head* __restrict__ head, const uint32_t* __restrict__ roff,
                                                 const Pre* __restrict__ pre, Cand* __restrict__ cand,
                                                 uint32_t* __restrict__ range_short) {
  const uint32_t c = blockIdx.x * bparse::kScanBlock + threadIdx.x;
  if (c >= head->n_cand) return;
  const Cand cd = cand[c];
  const Pre end = pre[roff[cd.range + 1]];  // the counts up to the range's end
  const uint32_t next = c + 1 < end.starts ? cand[c + 1].g : end.sig;
  const uint32_t found = next - cd.g;
  cand[c].found = found;
  if (bparse::is_short(cd.len, found)) range_short[cd.range] = 1u;
}

__global__ __launch_bounds__(256) void k_bp_status(const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                                   const Pre* __restrict__ pre, const uint32_t* __restrict__ src,
                                                   const uint32_t* __restrict__ range_short,
                                                   uint32_t* __restrict__ range_status) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_ranges) return;
  const Pre a = pre[roff[r]], b = pre[roff[r + 1]];
  const uint32_t nsig = b.sig - a.sig;
  const uint32_t first = nsig ? src[a.sig] >> bparse::kClassShift : bparse::kPad;
  uint32_t st = bparse::walk_status(nsig, first, b.bad - a.bad);
  if (st == bparse::kOk && range_short[r]) st = bparse::kEShort;
  range_status[r] = st;
}

// The counters of candidate c; zero beyond the candidates and for one whose range failed.
__device__ __forceinline__ Cand cand_counts(const Cand* __restrict__ cand, uint32_t c, uint64_t n_cand,
                                            const uint32_t* __restrict__ range_status, uint64_t (&v)[3]) {
  Cand cd{0, 0, 0, 0, 0, 0};
  bool is_blob = false;
  if (c < n_cand) {
    cd = cand[c];
    is_blob = range_status[cd.range] == bparse::kOk;
  }
  v[0] = is_blob ? 1u : 0u;
  v[1] = is_blob ? bparse::pad16(cd.len) : 0u;
  v[2] = is_blob ? cd.found : 0u;
  return cd;
}

__global__ __launch_bounds__(256) void k_bp_bsums(const Head* __restrict__ head, const Cand* __restrict__ cand,
                                                  const uint32_t* __restrict__ range_status,
                                                  uint64_t* __restrict__ sums2) {
  __shared__ uint64_t sh[kWaves * 3];
  uint64_t v[3], tot[3];
  cand_counts(cand, blockIdx.x * bparse::kScanBlock + threadIdx.x, head->n_cand, range_status, v);
  block_scan<uint64_t, 3>(v, tot, sh);
  if (threadIdx.x == 0) {
    sums2[blockIdx.x * 3] = tot[0];
    sums2[blockIdx.x * 3 + 1] = tot[1];
    sums2[blockIdx.x * 3 + 2] = tot[2];
  }
}

__global__ __launch_bounds__(256) void k_bp_bscan(uint64_t* __restrict__ sums2, uint64_t blocks,
                                                  uint64_t* __restrict__ doff, Head* __restrict__ head) {
  __shared__ uint64_t part[257 * 3];
  uint64_t tot[3];
  scan_blocks<uint64_t, 3>(sums2, blocks, tot, part);
  if (threadIdx.x == 0) {
    head->n_blobs = tot[0];
    head->total_bytes = tot[1];
    head->total_shares = tot[2];
    doff[tot[0]] = tot[1];  // tot[0] <= the candidates <= total: doff has total + 1 entries
  }
}

__global__ __launch_bounds__(256) void k_bp_bcompact(const uint8_t* __restrict__ eds, uint32_t klog,
                                                     const Head* __restrict__ head, const Cand* __restrict__ cand,
                                                     const uint32_t* __restrict__ range_status,
                                                     const uint64_t* __restrict__ sums2,
                                                     cel_blob_rec* __restrict__ recs, uint64_t* __restrict__ doff,
                                                     uint32_t* __restrict__ first) {
  __shared__ uint64_t sh[kWaves * 3];
  uint64_t v[3], tot[3];
  const Cand cd = cand_counts(cand, blockIdx.x * bparse::kScanBlock + threadIdx.x, head->n_cand, range_status, v);
  const uint64_t is_blob = v[0], bytes = v[1];
  block_scan<uint64_t, 3>(v, tot, sh);
  if (!is_blob) return;
  const uint64_t b = sums2[blockIdx.x * 3] + (v[0] - 1);  // below the blobs <= the candidates <= total
  const uint64_t off = sums2[blockIdx.x * 3 + 1] + (v[1] - bytes);
  const uint4* cell = cell_of(eds, klog, cd.share & bparse::kShareMask);
  const uint4 n0 = cell[0];
  uint4 n1 = cell[1];
  n1.w &= 0xFFu;  // 29 namespace bytes, then zeros
  uint4* out = reinterpret_cast<uint4*>(recs + b);
  out[0] = make_uint4(cd.range, cd.share, cd.found, 0u);
  out[1] = make_uint4(cd.len, 0u, (uint32_t)off, (uint32_t)(off >> 32));
  out[2] = n0;
  out[3] = n1;
  doff[b] = off;
  first[b] = cd.g;
}

// Mask of the bytes t of the dword at chunk byte at with lo <= at + t < hi.
__device__ __forceinline__ uint32_t byte_mask(uint32_t at, uint32_t lo, uint32_t hi) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t t = 0; t < 4; t++)
    if (at + t >= lo && at + t < hi) m |= 0xFFu << (8u * t);
  return m;
}

// The chunk bytes [pc.lo, pc.hi) out of one cell, or'ed into d.
__device__ __forceinline__ void take_piece(const uint32_t* __restrict__ cell, const bparse::Piece& pc, uint32_t (&d)[4]) {
  if (pc.lo >= pc.hi) return;
  const uint32_t w0 = pc.q >> 2, a = pc.q & 3u;
  uint32_t x[5];
#pragma unroll
  for (uint32_t i = 0; i < 5; i++) x[i] = w0 + i <= 127u ? cell[w0 + i] : 0u;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) d[i] |= __builtin_amdgcn_alignbyte(x[i + 1], x[i], a) & byte_mask(4u * i, pc.lo, pc.hi);
}

__global__ __launch_bounds__(256) void k_bp_gather(const uint8_t* __restrict__ eds, uint32_t klog, uint32_t k,
                                                   const Head* __restrict__ head, const cel_blob_rec* __restrict__ recs,
                                                   const uint64_t* __restrict__ doff, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ src, uint32_t n_blobs,
                                                   uint8_t* __restrict__ data) {
  if (head->k != k) return;
  const uint64_t held = head->n_blobs;
  const uint32_t nb = n_blobs < held ? n_blobs : (uint32_t)held;
  if (!nb) return;
  const uint64_t at = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (at >= doff[nb]) return;
  const uint32_t b = bparse::blob_of(doff, nb, at);
  const uint32_t o = (uint32_t)(at - doff[b]);
  const uint32_t len = recs[b].len;
  uint32_t d[4] = {0u, 0u, 0u, 0u};
  if (o < len) {
    bparse::Piece p0, p1;
    bparse::chunk_pieces(o, len, p0, p1);
    const uint32_t g = first[b];
    take_piece(reinterpret_cast<const uint32_t*>(cell_of(eds, klog, src[g + p0.j] & bparse::kShareMask)), p0, d);
    if (p1.lo < p1.hi)
      take_piece(reinterpret_cast<const uint32_t*>(cell_of(eds, klog, src[g + p1.j] & bparse::kShareMask)), p1, d);
  }
  *reinterpret_cast<uint4*>(data + at) = make_uint4(d[0], d[1], d[2], d[3]);
}

}  // namespace

hipError_t launch_blob_parse_plan(const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const Work& w, hipStream_t s) {
  const Range r("blob_parse_plan");
  const uint32_t klog = log2_of(k), total = (uint32_t)w.total, blocks = (uint32_t)w.blocks;
  uint32_t* sums1 = reinterpret_cast<uint32_t*>(w.sums1);
  uint64_t* sums2 = reinterpret_cast<uint64_t*>(w.sums2);
  hipError_t e = hipMemsetAsync(w.range_short, 0, (size_t)n_ranges * 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bp_classify, dim3(blocks), dim3(256), 0, s, d_eds, klog, w.roff, w.rstart, n_ranges, total, w.cls);
  hipLaunchKernelGGL(k_bp_sums, dim3(blocks), dim3(256), 0, s, w.cls, total, sums1);
  hipLaunchKernelGGL(k_bp_scan, dim3(1), dim3(256), 0, s, sums1, w.blocks, total, k, n_ranges, w.pre, w.head);
  hipLaunchKernelGGL(k_bp_compact, dim3(blocks), dim3(256), 0, s, w.cls, total, sums1, w.pre, w.src, w.cand);
  hipLaunchKernelGGL(k_bp_cand, dim3(blocks), dim3(256), 0, s, w.head, w.roff, w.pre, w.cand, w.range_short);
  hipLaunchKernelGGL(k_bp_status, dim3((n_ranges + 255) / 256), dim3(256), 0, s, w.roff, n_ranges, w.pre, w.src,
                     w.range_short, w.range_status);
  hipLaunchKernelGGL(k_bp_bsums, dim3(blocks), dim3(256), 0, s, w.head, w.cand, w.range_status, sums2);
  hipLaunchKernelGGL(k_bp_bscan, dim3(1), dim3(256), 0, s, sums2, w.blocks, w.doff, w.head);
  hipLaunchKernelGGL(k_bp_bcompact, dim3(blocks), dim3(256), 0, s, d_eds, klog, w.head, w.cand, w.range_status, sums2,
                     w.recs, w.doff, w.first);
  return hipGetLastError();
}

hipError_t launch_blob_parse_gather(const uint8_t* d_eds, uint32_t k, const Work& w, uint32_t n_blobs,
                                    uint64_t total_bytes, uint8_t* d_data, hipStream_t s) {
  if (!n_blobs || !total_bytes) return hipSuccess;
  const Range r("blob_parse_gather");
  const uint64_t chunks = total_bytes / 16;
  hipLaunchKernelGGL(k_bp_gather, dim3((uint32_t)((chunks + 255) / 256)), dim3(256), 0, s, d_eds, log2_of(k), k, w.head,
                     w.recs, w.doff, w.first, w.src, n_blobs, d_data);
  return hipGetLastError();
}

}  // namespace cel
