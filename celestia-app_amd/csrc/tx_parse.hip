// Txs out of a resident square (tx_parse.hpp): go-square v1.1.0 parseCompactShares over runs of
// ODS shares, the units' bytes gathered 16-byte aligned and, optionally, their SHA-256. The
// inverse of square.cpp's write_compact; it replaces a download of the compact shares and a
// serial parse on the host. The varint chain of a range is cut at the shares by their reserved
// bytes (the hints, tx_parse.hpp), so the work is one lane per share; the scans are
// blob_parse.hip's (scan_device.hpp), every place a prefix sum.
//
// k_tx_classify  one lane per share of the ranges (flat position p): the 38-byte head of its
//                cell gives the bytes it contributes, its hint and its flags.
// k_tx_sums, k_tx_scan, k_tx_bases  scan 1: each position's stream base (64 bits) and the
//                counts of bad versions, bad namespaces and walked shares before it.
// k_tx_status    one lane per range: its status from the counts and its first share.
// k_tx_walk      one lane per walked share: txparse::walk_from. A stopped walk lowers its range's
//                T with a vector atomic minimum: the result is the minimum, whatever the order.
// k_tx_link      one lane per walked share that is not stopped: a broken link lowers its range's
//                first-broken position the same way.
// k_tx_resolve   one lane per range: the hints hold if T is below the first broken link; then a
//                varint error at T is the range's. Otherwise the lane walks the range serially
//                (txparse::serial_walk) over the walks' table and flags the range.
// k_tx_usums, k_tx_uscan, k_tx_ubases  scan 2 over the walks that count (range without error,
//                position up to T): units and bytes rounded up to 16 before each position.
// k_tx_records   one lane per counting walk: it reads its units' prefixes again and writes their
//                records at their places.
// k_tx_gather    destination-driven like k_bp_gather: a lane owns one 16-byte chunk of one
//                unit's output and stores it with one aligned 16-byte store; its bytes come from
//                one or two shares, each read as five aligned dwords and funnelled with
//                v_alignbyte_b32. Bytes past the unit's length are stored as zero.
// k_tx_hash      one lane per unit: SHA-256 of its bytes in the gathered buffer.
//
// Bounds. The host has checked k, the ranges (start <= end <= k * k, fewer than 2^31 shares in
// all: api_txs.cpp, bparse::ranges_error) and carved the workspace for `total` positions and
// n_ranges ranges (txparse::carve). What the cells hold decides sizes, hints and lengths, never
// an address directly:
//   k_tx_classify  p < total; share = rstart[r] + p - roff[r] < ends[r] <= k * k: the cell lies
//                  in Q0 and the 40 bytes read lie in it. contrib <= 512, whatever R is.
//   scans          cls[p], pre[p], p < total; pre and upre have total + 1 entries.
//   StreamFetch    is asked for stream bytes x < size of its range only (read_uvarint and
//                  read_step compare with size first). locate keeps the share in [lo, hi); the
//                  byte is data_begin + (x - base) < data_begin + contrib = 512.
//   k_tx_walk      a walk's positions never pass size: a unit is taken only if it fits.
//   k_tx_link      next_walked answers in (p, hi]; wk[q] is read for q < hi only.
//   k_tx_resolve   T < hi when it is not kNone. serial_walk writes wk[lo .. hi).
//   k_tx_records   unit places u < n <= head->n_units; d_recs has n records by the caller's word.
//                  locate of a unit's last byte: it lies below size.
//   k_tx_gather    chunk at < head->emit_bytes, which k_tx_records set to the end of unit n - 1;
//                  the unit by search over the n records. The record's range, share and offset
//                  are checked against the plan again before they lead anywhere (d_recs is the
//                  caller's memory): r < n_ranges, the share inside its range, the bytes below
//                  the range's size. Of a cell the dwords (q >> 2) + 0 .. 4 are read, each only
//                  if its index is at most 127. The store covers [at, at + 16) below
//                  emit_bytes <= head->total_bytes, which the plan call gave the caller.
//   k_tx_hash      reads the 16-byte chunks below pad16(len) of its unit, writes 32 bytes at 32 u.
// Nothing of an emit runs when head->k is not the k passed.
#include <hip/hip_runtime.h>

#include "cel_internal.hpp"
#include "scan_device.hpp"
#include "sha256_device.hpp"
#include "tx_parse.hpp"

namespace cel {

using bparse::range_of;
using scan::block_scan;
using scan::cell_of;
using scan::kWaves;
using scan::log2_of;
using scan::scan_blocks;
using txparse::Class;
using txparse::Head;
using txparse::kNone;
using txparse::Pre;
using txparse::UnitPre;
using txparse::Walk;
using txparse::Work;

namespace {

__global__ __launch_bounds__(256) void k_tx_classify(const uint8_t* __restrict__ eds, uint32_t klog,
                                                     const uint32_t* __restrict__ roff,
                                                     const uint32_t* __restrict__ rstart, uint32_t n_ranges,
                                                     uint32_t total, Class* __restrict__ cls) {
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t r = range_of(roff, n_ranges, p);
  const uint32_t share = rstart[r] + (p - roff[r]);
  const uint4* cell = cell_of(eds, klog, share);
  const uint4 a = cell[0], b = cell[1];
  const uint32_t c0 = reinterpret_cast<const uint32_t*>(cell)[8], c1 = reinterpret_cast<const uint32_t*>(cell)[9];
  const uint32_t info = (b.w >> 8) & 0xFFu, last = b.w & 0xFFu;
  const bool compact = (a.x | a.y | a.z | a.w | b.x | b.y | b.z) == 0u && (last == 0x01u || last == 0x04u);
  // the reserved value, big-endian at bytes 30 .. 33 of a continuation, 34 .. 37 of a start
  const uint32_t cont = (((b.w >> 16) & 0xFFu) << 24) | ((b.w >> 24) << 16) | ((c0 & 0xFFu) << 8) | ((c0 >> 8) & 0xFFu);
  const uint32_t start = (((c0 >> 16) & 0xFFu) << 24) | ((c0 >> 24) << 16) | ((c1 & 0xFFu) << 8) | ((c1 >> 8) & 0xFFu);
  cls[p] = txparse::classify(info, compact, (info & 1u) ? start : cont, p == roff[r], share);
}

// The counters of position p; zero beyond the ranges.
__device__ __forceinline__ void share_counts(const Class* __restrict__ cls, uint32_t p, uint32_t total,
                                             uint64_t (&v)[4]) {
  Class c{0, 0, 0, 0};
  if (p < total) c = cls[p];
  v[0] = c.contrib;
  v[1] = (c.flags & txparse::kBadVersion) ? 1u : 0u;
  v[2] = (c.flags & txparse::kBadNamespace) ? 1u : 0u;
  v[3] = (c.flags & txparse::kWalkedShare) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_tx_sums(const Class* __restrict__ cls, uint32_t total,
                                                 uint64_t* __restrict__ sums1) {
  __shared__ uint64_t sh[kWaves * 4];
  uint64_t v[4], tot[4];
  share_counts(cls, blockIdx.x * txparse::kScanBlock + threadIdx.x, total, v);
  block_scan<uint64_t, 4>(v, tot, sh);
  if (threadIdx.x == 0) {
    for (int i = 0; i < 4; i++) sums1[blockIdx.x * 4 + i] = tot[i];
  }
}

__global__ __launch_bounds__(256) void k_tx_scan(uint64_t* __restrict__ sums1, uint64_t blocks, uint32_t total,
                                                 uint32_t k, uint32_t n_ranges, Pre* __restrict__ pre,
                                                 Head* __restrict__ head) {
  __shared__ uint64_t part[257 * 4];
  uint64_t tot[4];
  scan_blocks<uint64_t, 4>(sums1, blocks, tot, part);
  if (threadIdx.x == 0) {
    pre[total] = Pre{tot[0], tot[1], tot[2], tot[3]};
    head->total = total;
    head->k = k;
    head->n_ranges = n_ranges;
  }
}

__global__ __launch_bounds__(256) void k_tx_bases(const Class* __restrict__ cls, uint32_t total,
                                                  const uint64_t* __restrict__ sums1, Pre* __restrict__ pre) {
  __shared__ uint64_t sh[kWaves * 4];
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  uint64_t v[4], tot[4];
  share_counts(cls, p, total, v);
  const uint64_t mine[4] = {v[0], v[1], v[2], v[3]};
  block_scan<uint64_t, 4>(v, tot, sh);
  if (p >= total) return;
  const uint64_t* s = sums1 + (size_t)blockIdx.x * 4;
  pre[p] = Pre{s[0] + (v[0] - mine[0]), s[1] + (v[1] - mine[1]), s[2] + (v[2] - mine[2]), s[3] + (v[3] - mine[3])};
}

__global__ __launch_bounds__(256) void k_tx_status(const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                                   const Class* __restrict__ cls, const Pre* __restrict__ pre,
                                                   uint32_t* __restrict__ range_status,
                                                   uint32_t* __restrict__ range_flags, uint32_t* __restrict__ range_t,
                                                   uint32_t* __restrict__ range_bad) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_ranges) return;
  const uint32_t lo = roff[r], hi = roff[r + 1];
  const Pre a = pre[lo], b = pre[hi];
  range_status[r] = txparse::class_status(b.ver - a.ver, b.ns - a.ns, hi > lo ? cls[lo].flags : 0u);
  range_flags[r] = 0u;
  range_t[r] = kNone;
  range_bad[r] = kNone;
}

// The bytes of one range's stream out of the cells.
struct StreamFetch {
  const uint8_t* eds;
  uint32_t klog;
  const Class* cls;
  const Pre* pre;
  uint32_t lo, hi;
  uint32_t cur;  // the share asked for last, in [lo, hi)
  __device__ __forceinline__ uint8_t operator()(uint64_t x) {
    const uint64_t at = pre[lo].bytes + x;
    if (!(pre[cur].bytes <= at && at < pre[cur + 1].bytes)) cur = txparse::locate(pre, lo, hi, x);
    const Class c = cls[cur];
    const uint32_t byte = txparse::data_begin(c) + (uint32_t)(at - pre[cur].bytes);
    return reinterpret_cast<const uint8_t*>(cell_of(eds, klog, c.share))[byte & 511u];
  }
};

__global__ __launch_bounds__(256) void k_tx_walk(const uint8_t* __restrict__ eds, uint32_t klog,
                                                 const uint32_t* __restrict__ roff, uint32_t n_ranges, uint32_t total,
                                                 const Class* __restrict__ cls, const Pre* __restrict__ pre,
                                                 const uint32_t* __restrict__ range_status, Walk* __restrict__ wk,
                                                 uint32_t* __restrict__ range_t) {
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t r = range_of(roff, n_ranges, p);
  const Class c = cls[p];
  Walk w{0, 0, 0, 0, 0};
  if (range_status[r] == txparse::kOk && (c.flags & txparse::kWalkedShare)) {
    const uint32_t lo = roff[r], hi = roff[r + 1];
    const uint64_t b0 = pre[lo].bytes;
    StreamFetch f{eds, klog, cls, pre, lo, hi, p};
    w = txparse::walk_from(f, txparse::hinted_start(c, pre, lo, p), pre[p + 1].bytes - b0, pre[hi].bytes - b0);
    if (w.flags & txparse::kStopped) atomicMin(&range_t[r], p);
  }
  wk[p] = w;
}

__global__ __launch_bounds__(256) void k_tx_link(const uint32_t* __restrict__ roff, uint32_t n_ranges, uint32_t total,
                                                 const Pre* __restrict__ pre, const Walk* __restrict__ wk,
                                                 uint32_t* __restrict__ range_bad) {
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  if (p >= total) return;
  const uint32_t fl = wk[p].flags;
  if (!(fl & txparse::kWalked) || (fl & txparse::kStopped)) return;
  const uint32_t r = range_of(roff, n_ranges, p);
  if (txparse::link_broken(wk, pre, p, roff[r + 1])) atomicMin(&range_bad[r], p);
}

__global__ __launch_bounds__(256) void k_tx_resolve(const uint8_t* __restrict__ eds, uint32_t klog,
                                                    const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                                    const Class* __restrict__ cls, const Pre* __restrict__ pre,
                                                    Walk* __restrict__ wk, uint32_t* __restrict__ range_status,
                                                    uint32_t* __restrict__ range_flags, uint32_t* __restrict__ range_t,
                                                    const uint32_t* __restrict__ range_bad) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_ranges) return;
  const uint32_t lo = roff[r], hi = roff[r + 1];
  if (range_status[r] != txparse::kOk || lo == hi) return;
  const uint32_t t = range_t[r], bad = range_bad[r];
  bool verr;
  if (t != kNone && t < bad) {
    verr = (wk[t].flags & txparse::kVarintErr) != 0;
  } else {
    StreamFetch f{eds, klog, cls, pre, lo, hi, lo};
    verr = txparse::serial_walk(f, pre, lo, hi, wk);
    range_flags[r] = CEL_TX_FHINTS;
    range_t[r] = hi - 1;
  }
  if (verr) range_status[r] = txparse::kEVarint;
}

// The walk of position p if it counts, else none.
__device__ __forceinline__ Walk counting_walk(const Walk* __restrict__ wk, uint32_t p, uint32_t total,
                                              const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                              const uint32_t* __restrict__ range_status,
                                              const uint32_t* __restrict__ range_t, uint32_t* range) {
  Walk w{0, 0, 0, 0, 0};
  *range = 0;
  if (p >= total) return w;
  const uint32_t r = range_of(roff, n_ranges, p);
  *range = r;
  if (range_status[r] != txparse::kOk || p > range_t[r]) return w;  // T is kNone for an empty range only
  w = wk[p];
  if (!(w.flags & txparse::kWalked)) w.cnt = 0, w.bytes = 0;
  return w;
}

__global__ __launch_bounds__(256) void k_tx_usums(const Walk* __restrict__ wk, uint32_t total,
                                                  const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                                  const uint32_t* __restrict__ range_status,
                                                  const uint32_t* __restrict__ range_t, uint64_t* __restrict__ sums2) {
  __shared__ uint64_t sh[kWaves * 2];
  uint32_t r;
  const Walk w = counting_walk(wk, blockIdx.x * txparse::kScanBlock + threadIdx.x, total, roff, n_ranges, range_status,
                               range_t, &r);
  uint64_t v[2] = {w.cnt, w.bytes}, tot[2];
  block_scan<uint64_t, 2>(v, tot, sh);
  if (threadIdx.x == 0) {
    sums2[blockIdx.x * 2] = tot[0];
    sums2[blockIdx.x * 2 + 1] = tot[1];
  }
}

__global__ __launch_bounds__(256) void k_tx_uscan(uint64_t* __restrict__ sums2, uint64_t blocks, uint32_t total,
                                                  UnitPre* __restrict__ upre, Head* __restrict__ head) {
  __shared__ uint64_t part[257 * 2];
  uint64_t tot[2];
  scan_blocks<uint64_t, 2>(sums2, blocks, tot, part);
  if (threadIdx.x == 0) {
    upre[total] = UnitPre{tot[0], tot[1]};
    head->n_units = tot[0];
    head->total_bytes = tot[1];
    head->emit_bytes = 0;
  }
}

__global__ __launch_bounds__(256) void k_tx_ubases(const Walk* __restrict__ wk, uint32_t total,
                                                   const uint32_t* __restrict__ roff, uint32_t n_ranges,
                                                   const uint32_t* __restrict__ range_status,
                                                   const uint32_t* __restrict__ range_t,
                                                   const uint64_t* __restrict__ sums2, UnitPre* __restrict__ upre) {
  __shared__ uint64_t sh[kWaves * 2];
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  uint32_t r;
  const Walk w = counting_walk(wk, p, total, roff, n_ranges, range_status, range_t, &r);
  uint64_t v[2] = {w.cnt, w.bytes}, tot[2];
  block_scan<uint64_t, 2>(v, tot, sh);
  if (p >= total) return;
  upre[p] = UnitPre{sums2[blockIdx.x * 2] + (v[0] - w.cnt), sums2[blockIdx.x * 2 + 1] + (v[1] - w.bytes)};
}

__global__ __launch_bounds__(256) void k_tx_records(const uint8_t* __restrict__ eds, uint32_t klog, uint32_t k,
                                                    Head* __restrict__ head, const uint32_t* __restrict__ roff,
                                                    uint32_t n_ranges, uint32_t total, const Class* __restrict__ cls,
                                                    const Pre* __restrict__ pre, const Walk* __restrict__ wk,
                                                    const UnitPre* __restrict__ upre,
                                                    const uint32_t* __restrict__ range_status,
                                                    const uint32_t* __restrict__ range_t, uint64_t n_units,
                                                    cel_tx_rec* __restrict__ recs) {
  if (head->k != k) return;
  const uint64_t held = head->n_units;
  const uint64_t n = n_units < held ? n_units : held;
  const uint32_t p = blockIdx.x * txparse::kScanBlock + threadIdx.x;
  uint32_t r;
  const Walk w = counting_walk(wk, p, total, roff, n_ranges, range_status, range_t, &r);
  if (!w.cnt) return;
  const uint32_t lo = roff[r], hi = roff[r + 1];
  const uint64_t b0 = pre[lo].bytes, size = pre[hi].bytes - b0, base = pre[p].bytes - b0;
  const Class c = cls[p];
  StreamFetch f{eds, klog, cls, pre, lo, hi, p};
  uint64_t at = w.start, off = upre[p].bytes;
  const uint64_t u0 = upre[p].units;
  for (uint32_t i = 0; i < w.cnt && u0 + i < n; i++) {
    const txparse::Step s = txparse::read_step(f, at, size);
    if (s.kind != txparse::kUnit) return;  // the walk took it, so it is one
    const uint32_t last = txparse::locate(pre, lo, hi, at + s.n + s.len - 1);
    uint4* out = reinterpret_cast<uint4*>(recs + (u0 + i));
    out[0] = make_uint4(r, c.share, txparse::data_begin(c) + (uint32_t)(at - base), last - p + 1u);
    out[1] = make_uint4((uint32_t)s.len, (uint32_t)(s.len >> 32), (uint32_t)off, (uint32_t)(off >> 32));
    at += s.n + s.len;
    off += txparse::pad16(s.len);
    if (u0 + i == n - 1) head->emit_bytes = off;
  }
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
__device__ __forceinline__ void take_piece(const uint32_t* __restrict__ cell, const txparse::Piece& pc, uint32_t (&d)[4]) {
  if (pc.lo >= pc.hi) return;
  const uint32_t w0 = pc.q >> 2, a = pc.q & 3u;
  uint32_t x[5];
#pragma unroll
  for (uint32_t i = 0; i < 5; i++) x[i] = w0 + i <= 127u ? cell[w0 + i] : 0u;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) d[i] |= __builtin_amdgcn_alignbyte(x[i + 1], x[i], a) & byte_mask(4u * i, pc.lo, pc.hi);
}

// The unit that owns output byte `at` below the end of unit n - 1: the last u with
// recs[u].data_off <= at. Every unit has at least 16 bytes of output.
__device__ __forceinline__ uint64_t unit_of(const cel_tx_rec* __restrict__ recs, uint64_t n, uint64_t at) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (recs[mid].data_off <= at) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_tx_gather(const uint8_t* __restrict__ eds, uint32_t klog, uint32_t k,
                                                   const Head* __restrict__ head, const uint32_t* __restrict__ roff,
                                                   const uint32_t* __restrict__ rstart, const Class* __restrict__ cls,
                                                   const Pre* __restrict__ pre, const cel_tx_rec* __restrict__ recs,
                                                   uint64_t n_units, uint8_t* __restrict__ data) {
  if (head->k != k) return;
  const uint64_t held = head->n_units;
  const uint64_t n = n_units < held ? n_units : held;
  if (!n) return;
  const uint64_t at = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (at >= head->emit_bytes) return;
  const cel_tx_rec rec = recs[unit_of(recs, n, at)];
  uint32_t d[4] = {0u, 0u, 0u, 0u};
  const uint64_t o = at - rec.data_off;
  if (rec.range < head->n_ranges && o < rec.len) {
    const uint32_t lo = roff[rec.range], hi = roff[rec.range + 1];
    const uint32_t p = lo + (rec.share - rstart[rec.range]);
    if (rec.share >= rstart[rec.range] && p < hi) {
      const uint64_t b0 = pre[lo].bytes, size = pre[hi].bytes - b0;
      const Class c = cls[p];
      const uint64_t x = pre[p].bytes - b0 + (rec.share_off - txparse::data_begin(c)) + txparse::uvarint_len(rec.len) + o;
      const uint32_t nbytes = rec.len - o < 16u ? (uint32_t)(rec.len - o) : 16u;
      if (rec.share_off >= txparse::data_begin(c) && x < size && nbytes <= size - x) {
        // the unit's own shares are window enough; a wrong count in the caller's record only
        // makes the pieces miss, the reads stay inside the cells of [p, hi)
        const uint32_t a = txparse::locate_abs(pre, p, rec.shares < hi - p ? p + rec.shares : hi, b0 + x);
        const Class ca = cls[a];
        const Class cb = a + 1 < hi ? cls[a + 1] : ca;
        txparse::Piece p0, p1;
        txparse::chunk_pieces(x, nbytes, pre[a].bytes - b0, ca.contrib, txparse::data_begin(ca), txparse::data_begin(cb),
                              p0, p1);
        take_piece(reinterpret_cast<const uint32_t*>(cell_of(eds, klog, ca.share)), p0, d);
        if (p1.lo < p1.hi && a + 1 < hi)
          take_piece(reinterpret_cast<const uint32_t*>(cell_of(eds, klog, cb.share)), p1, d);
      }
    }
  }
  *reinterpret_cast<uint4*>(data + at) = make_uint4(d[0], d[1], d[2], d[3]);
}

__global__ __launch_bounds__(256) void k_tx_hash(uint32_t k, const Head* __restrict__ head,
                                                 const cel_tx_rec* __restrict__ recs, uint64_t n_units,
                                                 const uint8_t* __restrict__ data, uint8_t* __restrict__ hashes) {
  if (head->k != k) return;
  const uint64_t held = head->n_units;
  const uint64_t n = n_units < held ? n_units : held;
  const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (u >= n) return;
  const cel_tx_rec rec = recs[u];
  const uint4* src = reinterpret_cast<const uint4*>(data + rec.data_off);
  const uint64_t chunks = txparse::pad16(rec.len) / 16, blocks = (rec.len + 9 + 63) / 64;
  const uint64_t mark_block = rec.len / 64;
  const uint32_t mark_word = (uint32_t)(rec.len % 64) / 4, mark = 0x80u << (24u - 8u * (uint32_t)(rec.len % 4));
  uint32_t st[8];
  sha256_init(st);
  // one lane, one chain of compressions: the next block's loads are in flight during this one's
  uint4 next[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) next[q] = q < chunks ? src[q] : make_uint4(0u, 0u, 0u, 0u);
  for (uint64_t blk = 0; blk < blocks; blk++) {
    uint32_t w[16];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint4 v = next[q];
      w[4 * q] = bswap32(v.x), w[4 * q + 1] = bswap32(v.y), w[4 * q + 2] = bswap32(v.z), w[4 * q + 3] = bswap32(v.w);
      const uint64_t ch = (blk + 1) * 4 + q;
      next[q] = ch < chunks ? src[ch] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (blk == mark_block) {
#pragma unroll
      for (uint32_t i = 0; i < 16; i++)
        if (i == mark_word) w[i] |= mark;  // the bytes behind the unit are zero in the buffer
    }
    if (blk == blocks - 1) {
      w[14] = (uint32_t)((rec.len * 8) >> 32);
      w[15] = (uint32_t)(rec.len * 8);
    }
    sha256_compress_unrolled(st, w);
  }
  uint4* out = reinterpret_cast<uint4*>(hashes + u * 32);
  out[0] = make_uint4(bswap32(st[0]), bswap32(st[1]), bswap32(st[2]), bswap32(st[3]));
  out[1] = make_uint4(bswap32(st[4]), bswap32(st[5]), bswap32(st[6]), bswap32(st[7]));
}

}  // namespace

hipError_t launch_tx_parse_plan(const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const Work& w, hipStream_t s) {
  const Range r("tx_parse_plan");
  const uint32_t klog = log2_of(k), total = (uint32_t)w.total, blocks = (uint32_t)w.blocks;
  const uint32_t rblocks = (n_ranges + 255) / 256;
  uint64_t* sums1 = reinterpret_cast<uint64_t*>(w.sums1);
  uint64_t* sums2 = reinterpret_cast<uint64_t*>(w.sums2);
  hipLaunchKernelGGL(k_tx_classify, dim3(blocks), dim3(256), 0, s, d_eds, klog, w.roff, w.rstart, n_ranges, total, w.cls);
  hipLaunchKernelGGL(k_tx_sums, dim3(blocks), dim3(256), 0, s, w.cls, total, sums1);
  hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(256), 0, s, sums1, w.blocks, total, k, n_ranges, w.pre, w.head);
  hipLaunchKernelGGL(k_tx_bases, dim3(blocks), dim3(256), 0, s, w.cls, total, sums1, w.pre);
  hipLaunchKernelGGL(k_tx_status, dim3(rblocks), dim3(256), 0, s, w.roff, n_ranges, w.cls, w.pre, w.range_status,
                     w.range_flags, w.range_t, w.range_bad);
  hipLaunchKernelGGL(k_tx_walk, dim3(blocks), dim3(256), 0, s, d_eds, klog, w.roff, n_ranges, total, w.cls, w.pre,
                     w.range_status, w.wk, w.range_t);
  hipLaunchKernelGGL(k_tx_link, dim3(blocks), dim3(256), 0, s, w.roff, n_ranges, total, w.pre, w.wk, w.range_bad);
  hipLaunchKernelGGL(k_tx_resolve, dim3(rblocks), dim3(256), 0, s, d_eds, klog, w.roff, n_ranges, w.cls, w.pre, w.wk,
                     w.range_status, w.range_flags, w.range_t, w.range_bad);
  hipLaunchKernelGGL(k_tx_usums, dim3(blocks), dim3(256), 0, s, w.wk, total, w.roff, n_ranges, w.range_status, w.range_t,
                     sums2);
  hipLaunchKernelGGL(k_tx_uscan, dim3(1), dim3(256), 0, s, sums2, w.blocks, total, w.upre, w.head);
  hipLaunchKernelGGL(k_tx_ubases, dim3(blocks), dim3(256), 0, s, w.wk, total, w.roff, n_ranges, w.range_status,
                     w.range_t, sums2, w.upre);
  return hipGetLastError();
}

hipError_t launch_tx_parse_emit(const uint8_t* d_eds, uint32_t k, const Work& w, uint32_t n_ranges, uint64_t n_units,
                                uint64_t total_bytes, cel_tx_rec* d_recs, uint8_t* d_data, uint8_t* d_hashes,
                                hipStream_t s) {
  if (!n_units) return hipSuccess;
  const Range r("tx_parse_emit");
  const uint32_t klog = log2_of(k), total = (uint32_t)w.total, blocks = (uint32_t)w.blocks;
  hipError_t e = hipMemsetAsync(&w.head->emit_bytes, 0, sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tx_records, dim3(blocks), dim3(256), 0, s, d_eds, klog, k, w.head, w.roff, n_ranges, total,
                     w.cls, w.pre, w.wk, w.upre, w.range_status, w.range_t, n_units, d_recs);
  const uint64_t chunks = total_bytes / 16;
  if (chunks)
    hipLaunchKernelGGL(k_tx_gather, dim3((uint32_t)((chunks + 255) / 256)), dim3(256), 0, s, d_eds, klog, k, w.head, w.roff,
                       w.rstart, w.cls, w.pre, d_recs, n_units, d_data);
  if (d_hashes)
    hipLaunchKernelGGL(k_tx_hash, dim3((uint32_t)((n_units + 255) / 256)), dim3(256), 0, s, k, w.head, d_recs, n_units,
                       d_data, d_hashes);
  return hipGetLastError();
}

}  // namespace cel
