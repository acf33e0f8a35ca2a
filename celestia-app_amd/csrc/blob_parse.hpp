// Blobs out of a resident square (blob_parse.hip, api_blobs.cpp): go-square v1.1.0
// parseSparseShares over runs of ODS shares, the inverse of square_build.hip. The share
// classes, the rule that gives a range its status, the place of a blob's bytes in its shares,
// the range checks and the workspace are here. Everything above the launcher declarations is
// plain C++ with no HIP in it: tools/blob_parse_check.cpp includes this header alone and walks
// it on the host; under hipcc the small functions are device functions as well.
//
// A range is [start, end) in row-major ODS index; share s is cell (s / k, s % k) of Q0. The
// shares of all ranges, one range after the other, are the flat positions p = 0 .. total - 1
// (range r owns [roff[r], roff[r + 1])); ranges may overlap or repeat, a position belongs to
// one range.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/celestia_eds.h"
#include "blob_plan.hpp"

namespace cel {
namespace bparse {

constexpr uint32_t kPad = 0;     // tail padding, primary reserved padding, namespace padding: skipped
constexpr uint32_t kStart = 1;   // a sequence start with a length above 0
constexpr uint32_t kCont = 2;    // a continuation
constexpr uint32_t kBadVer = 3;  // a share version other than 0, padding or not

constexpr uint32_t kOk = 0, kEVersion = 1, kENoStart = 2, kEShort = 3;  // CEL_BLOB_E*

constexpr uint32_t kMaxWidth = 512;
constexpr uint64_t kMaxTotal = 1ull << 31;  // shares of all ranges of one plan, exclusive
constexpr uint32_t kShareBits = 18;         // an ODS index is below 512 * 512 = 2^18
constexpr uint32_t kShareMask = (1u << kShareBits) - 1;
constexpr uint32_t kClassShift = 30;        // src entry: ODS index | class << 30

constexpr uint32_t kFirstHdr = 34, kContHdr = 30;  // where the payload of a share begins

// The class of a share from its first 34 bytes: `ns_tail` / `ns_reserved`: its namespace is
// the tail-padding / primary-reserved-padding namespace. The version is looked at first, as
// parseSparseShares does.
CEL_BLOB_HD inline uint32_t classify(uint32_t info, bool ns_tail, bool ns_reserved, uint32_t len) {
  if (info >> 1) return kBadVer;
  if (ns_tail || ns_reserved) return kPad;
  if (info & 1u) return len ? kStart : kPad;
  return kCont;
}

// The status of a range from its walk alone (every error but kEShort). The shares that are
// not padding, bad-version ones among them, are the significant ones; `first` is the class of
// the range's first significant share, nsig and nbad the range's counts. parseSparseShares
// fails at the first share that has a bad version or is a continuation with no start before
// it; a start as the first significant share rules the second out for good.
CEL_BLOB_HD inline uint32_t walk_status(uint32_t nsig, uint32_t first, uint32_t nbad) {
  if (!nsig) return kOk;
  if (first == kBadVer) return kEVersion;
  if (first == kCont) return kENoStart;
  return nbad ? kEVersion : kOk;
}

// Does a blob of declared length len lack bytes with `found` shares? 64-bit throughout: a
// length of 0xFFFFFFFF needs 8,910,721 shares.
CEL_BLOB_HD inline bool is_short(uint32_t len, uint32_t found) {
  const uint64_t need = len <= blob::kSparseFirst ? 1u : 1u + ((uint64_t)len - blob::kSparseFirst + blob::kSparseCont - 1) / blob::kSparseCont;
  return found < need;
}

CEL_BLOB_HD inline uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// Share j of a blob holds the blob's bytes [base, base + cap) from its byte hdr on.
struct Span {
  uint32_t j, base, cap, hdr;
};
CEL_BLOB_HD inline Span span_of_share(uint32_t j) {
  if (j == 0) return Span{0, 0, blob::kSparseFirst, kFirstHdr};
  return Span{j, blob::kSparseFirst + blob::kSparseCont * (j - 1), blob::kSparseCont, kContHdr};
}
// The share that holds byte x of a blob. A blob that is gathered has its shares in one range,
// at most 2^18 of them, so x < 2^27 there and nothing here comes near 32 bits.
CEL_BLOB_HD inline Span span_of_byte(uint32_t x) {
  return span_of_share(x < blob::kSparseFirst ? 0u : 1u + (x - blob::kSparseFirst) / blob::kSparseCont);
}

// One 16-byte chunk of a blob's output, blob bytes [o, o + 16) with o a multiple of 16, takes
// bytes from share `a` and, where the chunk runs past a's last byte before the blob ends, from
// the share behind it. For each: the chunk's bytes [lo, hi) are the share's bytes from q + lo
// on. q >= 15: a payload begins at share byte 30 or 34 and a chunk begins at most 15 bytes
// before the share's first blob byte. q + hi <= 512.
struct Piece {
  uint32_t j;       // share of the blob
  uint32_t q;       // share byte that chunk byte 0 falls on (below the payload for a second piece)
  uint32_t lo, hi;  // chunk bytes taken from this share; lo == hi: none
};
CEL_BLOB_HD inline void chunk_pieces(uint32_t o, uint32_t len, Piece& a, Piece& b) {
  const uint64_t end = (uint64_t)o + 16 < len ? (uint64_t)o + 16 : len;  // o < len
  const Span s = span_of_byte(o);
  const uint64_t s_end = (uint64_t)s.base + s.cap;
  a.j = s.j;
  a.q = s.hdr + (o - s.base);
  a.lo = 0;
  a.hi = (uint32_t)((end < s_end ? end : s_end) - o);
  b = Piece{s.j + 1, 0, 0, 0};
  if (end > s_end) {
    const uint32_t lo = (uint32_t)(s_end - o);  // 1 .. 15
    b.q = kContHdr - lo;
    b.lo = lo;
    b.hi = (uint32_t)(end - o);
  }
}

// "" if the ranges can be planned over a square of width k, else what is wrong; *total: the
// shares of all ranges.
inline std::string ranges_error(uint32_t k, uint32_t n_ranges, const uint32_t* starts, const uint32_t* ends,
                                uint64_t* total) {
  *total = 0;
  if (!k || (k & (k - 1)) || k > kMaxWidth) return "square width " + std::to_string(k) + " is not a power of two up to 512";
  if (n_ranges && (!starts || !ends)) return "nil argument";
  uint64_t sum = 0;
  for (uint32_t r = 0; r < n_ranges; r++) {
    if (starts[r] > ends[r])
      return "range " + std::to_string(r) + ": start " + std::to_string(starts[r]) + " is above end " + std::to_string(ends[r]);
    if (ends[r] > k * k)
      return "range " + std::to_string(r) + ": end " + std::to_string(ends[r]) + " is beyond the " + std::to_string(k * k) +
             " shares of the square";
    sum += ends[r] - starts[r];
    if (sum >= kMaxTotal) return "the ranges hold 2^31 shares or more";
  }
  *total = sum;
  return "";
}

// roff[r]: the flat position of range r's first share; roff[n_ranges] = total.
inline void range_offsets(uint32_t n_ranges, const uint32_t* starts, const uint32_t* ends, uint32_t* roff) {
  uint32_t at = 0;
  for (uint32_t r = 0; r < n_ranges; r++) {
    roff[r] = at;
    at += ends[r] - starts[r];
  }
  roff[n_ranges] = at;
}

// The range of flat position p < roff[n]: the last r with roff[r] <= p (empty ranges share
// their offset with the range behind them and never own a position).
CEL_BLOB_HD inline uint32_t range_of(const uint32_t* roff, uint32_t n, uint32_t p) {
  uint32_t lo = 0, hi = n;  // roff[lo] <= p < roff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (roff[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// The blob that owns output byte `at` < doff[n]: the last b with doff[b] <= at. Every blob has
// at least 16 bytes of output, so the offsets are strictly increasing.
CEL_BLOB_HD inline uint32_t blob_of(const uint64_t* doff, uint32_t n, uint64_t at) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (doff[mid] <= at) lo = mid; else hi = mid;
  }
  return lo;
}

// A share as the classify kernel leaves it: 16 bytes.
struct Class {
  uint32_t cls, len;     // len: the declared length of a start (bytes 30 .. 33, big-endian)
  uint32_t share, range; // its ODS index and its range
};
static_assert(sizeof(Class) == 16, "Class layout");

// Exclusive prefix counts at a flat position: significant shares, starts, bad versions.
struct Pre {
  uint32_t sig, starts, bad;
};

// A start share, a blob unless its range fails: candidate c is the c-th start of the flat order.
struct Cand {
  uint32_t range, share;  // the start share's range and ODS index
  uint32_t g;             // its place in the source list
  uint32_t len;
  uint32_t found;         // significant shares up to the next start or the range's end
  uint32_t reserved;
};

// Running sums of the scan over the candidates.
struct BlobSums {
  uint64_t blobs, bytes, shares;
};

// The first bytes of a plan's workspace. The records follow at kRecOff.
struct Head {
  uint64_t n_blobs, total_bytes, total_shares;  // total_shares: the sum of the records' shares
  uint64_t n_cand, n_sig;
  uint64_t total;  // flat positions of the plan
  uint32_t k, n_ranges;
};
constexpr size_t kRecOff = 256;
static_assert(sizeof(Head) <= kRecOff, "the head is one region");

constexpr uint32_t kScanBlock = 256;

// The workspace of a plan of n_ranges ranges with `total` shares. On a null base every pointer
// is null and bytes is the size. A range of one-share blobs gives a blob per share, so every
// per-blob table has `total` entries.
struct Work {
  Head* head;
  cel_blob_rec* recs;     // [total] at most, at kRecOff
  uint64_t* doff;         // [total + 1] data offset of each blob, then the total
  uint32_t* first;        // [total] the place of each blob's start share in src
  uint32_t* roff;         // [n_ranges + 1] uploaded
  uint32_t* rstart;       // [n_ranges] uploaded, behind roff in one copy
  uint32_t* range_short;  // [n_ranges] a candidate of the range lacks bytes
  uint32_t* range_status; // [n_ranges]
  Class* cls;             // [total]
  Pre* pre;               // [total + 1]
  uint32_t* src;          // [total] the significant shares in flat order
  Cand* cand;             // [total]
  Pre* sums1;             // [blocks]
  BlobSums* sums2;        // [blocks]
  uint64_t total, blocks;
  size_t bytes;
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

inline Work carve(void* base, uint64_t total, uint32_t n_ranges) {
  uint8_t* b = static_cast<uint8_t*>(base);
  Work w{};
  w.total = total;
  w.blocks = total ? (total + kScanBlock - 1) / kScanBlock : 1;  // a plan of empty ranges still writes its head
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t* p = b ? b + off : nullptr;
    off += align256(bytes ? bytes : 1);
    return p;
  };
  w.head = reinterpret_cast<Head*>(take(sizeof(Head)));
  w.recs = reinterpret_cast<cel_blob_rec*>(take((size_t)total * sizeof(cel_blob_rec)));
  w.doff = reinterpret_cast<uint64_t*>(take(((size_t)total + 1) * 8));
  w.first = reinterpret_cast<uint32_t*>(take((size_t)total * 4));
  w.roff = reinterpret_cast<uint32_t*>(take((2 * (size_t)n_ranges + 1) * 4));
  w.rstart = w.roff ? w.roff + n_ranges + 1 : nullptr;
  w.range_short = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.range_status = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.cls = reinterpret_cast<Class*>(take((size_t)total * sizeof(Class)));
  w.pre = reinterpret_cast<Pre*>(take(((size_t)total + 1) * sizeof(Pre)));
  w.src = reinterpret_cast<uint32_t*>(take((size_t)total * 4));
  w.cand = reinterpret_cast<Cand*>(take((size_t)total * sizeof(Cand)));
  w.sums1 = reinterpret_cast<Pre*>(take((size_t)w.blocks * sizeof(Pre)));
  w.sums2 = reinterpret_cast<BlobSums*>(take((size_t)w.blocks * sizeof(BlobSums)));
  w.bytes = off;
  return w;
}

}  // namespace bparse
}  // namespace cel

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace cel {

// Classify, scan and compact the ranges whose offsets and starts are in w.roff / w.rstart
// (blob_parse.hip): afterwards w.head, w.recs, w.doff and w.range_status hold the plan.
hipError_t launch_blob_parse_plan(const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const bparse::Work& w,
                                  hipStream_t s);
// The bytes of the first min(n_blobs, head->n_blobs) blobs of the plan in d_work into d_data
// (16-byte aligned) at the records' data offsets. total_bytes: what the host knows of the plan,
// it sizes the grid; the kernel stops at the device's own figure.
hipError_t launch_blob_parse_gather(const uint8_t* d_eds, uint32_t k, const bparse::Work& w, uint32_t n_blobs,
                                    uint64_t total_bytes, uint8_t* d_data, hipStream_t s);

}  // namespace cel
#endif
