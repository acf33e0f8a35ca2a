// Txs out of a resident square (tx_parse.hip, api_txs.cpp): go-square v1.1.0 parseCompactShares
// over runs of ODS shares, the inverse of square.cpp's write_compact. The rules are stated in
// include/celestia_eds.h ("txs by range"); here are the header sizes, the uvarint reader, one
// parse step, the walk of the units that begin in one share, the rule by which the shares'
// reserved bytes (the hints) are accepted, the cut of an output chunk into source shares, the
// status rule and the workspace. Everything above the launcher declarations is plain C++ with no
// HIP in it: tools/tx_parse_check.cpp includes this header alone and walks it on the host; under
// hipcc the small functions are device functions as well.
//
// Ranges and flat positions are blob_parse.hpp's. The stream of a range is the concatenation of
// its shares' contributions; all stream positions are relative to the range (64 bits). The
// bytes of a stream are reached through a fetch functor: uint8_t operator()(uint64_t x), x below
// the stream's size.
//
// Hints. A compact share's reserved bytes name the first unit that begins in it, so the units of
// a range can be found with one lane per share and no chain through the range:
//   walked shares  the range's first share, which begins at stream position 0 whatever it names,
//                  and every later share whose value R is usable, h <= R < 512; its hinted start
//                  is its base + R - h.
//   the walk       of a walked share takes the units that begin at or after its start and before
//                  the next share's base, and reads the step behind them too: a walk is stopped
//                  if a step of it stops the parse (the stream's end, a length of 0, a cut unit,
//                  a varint that overflows).
//   the link       of a walked share that is not stopped holds if the position behind its last
//                  unit is the start of the next walked share.
//   T              the first stopped walked share. The hints hold if there is one and every
//                  walked share before it has its link: then the walks up to T are the
//                  sequential parse cut at the shares' bases, by induction over the walked
//                  shares (the first begins where the parse begins; a link hands the parse's
//                  position to the next walk unchanged), and T's stop is the parse's stop. What
//                  lies behind T plays no part, as nothing behind the stop does in the parse.
//   otherwise      one lane walks the range from position 0 (serial_walk), which is the parse by
//                  definition, and the range is flagged CEL_TX_FHINTS.
// In terms of the sequential parse alone, with its last unit beginning in share t: the hints hold
// iff every later share j <= t in which a unit begins names the first such unit, and every one
// in which none begins has no usable value (tx_parse_check.cpp checks the equivalence over all
// hint patterns of short streams; celestia_eds.square.compact_walk states it in Python).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/celestia_eds.h"
#include "blob_parse.hpp"

namespace cel {
namespace txparse {

using bparse::align256;
using bparse::kScanBlock;
using bparse::pad16;

constexpr uint32_t kOk = 0, kEVersion = 1, kENamespace = 2, kEReserved = 3, kEVarint = 4;  // CEL_TX_E*
constexpr uint32_t kStartHdr = 38, kContHdr = 34;  // where the data of a compact share begins
constexpr uint32_t kShareBytes = 512;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// Class flags of a share.
constexpr uint32_t kBadVersion = 1u, kBadNamespace = 2u, kSeqStart = 4u, kFirst = 8u, kBadReserved = 16u,
                   kWalkedShare = 32u;

// A share as the classify kernel leaves it: 16 bytes.
struct Class {
  uint32_t contrib;  // bytes it gives to its range's stream
  uint32_t hint;     // its reserved value R
  uint32_t flags;
  uint32_t share;    // its ODS index
};
static_assert(sizeof(Class) == 16, "Class layout");

CEL_BLOB_HD inline uint32_t header_of(uint32_t info) { return (info & 1u) ? kStartHdr : kContHdr; }

// The class of a share from its info byte, whether its namespace is one of the two compact ones,
// its reserved value and whether it is the first of its range.
CEL_BLOB_HD inline Class classify(uint32_t info, bool compact_ns, uint32_t reserved, bool first, uint32_t share) {
  const uint32_t h = header_of(info);
  Class c{0, reserved, 0, share};
  if (info >> 1) c.flags |= kBadVersion;
  if (!compact_ns) c.flags |= kBadNamespace;
  if (info & 1u) c.flags |= kSeqStart;
  if (first) {
    c.flags |= kFirst | kWalkedShare;
    if (reserved >= kShareBytes) c.flags |= kBadReserved;
    else c.contrib = reserved ? kShareBytes - reserved : 0u;  // R < h too: go slices there
  } else {
    c.contrib = kShareBytes - h;
    if (reserved >= h && reserved < kShareBytes) c.flags |= kWalkedShare;
  }
  return c;
}

// The share byte at which a share's contribution begins.
CEL_BLOB_HD inline uint32_t data_begin(const Class& c) {
  return (c.flags & kFirst) ? c.hint : ((c.flags & kSeqStart) ? kStartHdr : kContHdr);
}

// The status of a range before its units are read: the first of version, namespace, reserved.
CEL_BLOB_HD inline uint32_t class_status(uint64_t nver, uint64_t nns, uint32_t first_flags) {
  if (nver) return kEVersion;
  if (nns) return kENamespace;
  return (first_flags & kBadReserved) ? kEReserved : kOk;
}

// Exclusive prefix sums at a flat position: stream bytes, bad versions, bad namespaces, walked
// shares.
struct Pre {
  uint64_t bytes, ver, ns, walked;
};

CEL_BLOB_HD inline uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >>= 7) n++;
  return n;
}

// binary.Uvarint over the 10 stream bytes at p, zeros behind the stream's end: false for more
// than 10 bytes or a 10th byte above 1. *v: the value; the bytes read play no further part,
// ParseDelimiter skips the value's canonical length.
template <class Fetch>
CEL_BLOB_HD inline bool read_uvarint(Fetch& f, uint64_t p, uint64_t size, uint64_t* v) {
  uint64_t x = 0;
  for (uint32_t i = 0; i < 10; i++) {
    const uint32_t b = p + i < size ? f(p + i) : 0u;
    if (b < 0x80u) {
      if (i == 9 && b > 1) return false;
      *v = x | ((uint64_t)b << (7 * i));
      return true;
    }
    x |= (uint64_t)(b & 0x7Fu) << (7 * i);
  }
  return false;
}

constexpr uint32_t kUnit = 0, kStopEnd = 1, kStopZero = 2, kStopCut = 3, kStopVarint = 4;
struct Step {
  uint64_t len;   // of the unit
  uint32_t n;     // of its prefix (canonical)
  uint32_t kind;  // kUnit, or why the parse stops here
};
// One step of the parse at stream position p <= size.
template <class Fetch>
CEL_BLOB_HD inline Step read_step(Fetch& f, uint64_t p, uint64_t size) {
  if (p >= size) return Step{0, 0, kStopEnd};
  uint64_t len = 0;
  if (!read_uvarint(f, p, size, &len)) return Step{0, 0, kStopVarint};
  if (len == 0) return Step{0, 1, kStopZero};
  const uint32_t n = uvarint_len(len);
  const uint64_t left = size - p >= n ? size - p - n : 0u;  // no sum with len: it may be 2^64 - 1
  if (len > left) return Step{len, n, kStopCut};
  return Step{len, n, kUnit};
}

constexpr uint32_t kWalked = 1u, kStopped = 2u, kVarintErr = 4u;
// The walk of one share: 32 bytes.
struct Walk {
  uint64_t start, end;  // its first unit's position; the position behind its last
  uint64_t bytes;       // its units' lengths, each rounded up to 16
  uint32_t cnt;         // its units
  uint32_t flags;
};
static_assert(sizeof(Walk) == 32, "Walk layout");

// The units that begin in [start, limit), and the step behind them.
template <class Fetch>
CEL_BLOB_HD inline Walk walk_from(Fetch& f, uint64_t start, uint64_t limit, uint64_t size) {
  Walk w{start, start, 0, 0, kWalked};
  uint64_t p = start;
  for (;;) {
    const Step s = read_step(f, p, size);
    if (s.kind != kUnit) {
      w.flags |= kStopped | (s.kind == kStopVarint ? kVarintErr : 0u);
      break;
    }
    if (p >= limit) break;  // it begins in a later share
    w.cnt++;
    w.bytes += pad16(s.len);
    p += s.n + s.len;  // at most size
  }
  w.end = p;
  return w;
}

// The last position j of [a, b) whose base is at or below `at`, a stream position counted from the
// first range on (pre[].bytes itself); pre[a].bytes <= at.
CEL_BLOB_HD inline uint32_t locate_abs(const Pre* pre, uint32_t a, uint32_t b, uint64_t at) {
  while (b - a > 1) {  // pre[a].bytes <= at < pre[b].bytes, or b is the window's end
    const uint32_t mid = a + (b - a) / 2;
    if (pre[mid].bytes <= at) a = mid; else b = mid;
  }
  return a;
}
// The share that holds stream byte x < size of the range [lo, hi). (Only a first share gives no
// bytes; it shares its base with the share behind it and is never the answer for an x below size.)
CEL_BLOB_HD inline uint32_t locate(const Pre* pre, uint32_t lo, uint32_t hi, uint64_t x) {
  return locate_abs(pre, lo, hi, pre[lo].bytes + x);
}

// The first walked share behind p in [lo, hi), or hi.
CEL_BLOB_HD inline uint32_t next_walked(const Pre* pre, uint32_t p, uint32_t hi) {
  const uint64_t seen = pre[p + 1].walked;
  uint32_t a = p, b = hi;  // pre[a + 1].walked == seen; pre[b + 1].walked > seen or b == hi
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (pre[mid + 1].walked == seen) a = mid; else b = mid;
  }
  return b;
}

// The hinted start of walked share p of the range that begins at lo.
CEL_BLOB_HD inline uint64_t hinted_start(const Class& c, const Pre* pre, uint32_t lo, uint32_t p) {
  if (c.flags & kFirst) return 0;
  return pre[p].bytes - pre[lo].bytes + (c.hint - data_begin(c));
}

// Does walked, unstopped share p of [lo, hi) lack its link?
CEL_BLOB_HD inline bool link_broken(const Walk* wk, const Pre* pre, uint32_t p, uint32_t hi) {
  const uint32_t q = next_walked(pre, p, hi);
  return q >= hi || wk[q].start != wk[p].end;
}

// The hints of [lo, hi) from its walks, one share after the other (the device takes the two
// minima in parallel): do they hold, and T.
CEL_BLOB_HD inline bool hints_hold(const Class* cls, const Walk* wk, const Pre* pre, uint32_t lo, uint32_t hi,
                                   uint32_t* t) {
  for (uint32_t p = lo; p < hi; p++) {
    if (!(cls[p].flags & kWalkedShare)) continue;
    if (wk[p].flags & kStopped) {
      *t = p;
      return true;
    }
    if (link_broken(wk, pre, p, hi)) return false;
  }
  return false;
}

// The sequential parse of [lo, hi) cut at the shares' bases into wk[lo .. hi): true if it stopped
// at a varint that overflows.
template <class Fetch>
CEL_BLOB_HD inline bool serial_walk(Fetch& f, const Pre* pre, uint32_t lo, uint32_t hi, Walk* wk) {
  const uint64_t b0 = pre[lo].bytes, size = pre[hi].bytes - b0;
  uint64_t at = 0;
  bool stopped = false, verr = false;
  for (uint32_t p = lo; p < hi; p++) {
    const uint64_t limit = pre[p + 1].bytes - b0;
    Walk w{0, 0, 0, 0, 0};
    if (!stopped && at < limit) {
      w = walk_from(f, at, limit, size);
      at = w.end;
      stopped = (w.flags & kStopped) != 0;
      verr = (w.flags & kVarintErr) != 0;
    }
    wk[p] = w;
  }
  return verr;
}

// One 16-byte chunk of a unit's output: its bytes [0, nbytes), nbytes <= 16, are the stream bytes
// [x, x + nbytes). Share a gives the stream bytes [abase, abase + acontrib), abase <= x <
// abase + acontrib, from its byte abegin on; what it lacks comes from the share behind it, whose
// data begins at byte nbegin (34 or 38) and is 474 bytes or more. For each piece: the chunk's
// bytes [lo, hi) are the share's bytes from q + lo on; q + hi <= 512, and q >= 19 for the second
// piece.
struct Piece {
  uint32_t q;       // share byte that chunk byte 0 falls on
  uint32_t lo, hi;  // chunk bytes taken from this share; lo == hi: none
};
CEL_BLOB_HD inline void chunk_pieces(uint64_t x, uint32_t nbytes, uint64_t abase, uint32_t acontrib, uint32_t abegin,
                                     uint32_t nbegin, Piece& a, Piece& b) {
  const uint64_t avail = abase + acontrib - x;  // 1 .. 512
  a = Piece{abegin + (uint32_t)(x - abase), 0, nbytes < avail ? nbytes : (uint32_t)avail};
  b = Piece{0, 0, 0};
  if (nbytes > avail) b = Piece{nbegin - (uint32_t)avail, (uint32_t)avail, nbytes};
}

// The first bytes of a plan's workspace.
struct Head {
  uint64_t n_units, total_bytes;
  uint64_t emit_bytes;  // the data bytes of the units of the last emit call
  uint64_t total;       // flat positions of the plan
  uint32_t k, n_ranges;
};

// Exclusive prefix sums of the walks that count: units, padded bytes.
struct UnitPre {
  uint64_t units, bytes;
};

// The workspace of a plan of n_ranges ranges with `total` shares: linear in both, whatever the
// number of units. On a null base every pointer is null and bytes is the size.
struct Work {
  Head* head;
  uint32_t* roff;          // [n_ranges + 1] uploaded
  uint32_t* rstart;        // [n_ranges] uploaded, behind roff in one copy
  uint32_t* range_status;  // [n_ranges]
  uint32_t* range_flags;   // [n_ranges]
  uint32_t* range_t;       // [n_ranges] T; behind the plan: the last position whose walk counts
  uint32_t* range_bad;     // [n_ranges] the first walked share without its link
  Class* cls;              // [total]
  Pre* pre;                // [total + 1]
  Walk* wk;                // [total]
  UnitPre* upre;           // [total + 1]
  Pre* sums1;              // [blocks]
  UnitPre* sums2;          // [blocks]
  uint64_t total, blocks;
  size_t bytes;
};

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
  w.roff = reinterpret_cast<uint32_t*>(take((2 * (size_t)n_ranges + 1) * 4));
  w.rstart = w.roff ? w.roff + n_ranges + 1 : nullptr;
  w.range_status = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.range_flags = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.range_t = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.range_bad = reinterpret_cast<uint32_t*>(take((size_t)n_ranges * 4));
  w.cls = reinterpret_cast<Class*>(take((size_t)total * sizeof(Class)));
  w.pre = reinterpret_cast<Pre*>(take(((size_t)total + 1) * sizeof(Pre)));
  w.wk = reinterpret_cast<Walk*>(take((size_t)total * sizeof(Walk)));
  w.upre = reinterpret_cast<UnitPre*>(take(((size_t)total + 1) * sizeof(UnitPre)));
  w.sums1 = reinterpret_cast<Pre*>(take((size_t)w.blocks * sizeof(Pre)));
  w.sums2 = reinterpret_cast<UnitPre*>(take((size_t)w.blocks * sizeof(UnitPre)));
  w.bytes = off;
  return w;
}

}  // namespace txparse
}  // namespace cel

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace cel {

// Classify, scan, walk and count the ranges whose offsets and starts are in w.roff / w.rstart
// (tx_parse.hip): afterwards w.head, w.range_status, w.range_flags, w.wk and w.upre hold the plan.
hipError_t launch_tx_parse_plan(const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const txparse::Work& w,
                                hipStream_t s);
// The records of the first min(n_units, head->n_units) units of the plan in w into d_recs, their
// bytes into d_data (16-byte aligned) at the records' data offsets and, with d_hashes, their
// SHA-256 (32 bytes each). total_bytes: what the host knows of the plan, it sizes the gather's
// grid; the kernel stops at the device's own figure.
hipError_t launch_tx_parse_emit(const uint8_t* d_eds, uint32_t k, const txparse::Work& w, uint32_t n_ranges,
                                uint64_t n_units, uint64_t total_bytes, cel_tx_rec* d_recs, uint8_t* d_data, uint8_t* d_hashes,
                                hipStream_t s);

}  // namespace cel
#endif
