// Namespace queries on the tree index of a resident square (nmt_namespace.hip,
// api_namespace.cpp): nmt ProveNamespace for every (namespace, row) of a batch. What a row
// yields for a namespace follows from three facts the find kernel collects (does the row's root
// range hold the namespace; how many leaves lie below it; how many at or below it); the
// classification, the node count and the per-entry record the emit kernel reads are here.
// Everything above the launcher declarations is plain C++ with no HIP in it:
// tools/namespace_plan_check.cpp includes this header alone and walks it on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nmt_prove.hpp"

namespace cel {
namespace nsq {

constexpr uint32_t kInclusion = 0;  // CEL_NS_INCLUSION
constexpr uint32_t kAbsence = 1;    // CEL_NS_ABSENCE

// One (namespace, row) pair as the find kernel leaves it: 16 bytes. entry = 0: the row has
// nothing to say about the namespace, and every other field is 0.
struct Pair {
  uint32_t entry;  // 0 or 1
  uint32_t kind;
  uint32_t start, end;
};
static_assert(sizeof(Pair) == 16, "Pair layout");

// inside: root.min <= nid <= root.max. lt / le: the leaves of the row's W whose (min) namespace
// is < nid / <= nid, by counting, so lt <= le <= W for any cells.
//   outside the root's range, or every leaf below nid   no entry
//   le > lt   inclusion of [lt, le)
//   else      absence: [lt, lt + 1), the leaf that follows where the namespace would be;
//             lt < W here, so that leaf is a leaf of the row
CEL_PROVE_HD inline Pair classify(bool inside, uint32_t lt, uint32_t le, uint32_t W) {
  if (!inside || lt >= W) return Pair{0, 0, 0, 0};
  if (le > lt) return Pair{1, kInclusion, lt, le};
  return Pair{1, kAbsence, lt, lt + 1};
}

// The packed nodes of an entry: ProveRange(start, end)'s, and the leaf hash of an absence entry.
CEL_PROVE_HD inline uint32_t entry_nodes(uint32_t L, const Pair& p) {
  return p.entry ? prove::node_count(L, p.start, p.end - 1) + (p.kind == kAbsence ? 1u : 0u) : 0u;
}
// Its shares: an absence entry has none.
CEL_PROVE_HD inline uint32_t entry_leaves(const Pair& p) {
  return p.entry && p.kind == kInclusion ? p.end - p.start : 0u;
}

// One entry of a plan as the emit kernel reads it and as the plan call downloads it: entry e
// of the (namespace index, row) order, its nodes from packed node node0 on, its shares from
// share leaf0 on.
struct Request {
  uint32_t ns_idx, row;
  int32_t start, end;
  uint32_t kind, nnodes;
  uint64_t node0, leaf0;
};
static_assert(sizeof(Request) == 40, "Request layout");

// A plan over a batch index (nmt_prove.hpp: n_squares indexes back to back). Query i is a
// (square, namespace) pair. Its row of the query table is the namespace's 29 bytes and the
// square in the three bytes that pad it to 32, little-endian: the find kernel's compare words
// drop those bytes, so the namespace compares as in a single-square plan. An entry of such a
// plan carries its query's square above its kind, so the emit kernel needs nothing but the entry
// to find the cells and the index slice; the plan call hands the caller the kind alone. The
// head's W of such a plan has kSquaresPlan set: each emit kernel does nothing on a plan of the
// other sort.
constexpr uint32_t kSquaresPlan = 0x80000000u;
constexpr uint32_t kMaxPlanSquares = 1u << 24;  // what three bytes hold; the calls take prove::kMaxSquares
// Word 7 of a query's row of the table -> its square.
CEL_PROVE_HD inline uint32_t query_square(uint32_t word7) { return word7 >> 8; }
CEL_PROVE_HD inline uint32_t entry_pack(uint32_t kind, uint32_t square) { return kind | (square << 8); }
CEL_PROVE_HD inline uint32_t entry_kind(uint32_t packed) { return packed & 0xFFu; }
CEL_PROVE_HD inline uint32_t entry_square(uint32_t packed) { return packed >> 8; }
// Row i of the query table from a namespace and a square < kMaxPlanSquares.
inline void query_row(uint8_t* row, const uint8_t* ns29, uint32_t square) {
  for (uint32_t j = 0; j < 29; j++) row[j] = ns29[j];
  row[29] = (uint8_t)square;
  row[30] = (uint8_t)(square >> 8);
  row[31] = (uint8_t)(square >> 16);
}

// Running sums of the three counters a scan carries.
struct Sums {
  uint64_t entries, nodes, leaves;
};

// The first bytes of a plan's workspace, written by the scan: what the plan holds. The entries
// follow at kReqOff whatever n is, so the emit kernel needs nothing but the workspace to find
// them, and its load of an entry does not wait for a load of the head.
struct Head {
  Sums totals;
  uint64_t W;  // the width the plan was made for: the emit kernel does nothing on another
};
constexpr size_t kReqOff = 256;
static_assert(sizeof(Head) <= kReqOff, "the head is one region");

constexpr uint32_t kScanBlock = 256;  // pairs per block of the prefix sum

// The workspace of a plan of n namespaces over the 2k rows of a square. On a null base every
// pointer is null and bytes is the size.
struct Work {
  Head* head;        // written by the scan, read by the emit kernel
  uint32_t* ns;      // [n][8] the namespaces, 29 bytes zero padded to 32
  Pair* pairs;       // [n * W]
  Sums* block_sums;  // [blocks]; exclusive after the scan
  Request* req;      // [n * W] at most, at kReqOff
  uint64_t blocks, npairs;
  size_t bytes;
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

inline Work carve(void* base, uint32_t k, uint32_t n) {
  uint8_t* b = static_cast<uint8_t*>(base);
  Work w{};
  w.npairs = (uint64_t)n * 2 * k;
  w.blocks = (w.npairs + kScanBlock - 1) / kScanBlock;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t* p = b ? b + off : nullptr;
    off += align256(bytes ? bytes : 1);
    return p;
  };
  w.head = reinterpret_cast<Head*>(take(sizeof(Head)));  // sizeof(Head) <= kReqOff: one region of 256 bytes
  w.req = reinterpret_cast<Request*>(take((size_t)w.npairs * sizeof(Request)));
  w.ns = reinterpret_cast<uint32_t*>(take((size_t)n * 32));
  w.pairs = reinterpret_cast<Pair*>(take((size_t)w.npairs * sizeof(Pair)));
  w.block_sums = reinterpret_cast<Sums*>(take((size_t)w.blocks * sizeof(Sums)));
  w.bytes = off;
  return w;
}

// The prefix sum and compaction on the host, step for step as the kernels run them (the
// counters of each block of kScanBlock pairs; the exclusive scan of the block sums; each pair's
// exclusive prefix inside its block added to its block's base): req gets the entries, the
// return value the totals. tools/namespace_plan_check.cpp walks it.
inline Sums plan_scan(const Pair* pairs, uint64_t npairs, uint32_t W, uint32_t L, Sums* block_sums, Request* req) {
  const uint64_t blocks = (npairs + kScanBlock - 1) / kScanBlock;
  for (uint64_t b = 0; b < blocks; b++) {
    Sums s{0, 0, 0};
    for (uint64_t p = b * kScanBlock; p < npairs && p < (b + 1) * kScanBlock; p++) {
      s.entries += pairs[p].entry ? 1 : 0;
      s.nodes += entry_nodes(L, pairs[p]);
      s.leaves += entry_leaves(pairs[p]);
    }
    block_sums[b] = s;
  }
  Sums run{0, 0, 0};
  for (uint64_t b = 0; b < blocks; b++) {
    const Sums v = block_sums[b];
    block_sums[b] = run;
    run.entries += v.entries;
    run.nodes += v.nodes;
    run.leaves += v.leaves;
  }
  for (uint64_t b = 0; b < blocks; b++) {
    Sums at = block_sums[b];
    for (uint64_t p = b * kScanBlock; p < npairs && p < (b + 1) * kScanBlock; p++) {
      if (!pairs[p].entry) continue;
      const uint32_t nn = entry_nodes(L, pairs[p]);
      req[at.entries] = Request{(uint32_t)(p / W), (uint32_t)(p % W), (int32_t)pairs[p].start, (int32_t)pairs[p].end,
                                pairs[p].kind, nn, at.nodes, at.leaves};
      at.entries++;
      at.nodes += nn;
      at.leaves += entry_leaves(pairs[p]);
    }
  }
  return run;
}

}  // namespace nsq
}  // namespace cel

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace cel {

// Find, prefix sum and compaction of a plan whose namespaces are in w.ns (nmt_namespace.hip):
// afterwards w.head and w.req hold the plan. stages: bit 0 find, bit 1 the prefix sum and the
// compaction (a measurement runs them apart).
hipError_t launch_ns_plan(const void* d_index, uint32_t k, uint32_t n, const nsq::Work& w, int stages, hipStream_t s);
// The first min(n_entries, head->totals.entries) entries of the plan that d_work holds: nodes
// and shares. d_leaves nullable (then eds is not read); both 16-byte aligned. d_nodes 2-byte
// aligned.
hipError_t launch_ns_emit(const uint8_t* eds, const void* d_index, uint32_t k, const void* d_work, uint32_t n_entries,
                          uint8_t* d_leaves, uint8_t* d_nodes, hipStream_t s);
// The two over a batch index: w.ns holds the (square, namespace) query table (nsq::query_row),
// every square below the number of squares the index holds; the emit runs over the entries whose
// square is below n_squares.
hipError_t launch_ns_plan_squares(const void* d_index, uint32_t k, uint32_t n, const nsq::Work& w, hipStream_t s);
hipError_t launch_ns_emit_squares(const uint8_t* eds, const void* d_index, uint32_t k, uint32_t n_squares,
                                  const void* d_work, uint32_t n_entries, uint8_t* d_leaves, uint8_t* d_nodes,
                                  hipStream_t s);

}  // namespace cel
#endif
