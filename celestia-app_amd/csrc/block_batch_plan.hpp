// The batched block path's host planner (api_block.cpp, cel_block_extend_batch and
// cel_dev_square_build_batch): everything it decides from each block's (k, status, segment
// count, compact share count) alone. Blocks that constructed are grouped into width classes
// (ascending k, the caller's order kept inside a class), so that launch_extend and launch_commit,
// which batch squares of one k lying back to back, serve a class with one launch each; the
// class-ordered blocks are cut into chunks whose EDS bytes fit a budget; and every block gets
// the record k_square_build_batch (square_build.hip) reads. Plain C++ with no HIP in it:
// tools/block_batch_plan_check.cpp includes this header alone and walks it on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cel {
namespace bb {

constexpr uint64_t kShareBytes = 512;
// EDS bytes of one chunk when the caller names no budget: 64 squares of k = 128 (32 MiB each),
// a quarter of the headline batch of 256. Chosen by reasoning, not by a sweep: a k = 128 class
// of 64 squares gives the batched extension and commit kernels 64 times the workgroups that
// fill the card for one square, so a larger chunk cannot raise their rate much, while the
// ctx's grow-only EDS scratch stays at 2 GiB, under 1 % of the card's HBM. A range of small
// blocks (k <= 32, 2 MiB each at most) fits one chunk up to a thousand heights.
constexpr uint64_t kDefaultEdsBudget = 2ull << 30;
// No chunk budget above this: a chunk's shares * 32 lanes stay below 2^32 (2^25 shares), so the
// kernel's 32-bit lane index covers every chunk but one made of a single block, and the widest
// block (k = 512, 2^18 shares) is far below it.
constexpr uint64_t kMaxEdsBudget = 1ull << 36;

inline uint64_t eds_bytes(uint32_t k) { return 4ull * k * k * kShareBytes; }

// What the planner reads of a block's layout.
struct BlockIn {
  uint32_t k;         // square width (a power of two) if status == 0
  int32_t status;     // cel_status of the layout: a block with status != 0 is in no chunk
  uint32_t nseg;      // segments
  uint32_t ncompact;  // compact shares
};

// What the kernel reads of a block: 32 bytes, uploaded as they are. cel_square_segment is ABI
// and stays as it is; what the batch adds lives here, and seg_block[] (a parallel array the
// caller fills from seg_base and the segment counts) names a segment's block.
struct BlockRec {
  uint64_t eds_off;       // byte offset of the block's EDS in the chunk's buffer, 16-byte aligned
  uint64_t txs_base;      // added to a BLOB segment's off: where the block's txs start (the caller's; wraps)
  uint32_t first_share;   // the block's first share among the chunk's shares
  uint32_t seg_base;      // its first segment among the chunk's segments
  uint32_t compact_base;  // its first compact share among the chunk's compact shares
  uint32_t klog;          // log2 k
};
static_assert(sizeof(BlockRec) == 32, "uploaded as is");

// A run of blocks of one width inside a chunk: plan.order[first .. first + count).
struct ClassRun {
  uint32_t k, first, count;
};

// plan.order[first .. first + count) and plan.runs[run0 .. run0 + nruns).
struct Chunk {
  uint32_t first, count;
  uint32_t run0, nruns;
  uint64_t eds_bytes;                // of all its blocks, back to back
  uint32_t shares, nseg, ncompact;   // totals: the lengths of the chunk's concatenated plan
};

struct Plan {
  std::vector<uint32_t> order;   // the caller's index of every constructed block, class-ordered
  std::vector<BlockRec> recs;    // parallel to order; txs_base left 0 for the caller
  std::vector<ClassRun> runs;
  std::vector<Chunk> chunks;
  std::vector<int32_t> slot;     // per caller block: its place in order, or -1 if it failed
};

inline uint32_t log2u(uint32_t k) {
  uint32_t l = 0;
  while ((1u << l) < k) l++;
  return l;
}

// budget: EDS bytes per chunk, 0 = kDefaultEdsBudget; a block above the budget is a chunk of
// its own.
inline Plan plan_blocks(const BlockIn* in, uint32_t n, uint64_t budget) {
  if (budget == 0) budget = kDefaultEdsBudget;
  if (budget > kMaxEdsBudget) budget = kMaxEdsBudget;
  Plan p;
  p.slot.assign(n, -1);
  // a stable counting sort by log2 k (k <= 2^31)
  uint32_t cnt[33] = {};
  for (uint32_t i = 0; i < n; i++)
    if (in[i].status == 0) cnt[log2u(in[i].k) + 1]++;
  for (uint32_t l = 0; l < 32; l++) cnt[l + 1] += cnt[l];
  p.order.resize(cnt[32]);
  for (uint32_t i = 0; i < n; i++)
    if (in[i].status == 0) {
      const uint32_t at = cnt[log2u(in[i].k)]++;
      p.order[at] = i;
      p.slot[i] = (int32_t)at;
    }
  p.recs.resize(p.order.size());
  for (uint32_t o = 0; o < p.order.size(); o++) {
    const BlockIn& b = in[p.order[o]];
    const uint64_t bytes = eds_bytes(b.k);
    if (p.chunks.empty() || p.chunks.back().eds_bytes + bytes > budget) p.chunks.push_back(Chunk{o, 0, (uint32_t)p.runs.size(), 0, 0, 0, 0, 0});
    Chunk& c = p.chunks.back();
    if (c.nruns == 0 || p.runs.back().k != b.k) {
      p.runs.push_back(ClassRun{b.k, o, 0});
      c.nruns++;
    }
    p.runs.back().count++;
    p.recs[o] = BlockRec{(c.eds_bytes + 15) & ~15ull, 0, c.shares, c.nseg, c.ncompact, log2u(b.k)};
    c.eds_bytes = p.recs[o].eds_off + bytes;
    c.shares += b.k * b.k;
    c.nseg += b.nseg;
    c.ncompact += b.ncompact;
    c.count++;
  }
  return p;
}

}  // namespace bb
}  // namespace cel
