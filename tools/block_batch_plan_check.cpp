// Stand-alone host check of the batched block path's planner
// (celestia-app_amd/csrc/block_batch_plan.hpp): no HIP, no device. Build it with a host
// compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/block_batch_plan_check.cpp -o block_batch_plan_check && ./block_batch_plan_check
// For every multiset of 1 .. 6 widths from {1, 2, 4, ..., 512} it makes a batch: the widths in
// a shuffled order (splitmix64 of the multiset's number), failed blocks (a non-zero status and
// a width that is no power of two) put in front of some of them and behind the last, segment
// and compact share counts drawn per block. It plans the batch under four budgets (one byte;
// the widest block's EDS; the whole batch's EDS bytes; 0, the default) and checks:
// 1. the map back: slot[] is -1 exactly for the failed blocks, and order[slot[i]] == i is a
//    bijection between the constructed blocks and order[];
// 2. classes: widths never fall along order[], and inside a width the caller's indices rise;
// 3. chunks: they follow one another and cover order[] exactly once; none is empty; a chunk
//    above the budget holds one block; a chunk stops only where the next block would not fit;
// 4. class runs: a chunk's runs follow one another and cover it, a run holds one width,
//    neighbouring runs of a chunk differ in width, and a run's EDSs lie back to back;
// 5. records: eds_off is a multiple of 16, the EDS ranges of a chunk rise without overlap and
//    end inside the chunk's bytes; first_share, seg_base and compact_base are the prefix sums
//    of k * k, the segment counts and the compact share counts inside the chunk; klog is
//    log2 k; the chunk's totals are the sums.
// Per batch size it prints the multisets and the chunks summed over the four budgets;
// tests/test_block_batch_plan_check.py works the same figures out with numpy, builds this
// program plain and under ASan + UBSan, and runs it.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "block_batch_plan.hpp"

using namespace cel::bb;

static int fails = 0;
static uint64_t cur_set = 0, cur_budget = 0;
#define CHECK(c)                                                                                          \
  do {                                                                                                    \
    if (!(c)) {                                                                                           \
      if (fails < 20)                                                                                     \
        std::printf("FAIL %s:%d: %s (multiset %llu, budget %llu)\n", __FILE__, __LINE__, #c,              \
                    (unsigned long long)cur_set, (unsigned long long)cur_budget);                         \
      fails++;                                                                                            \
    }                                                                                                     \
  } while (0)

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

static const uint32_t kWidths[10] = {1, 2, 4, 8, 16, 32, 64, 128, 256, 512};
constexpr uint32_t kMaxBlocks = 6;

// The batch of a multiset: shuffled, failed blocks interleaved.
static std::vector<BlockIn> batch_of(const std::vector<uint32_t>& widths, uint64_t seed) {
  std::vector<uint32_t> w = widths;
  for (size_t i = w.size(); i > 1; i--) std::swap(w[i - 1], w[mix(seed * 16 + i) % i]);
  std::vector<BlockIn> out;
  for (size_t i = 0; i < w.size(); i++) {
    const uint64_t h = mix(seed * 64 + 32 + i);
    if (h % 3 == 0) out.push_back(BlockIn{7, h % 2 ? -1 : 2, 3, 1});
    out.push_back(BlockIn{w[i], 0, 1 + (uint32_t)((h >> 8) % 5), (uint32_t)((h >> 16) % 4)});
  }
  if (mix(seed) % 2) out.push_back(BlockIn{0, -5, 0, 0});
  return out;
}

// -> chunks
static uint32_t check_plan(const std::vector<BlockIn>& in, uint64_t budget) {
  const uint32_t n = (uint32_t)in.size();
  const Plan p = plan_blocks(in.data(), n, budget);
  const uint64_t limit = budget == 0 ? kDefaultEdsBudget : budget;
  // 1
  uint32_t ok = 0;
  CHECK(p.slot.size() == n);
  for (uint32_t i = 0; i < n && i < p.slot.size(); i++) {
    if (in[i].status != 0) {
      CHECK(p.slot[i] == -1);
      continue;
    }
    ok++;
    CHECK(p.slot[i] >= 0 && (size_t)p.slot[i] < p.order.size());
    if (p.slot[i] >= 0 && (size_t)p.slot[i] < p.order.size()) CHECK(p.order[p.slot[i]] == i);
  }
  CHECK(p.order.size() == ok && p.recs.size() == ok);
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t i : p.order) {
    CHECK(i < n);
    if (i >= n) return 0;
    CHECK(!seen[i] && in[i].status == 0);
    seen[i] = 1;
  }
  if (p.recs.size() != p.order.size()) return 0;
  // 2
  for (size_t o = 1; o < p.order.size(); o++) {
    const BlockIn &a = in[p.order[o - 1]], &b = in[p.order[o]];
    CHECK(a.k <= b.k);
    if (a.k == b.k) CHECK(p.order[o - 1] < p.order[o]);
  }
  // 3, 4, 5
  uint32_t at = 0, run_at = 0;
  for (const Chunk& c : p.chunks) {
    CHECK(c.first == at && c.count > 0 && c.run0 == run_at && c.nruns > 0);
    if (c.first != at || c.count == 0 || at + c.count > p.order.size()) return 0;
    CHECK(c.eds_bytes <= limit || c.count == 1);
    if (at + c.count < p.order.size()) CHECK(c.eds_bytes + eds_bytes(in[p.order[at + c.count]].k) > limit);
    uint64_t end = 0;
    uint32_t shares = 0, nseg = 0, ncompact = 0;
    for (uint32_t o = at; o < at + c.count; o++) {
      const BlockIn& b = in[p.order[o]];
      const BlockRec& r = p.recs[o];
      CHECK(r.eds_off % 16 == 0 && r.eds_off >= end);
      end = r.eds_off + eds_bytes(b.k);
      CHECK(end <= c.eds_bytes);
      CHECK(r.first_share == shares && r.seg_base == nseg && r.compact_base == ncompact);
      CHECK((1u << r.klog) == b.k && r.txs_base == 0);
      shares += b.k * b.k;
      nseg += b.nseg;
      ncompact += b.ncompact;
    }
    CHECK(end == c.eds_bytes && c.shares == shares && c.nseg == nseg && c.ncompact == ncompact);
    uint32_t o = at;
    for (uint32_t r = c.run0; r < c.run0 + c.nruns; r++) {
      CHECK(r < p.runs.size());
      if (r >= p.runs.size()) return 0;
      const ClassRun& run = p.runs[r];
      CHECK(run.first == o && run.count > 0 && o + run.count <= at + c.count);
      if (run.first != o || o + run.count > at + c.count) return 0;
      if (r > c.run0) CHECK(p.runs[r - 1].k != run.k);
      for (uint32_t q = o; q < o + run.count; q++) {
        CHECK(in[p.order[q]].k == run.k);
        if (q > o) CHECK(p.recs[q].eds_off == p.recs[q - 1].eds_off + eds_bytes(run.k));
      }
      o += run.count;
    }
    CHECK(o == at + c.count);
    at += c.count;
    run_at += c.nruns;
  }
  CHECK(at == p.order.size() && run_at == p.runs.size());
  return (uint32_t)p.chunks.size();
}

int main() {
  uint64_t set_no = 0;
  for (uint32_t m = 1; m <= kMaxBlocks; m++) {
    uint64_t sets = 0, chunks = 0;
    std::vector<uint32_t> idx(m, 0);  // non-decreasing indices into kWidths: a multiset
    for (;;) {
      std::vector<uint32_t> widths(m);
      uint64_t total = 0, widest = 0;
      for (uint32_t i = 0; i < m; i++) {
        widths[i] = kWidths[idx[i]];
        total += eds_bytes(widths[i]);
        widest = std::max(widest, eds_bytes(widths[i]));
      }
      cur_set = set_no;
      const std::vector<BlockIn> in = batch_of(widths, set_no++);
      const uint64_t budgets[4] = {1, widest, total, 0};
      for (uint64_t b : budgets) {
        cur_budget = b;
        chunks += check_plan(in, b);
      }
      sets++;
      // the next multiset
      int32_t i = (int32_t)m - 1;
      while (i >= 0 && idx[i] == 9) i--;
      if (i < 0) break;
      const uint32_t v = idx[i] + 1;
      for (uint32_t j = (uint32_t)i; j < m; j++) idx[j] = v;
    }
    std::printf("n = %u: %llu multisets, %llu chunks\n", m, (unsigned long long)sets, (unsigned long long)chunks);
  }
  // a batch of failed blocks only, and an empty one
  const std::vector<BlockIn> none = {BlockIn{3, -1, 0, 0}, BlockIn{0, 2, 0, 0}};
  CHECK(check_plan(none, 0) == 0);
  CHECK(plan_blocks(nullptr, 0, 0).chunks.empty());
  if (fails) {
    std::printf("block batch plan check: %d FAILED\n", fails);
    return 1;
  }
  std::printf("block batch plan check: ok\n");
  return 0;
}
