// Stand-alone host check of the batched prover's arithmetic
// (celestia-app_amd/csrc/nmt_prove.hpp): no HIP, no device. Build it with a host compiler,
// optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/prove_select_check.cpp -o prove_select_check && ./prove_select_check
// 1. For every width 2k = 2 .. 256 and every range [s, e) of it, the closed form (node_count,
//    node_at) against the recursion of nmt's buildRangeProof as proof.cpp states it (collect,
//    copied below): the same nodes, in the same order, by level and position.
// 2. For k = 1, 2, 4 .. 512 the index layout: level 0 starts at byte 0, every level starts
//    where the one before ends, the tail follows the last level and ends at the index's size,
//    every part 16-byte aligned. For k <= 32 every (axis, tree, level, position) is also mapped
//    through index_record into a table of exactly the record count: every leaf record is
//    named twice (by its row and by its column), every other record once, none outside.
// tests/test_prove_select.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "nmt_prove.hpp"

using namespace cel::prove;

static int fails = 0;
#define CHECK(c)                                                                                   \
  do {                                                                                             \
    if (!(c)) {                                                                                    \
      if (fails < 20) std::printf("FAIL %s:%d: %s (W = %u, s = %u, e = %u)\n", __FILE__, __LINE__, #c, W, s, e); \
      fails++;                                                                                     \
    }                                                                                              \
  } while (0)

// proof.cpp's collect with (level, position) in place of the node's offset: left to right, the
// roots of the maximal subtrees of [start, end) that do not overlap [ps, pe).
static void collect(uint32_t start, uint32_t end, uint32_t ps, uint32_t pe, std::vector<NodeAt>& out) {
  if (end <= ps || start >= pe) {
    uint32_t level = 0;
    while ((1u << level) < end - start) level++;
    out.push_back(NodeAt{level, start >> level});
    return;
  }
  if (end - start == 1) return;  // a leaf inside the range
  const uint32_t half = (end - start) / 2;
  collect(start, start + half, ps, pe, out);
  collect(start + half, end, ps, pe, out);
}

static uint64_t check_selection(uint32_t W) {
  uint32_t L = 0, s = 0, e = 0;
  while ((1u << L) < W) L++;
  uint64_t nodes = 0;
  std::vector<NodeAt> want;
  for (s = 0; s < W; s++)
    for (e = s + 1; e <= W; e++) {
      want.clear();
      collect(0, W, s, e, want);
      const uint32_t n = node_count(L, s, e - 1);
      CHECK(n == want.size());
      CHECK(n <= 2 * L);
      for (uint32_t j = 0; j < n && j < want.size(); j++) {
        const NodeAt a = node_at(L, s, e - 1, j);
        CHECK(a.level == want[j].level && a.pos == want[j].pos);
        CHECK(a.level < L && a.pos < (W >> a.level));
      }
      const NodeAt past = node_at(L, s, e - 1, n);
      CHECK(past.level == L);
      nodes += n;
    }
  return nodes;
}

static void check_layout(uint32_t k) {
  const IndexLayout x = index_layout(k);
  const uint32_t W = 2 * k, s = 0, e = 0;
  CHECK(x.W == W && (1u << x.L) == W);
  CHECK(x.level_off[0] == 0);
  uint64_t at = (uint64_t)W * W * kRecordBytes;  // the leaves, once
  for (uint32_t l = 1; l <= x.L; l++) {
    CHECK(x.level_off[l] == at);
    CHECK(x.level_off[l] % 16 == 0);
    at += (uint64_t)2 * W * (W >> l) * kRecordBytes;
  }
  CHECK(x.records * kRecordBytes == at);
  CHECK(index_level_rec(W, x.L + 1) == x.records);
  CHECK(x.leafd_off == at && x.leafd_off % 16 == 0);
  CHECK(x.dah_off == x.leafd_off + (uint64_t)2 * W * 32);
  CHECK(x.bad_off == x.dah_off + 32 && x.status_off == x.bad_off + 4);
  CHECK(x.bytes >= x.status_off + 4 && x.bytes < x.status_off + 4 + 16 && x.bytes % 16 == 0);
  if (k > 32) return;
  std::vector<uint8_t> seen(x.records, 0);  // exactly the records: one outside is a write out of bounds
  for (uint32_t axis = 0; axis < 2; axis++)
    for (uint32_t t = 0; t < W; t++)
      for (uint32_t l = 0; l <= x.L; l++)
        for (uint32_t p = 0; p < (W >> l); p++) {
          const uint64_t r = index_record(W, axis, t, l, p);
          CHECK(r < x.records);
          CHECK(r * kRecordBytes >= x.level_off[l]);
          CHECK(l == x.L ? r < x.records : r * kRecordBytes < x.level_off[l + 1]);
          if (r < x.records) seen[r]++;
        }
  for (uint64_t r = 0; r < x.records; r++) CHECK(seen[r] == (r < (uint64_t)W * W ? 2 : 1));
  // a row's leaf c and a column's leaf r are the same record: cell (r, c)
  for (uint32_t r = 0; r < W; r++)
    for (uint32_t c = 0; c < W; c++) CHECK(index_record(W, 0, r, 0, c) == index_record(W, 1, c, 0, r));
}

int main() {
  for (uint32_t W = 2; W <= 256; W *= 2) {
    const uint64_t nodes = check_selection(W);
    std::printf("W = %3u: %5u ranges, %7llu proof nodes\n", W, W * (W + 1) / 2, (unsigned long long)nodes);
  }
  for (uint32_t k = 1; k <= 512; k *= 2) {
    check_layout(k);
    const IndexLayout x = index_layout(k);
    std::printf("k = %3u: %8llu records in %2u levels, %10llu bytes\n", k, (unsigned long long)x.records, x.L + 1,
                (unsigned long long)x.bytes);
  }
  std::printf("prove select check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
