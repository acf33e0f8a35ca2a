// Stand-alone host check of the blob commitment planner (celestia-app_amd/csrc/blob_plan.hpp):
// no HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/blob_plan_check.cpp -o blob_plan_check && ./blob_plan_check
// It plans batches of the sizes the tests use at several thresholds and checks, per blob,
// that the slot layout and the per-slot root rule agree with MerkleMountainRangeSizes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blob_plan.hpp"

using namespace cel::blob;

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      fails++;                                                      \
    }                                                               \
  } while (0)

static uint64_t len_for(uint32_t n) { return kSparseFirst + (uint64_t)kSparseCont * (n - 1); }

static void check_batch(const std::vector<uint64_t>& lens, uint32_t threshold) {
  Plan p;
  uint8_t ns[29] = {0};
  uint64_t off = 3;  // an odd base, as in a caller's buffer
  for (uint64_t len : lens) {
    plan_add(p, ns, off, len, threshold);
    off += len;
  }
  const uint64_t slots = (p.slots + kTile - 1) / kTile * kTile;
  std::vector<uint32_t> table(slots);  // exactly what the planner may write
  plan_finish(p, table.data());
  CHECK(p.slots == slots && slots % kTile == 0 && slots <= kMaxSlots);
  uint64_t roots = 0, prev_end = 0;
  for (size_t b = 0; b < p.recs.size(); b++) {
    const Rec& r = p.recs[b];
    const uint32_t w = 1u << r.wlog;
    CHECK(r.n == sparse_shares_needed(r.len) && w == subtree_width(r.n, threshold) && w <= 1024);
    CHECK(r.first % w == 0 && r.first >= prev_end && (uint64_t)r.first + r.n <= slots);
    CHECK(r.root0 == roots);
    prev_end = (uint64_t)r.first + r.n;
    std::vector<uint32_t> mmr;
    mountain_range(r.n, w, mmr);
    CHECK(mmr.size() == r.nroots && r.nroots == root_count(r.n, w));
    // walk the mountain range and the per-slot rule side by side
    uint32_t s = 0, seen = 0;
    for (size_t i = 0; i < mmr.size(); i++) {
      uint32_t index = ~0u, level = ~0u;
      CHECK(root_at(r.n, r.wlog, s, &index, &level));
      CHECK(index == i && (1u << level) == mmr[i]);
      CHECK(s % mmr[i] == 0);                                  // aligned to its own size
      CHECK(mmr[i] > kTile || (r.first + s) / kTile == (r.first + s + mmr[i] - 1) / kTile);  // no straddle
      s += mmr[i];
    }
    CHECK(s == r.n);
    for (uint32_t q = 0; q < r.n; q++) {
      uint32_t index, level;
      if (root_at(r.n, r.wlog, q, &index, &level)) seen++;
      CHECK(table[r.first + q] == b);
    }
    CHECK(seen == r.nroots);
    roots += r.nroots;
  }
  CHECK(roots == p.roots);
  uint64_t owned = 0;
  for (uint32_t v : table) owned += v != kNoBlob;
  uint64_t shares = 0;
  for (const Rec& r : p.recs) shares += r.n;
  CHECK(owned == shares && slots <= 2 * shares + kTile);
}

int main() {
  const uint32_t counts[] = {63, 64, 65, 267, 352, 1031, 16384, 70000};
  const uint32_t thresholds[] = {1, 8, 64, 4096};
  std::vector<uint64_t> lens = {1, 478, 479, 960, 961};
  for (uint32_t n : counts) lens.push_back(len_for(n));
  for (uint32_t t : thresholds) {
    check_batch(lens, t);
    for (uint64_t len : lens) check_batch({len}, t);
  }
  check_batch({len_for(3000)}, 4096);
  check_batch({len_for(kMaxShares)}, 64);
  check_batch({len_for(kMaxShares), 1, len_for(kMaxShares - 1)}, 1);
  std::vector<uint64_t> many;
  uint64_t x = 12345;
  for (int i = 0; i < 3000; i++) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    many.push_back(1 + (x >> 33) % 40000);
  }
  check_batch(many, 64);
  check_batch(many, 2);
  std::printf(fails ? "blob plan check: %d failures\n" : "blob plan check: ok\n", fails);
  return fails ? 1 : 0;
}
