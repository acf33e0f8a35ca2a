// Stand-alone host check of the blob commitment planner (celestia-app_amd/csrc/blob_plan.hpp):
// no HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/blob_plan_check.cpp -o blob_plan_check && ./blob_plan_check
// It plans batches of the sizes the tests use at several thresholds and checks, per blob,
// that the slot layout and the per-slot root rule agree with MerkleMountainRangeSizes.
// tests/test_blob_plan_check.py builds and runs it, plain and under ASan + UBSan.
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

static Plan check_batch(const std::vector<uint64_t>& lens, uint32_t threshold) {
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
  return p;
}

// The bottom-up RFC-6962 level sizes of k_blob_commit's global-memory loop (an unpaired last
// node moves up) from count down to the first that fits its LDS (1024 digests).
static std::vector<uint32_t> rfc_levels(uint32_t count) {
  std::vector<uint32_t> v = {count};
  while (v.back() > 1024) v.push_back((v.back() + 1) / 2);
  return v;
}

// The shapes tests/test_gpu_commitment_shapes.py and tests/test_gpu_block_shapes.py rely on.
static void check_test_shapes() {
  using V = std::vector<uint32_t>;
  // widths 1024 and 256 at threshold 64, their root counts and tails
  const uint64_t wide = len_for(264001) - 7, mid = len_for(20037) - 3;
  Plan p = check_batch({wide}, 64);
  CHECK(p.recs[0].n == 264001 && p.recs[0].wlog == 10 && p.recs[0].nroots == 261 && p.max_wlog == 10);
  V mmr;
  mountain_range(264001, 1024, mmr);
  CHECK(mmr.size() == 261 && V(mmr.begin() + 257, mmr.end()) == (V{512, 256, 64, 1}));
  p = check_batch({mid}, 64);
  CHECK(p.recs[0].n == 20037 && p.recs[0].wlog == 8 && p.recs[0].nroots == 81 && p.max_wlog == 8);
  mountain_range(20037, 256, mmr);
  CHECK(V(mmr.begin() + 78, mmr.end()) == (V{64, 4, 1}));
  // the width-1024 blob between small ones, whole (the device entry) and as the host entry's
  // three chunks of at most 64 MiB
  p = check_batch({1000, wide, 5000, 3u << 20, mid}, 64);
  CHECK(p.max_wlog == 10 && p.recs[1].first % 1024 == 0 && p.recs[1].first > 0 && p.recs[2].first > p.recs[1].first);
  CHECK(1000 + wide > (64ull << 20) && 5000 + (3ull << 20) + mid <= (64ull << 20));
  check_batch({1000}, 64);
  check_batch({5000, 3u << 20, mid}, 64);
  // 70000 shares inside the k = 512 block: width 512
  p = check_batch({len_for(70000) - 7, 1u << 20, 1u << 20}, 64);
  CHECK(p.recs[0].wlog == 9 && p.recs[1].n == 2176);
  // width 1 at threshold 2^20: one root per share, on both sides of the 128 / 129 switch of
  // the commit block and of the 1024 digests its LDS holds
  const V a = {1, 2, 3, 5, 7, 127, 128}, b = {129, 1023, 1024, 1025, 2049, 2051, 3000};
  for (const V* counts : {&a, &b}) {
    std::vector<uint64_t> lens;
    for (uint32_t n : *counts) lens.push_back(len_for(n) - (n > 1 ? 481 : 0));
    p = check_batch(lens, 1u << 20);
    for (size_t i = 0; i < counts->size(); i++) CHECK(p.recs[i].wlog == 0 && p.recs[i].nroots == (*counts)[i]);
    uint64_t shares = 0;
    for (uint32_t n : *counts) shares += n;
    CHECK(p.max_wlog == 0 && p.max_roots == counts->back() && p.roots == shares);
  }
  CHECK(rfc_levels(1024) == (V{1024}) && rfc_levels(1025) == (V{1025, 513}));
  CHECK(rfc_levels(2049) == (V{2049, 1025, 513}) && rfc_levels(2051) == (V{2051, 1026, 513}));
  CHECK(rfc_levels(3000) == (V{3000, 1500, 750}));
  // a random batch shaped like the tests' mixed one: about 120 share counts log-uniform in
  // 1..3000 (a power of two times a uniform factor), three of 5000..20000, one above 16384
  std::vector<uint64_t> mixed;
  uint64_t x = 2024;
  auto next = [&x](uint64_t m) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (x >> 33) % m;
  };
  for (int i = 0; i < 120; i++) {
    const uint32_t e = (uint32_t)next(12), n = (1u << e) + (uint32_t)next(1u << e);
    mixed.push_back(len_for(n < 3000 ? n : 3000) - next(478));
  }
  mixed.insert(mixed.begin() + 40, len_for(5000 + (uint32_t)next(11385)) - next(478));
  mixed.insert(mixed.begin() + 80, len_for(16385 + (uint32_t)next(3616)) - next(478));
  mixed.push_back(len_for(5000 + (uint32_t)next(11385)) - next(478));
  for (uint32_t t : {1u, 5u, 64u, 1000u}) {
    p = check_batch(mixed, t);
    if (t == 1) CHECK(p.max_wlog == 8);
  }
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
  check_batch(many, 5);
  check_batch(many, 1000);
  check_test_shapes();
  std::printf(fails ? "blob plan check: %d failures\n" : "blob plan check: ok\n", fails);
  return fails ? 1 : 0;
}
