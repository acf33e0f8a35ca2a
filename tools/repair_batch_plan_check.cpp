// Stand-alone host check of the batch repair's planner (celestia-app_amd/csrc/repair_plan.hpp,
// BatchPasses): no HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/repair_batch_plan_check.cpp -o repair_batch_plan_check && ./repair_batch_plan_check
// For every width W = 2 .. 256 it takes the masks of tools/repair_plan_check.cpp (random at
// survival p = 0.3 .. 0.9 by splitmix64, one quadrant, the left half, all but one cell, all
// present) in batches of five and merges their pass schedules as cel_dev_repair_batch does:
// 1. the early pass: first_row_pass_batch = every square's rows with k <= known cells < W, and
//    the first merged pass is that list whenever it is not empty;
// 2. every entry names a square below n and an axis below W, and no (square, direction, axis)
//    is listed twice;
// 3. each square's projection of the merged passes (direction, axes, completed orthogonal
//    axes) is its own schedule, taken from a byte mask filled cell by cell; a complete square
//    and one stuck at the start are in no pass;
// 4. each square's check order and solve log are those of the square stepped alone (its own
//    SquarePasses, as the single repair steps it; tools/repair_plan_check.cpp checks that one
//    against the byte mask), and rollback over its own log gives the byte mask before solve t
//    for t = 0, the middle, the end;
// 5. the verdicts over synthetic results in the batch's layout ([n][W] row roots, [n][W] column
//    roots, flags [n][2][W]): one square fails (a root, or a flag) at a check of its order, the
//    others pass, for every choice of the failing square.
// tests/test_repair_batch_plan_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "repair_plan.hpp"

using namespace cel::repair;

static int fails = 0;
static uint32_t cur_w = 0, cur_batch = 0;
#define CHECK(c)                                                                                                    \
  do {                                                                                                              \
    if (!(c)) {                                                                                                     \
      if (fails < 20) std::printf("FAIL %s:%d: %s (W = %u, batch %u)\n", __FILE__, __LINE__, #c, cur_w, cur_batch); \
      fails++;                                                                                                      \
    }                                                                                                               \
  } while (0)

// cell c of the random mask `seed` survives with probability p (counter-based splitmix64)
static bool survives(uint64_t seed, uint64_t c, double p) {
  uint64_t x = seed + (c + 1) * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double)(x >> 11) * (1.0 / 9007199254740992.0) < p;
}

static const double kP[] = {0.3, 0.5, 0.55, 0.7, 0.9};
constexpr uint32_t kReps = 4;   // random masks per p
constexpr uint32_t kBatch = 5;  // squares per batch

static std::vector<std::vector<uint8_t>> masks_of(uint32_t W) {
  const uint32_t k = W / 2;
  const size_t cells = (size_t)W * W;
  std::vector<std::vector<uint8_t>> out;
  for (uint32_t pi = 0; pi < 5; pi++)
    for (uint32_t rep = 0; rep < kReps; rep++) {
      std::vector<uint8_t> m(cells);
      const uint64_t seed = 0xC0FFEEull + (uint64_t)W * 1000 + pi * 10 + rep;
      for (size_t c = 0; c < cells; c++) m[c] = survives(seed, c, kP[pi]);
      out.push_back(m);
    }
  std::vector<uint8_t> quad(cells, 0), left(cells, 0), but_one(cells, 1), all(cells, 1);
  for (uint32_t i = 0; i < W; i++)
    for (uint32_t j = 0; j < k; j++) {
      left[(size_t)i * W + j] = 1;
      if (i < k) quad[(size_t)i * W + j] = 1;
    }
  but_one[(size_t)(W - 1) * W + k] = 0;
  out.push_back(quad);
  out.push_back(left);
  out.push_back(but_one);
  out.push_back(all);
  return out;
}

// Batch b of the 24 masks: five of them at stride 5 from b (random ones of every p beside the
// structured ones, the all-present mask in batch 3, a p = 0.3 mask stuck at the start in most).
static std::vector<uint32_t> batch_of(uint32_t b, uint32_t nmasks) {
  std::vector<uint32_t> ids;
  for (uint32_t j = 0; j < kBatch; j++) ids.push_back((b + 5 * j) % nmasks);
  return ids;
}

static uint32_t known(const uint8_t* m, uint32_t W, int is_col, uint32_t i) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < W; j++) c += m[is_col ? (size_t)j * W + i : (size_t)i * W + j] != 0;
  return c;
}

// solve (is_col, i) applied to m cell by cell; the orthogonal axes it completes go into done
static void apply_solve(uint8_t* m, uint32_t W, int is_col, uint32_t i, std::vector<int32_t>& done) {
  for (uint32_t j = 0; j < W; j++) {
    uint8_t& cell = m[is_col ? (size_t)j * W + i : (size_t)i * W + j];
    if (cell) continue;
    cell = 1;
    if (known(m, W, !is_col, j) == W) done.push_back((int32_t)j);
  }
}

// A square's own schedule from the byte mask: passes of (direction, axes, orthogonal axes
// completed, ascending), rows then columns until solved or stuck.
struct OwnPass {
  int is_col;
  std::vector<int32_t> list, orth;
  bool operator==(const OwnPass& o) const { return is_col == o.is_col && list == o.list && orth == o.orth; }
};
static std::vector<OwnPass> own_schedule(std::vector<uint8_t> m, uint32_t W) {
  const uint32_t k = W / 2;
  std::vector<OwnPass> out;
  for (;;) {
    bool progress = false;
    for (int is_col = 0; is_col < 2; is_col++) {
      OwnPass p{is_col, {}, {}};
      for (uint32_t i = 0; i < W; i++) {
        const uint32_t c = known(m.data(), W, is_col, i);
        if (c >= k && c < W) p.list.push_back((int32_t)i);
      }
      if (p.list.empty()) continue;
      for (int32_t i : p.list) apply_solve(m.data(), W, is_col, (uint32_t)i, p.orth);
      std::sort(p.orth.begin(), p.orth.end());
      out.push_back(p);
      progress = true;
    }
    if (!progress) break;
  }
  return out;
}

// The square alone, stepped as the single repair steps it: the check order and the solve log.
static SquarePasses single_logs(const std::vector<uint8_t>& hm, uint32_t W) {
  SquarePasses sp(hm.data(), W / 2);
  std::vector<int32_t> list, orth;
  int is_col;
  while (sp.next(&is_col, list)) sp.apply(orth);
  return sp;
}

static bool same(const std::vector<Check>& a, const std::vector<Check>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].kind != b[i].kind || a[i].is_col != b[i].is_col || a[i].idx != b[i].idx || a[i].solve != b[i].solve) return false;
  return true;
}

struct Counts {
  uint64_t batches, passes, entries;
};

static void check_batch(const std::vector<std::vector<uint8_t>>& all, const std::vector<uint32_t>& ids, uint32_t W, Counts* cn) {
  const uint32_t k = W / 2, n = (uint32_t)ids.size();
  const size_t cells = (size_t)W * W;
  std::vector<uint8_t> masks;
  for (uint32_t id : ids) masks.insert(masks.end(), all[id].begin(), all[id].end());
  CHECK(entries_fit(n, W));
  // 1. the early pass
  std::vector<int32_t> want_first;
  for (uint32_t q = 0; q < n; q++)
    for (uint32_t i = 0; i < W; i++) {
      const uint32_t c = known(masks.data() + q * cells, W, 0, i);
      if (c >= k && c < W) want_first.push_back(pack_entry(q, i, 0));
    }
  const std::vector<int32_t> first = first_row_pass_batch(masks, n, k);
  CHECK(first == want_first);
  BatchPasses bp(masks, n, k);
  const std::vector<BatchPass> passes = plan_batch(bp);
  if (!first.empty()) CHECK(!passes.empty() && passes[0].is_col == 0 && passes[0].entries == first);
  else CHECK(passes.empty() || passes[0].is_col == 1);
  // 2. the entries, and 3. the projections
  std::set<std::tuple<uint32_t, int, uint32_t>> seen;
  std::vector<std::vector<OwnPass>> proj(n);
  for (const BatchPass& p : passes) {
    CHECK(!p.entries.empty());
    for (size_t t = 0; t < p.entries.size(); t++) {
      const int32_t e = p.entries[t];
      const uint32_t q = entry_square(e), ax = entry_axis(e);
      CHECK(q < n && ax < W && entry_is_col(e) == p.is_col);
      if (q >= n) continue;
      CHECK(seen.insert({q, p.is_col, ax}).second);
      if (t > 0) CHECK(p.entries[t - 1] < e);  // squares ascending, a square's axes ascending
    }
  }
  for (size_t pi = 0; pi < passes.size(); pi++) {
    const BatchPass& p = passes[pi];
    std::vector<OwnPass> part(n, OwnPass{p.is_col, {}, {}});
    for (int32_t e : p.entries)
      if (entry_square(e) < n) part[entry_square(e)].list.push_back((int32_t)entry_axis(e));
    for (int32_t e : p.orth) {
      CHECK(entry_square(e) < n && entry_axis(e) < W && entry_is_col(e) == !p.is_col);
      if (entry_square(e) < n) part[entry_square(e)].orth.push_back((int32_t)entry_axis(e));
    }
    for (uint32_t q = 0; q < n; q++) {
      if (part[q].list.empty()) CHECK(part[q].orth.empty());  // only a square in the pass completes axes
      else proj[q].push_back(part[q]);
    }
    cn->entries += p.entries.size();
  }
  cn->passes += passes.size();
  for (uint32_t q = 0; q < n; q++) {
    const std::vector<uint8_t> hm(masks.begin() + (ptrdiff_t)(q * cells), masks.begin() + (ptrdiff_t)((q + 1) * cells));
    const std::vector<OwnPass> own = own_schedule(hm, W);
    CHECK(proj[q] == own);
    // complete, or stuck at the start: in no pass
    bool any_solvable = false;
    for (int d = 0; d < 2; d++)
      for (uint32_t i = 0; i < W; i++) {
        const uint32_t c = known(hm.data(), W, d, i);
        any_solvable |= c >= k && c < W;
      }
    if (!any_solvable) CHECK(proj[q].empty());
    // 4. the logs and the rollback
    const SquarePasses alone = single_logs(hm, W);
    const std::vector<Check>& order = alone.order;
    const std::vector<Solve>& solves = alone.solves;
    const SquarePasses& sq = bp.sq[q];
    CHECK(sq.sanity[0] == alone.sanity[0] && sq.sanity[1] == alone.sanity[1]);
    CHECK(same(sq.order, order));
    CHECK(sq.solves.size() == solves.size());
    for (size_t t = 0; t < solves.size() && t < sq.solves.size(); t++)
      CHECK(sq.solves[t].is_col == solves[t].is_col && sq.solves[t].idx == solves[t].idx);
    std::vector<uint8_t> end(hm);
    for (const Solve& s : sq.solves)
      for (uint32_t j = 0; j < W; j++) end[s.is_col ? (size_t)j * W + (uint32_t)s.idx : (size_t)s.idx * W + j] = 1;
    size_t tot = 0;
    for (uint8_t c : end) tot += c;
    CHECK(sq.solved() == (tot == cells));
    const size_t S = sq.solves.size();
    for (size_t t : {(size_t)0, S / 2, S}) {
      std::vector<uint8_t> want(hm), got(hm);
      for (size_t u = 0; u < t; u++)
        for (uint32_t j = 0; j < W; j++)
          want[sq.solves[u].is_col ? (size_t)j * W + (uint32_t)sq.solves[u].idx : (size_t)sq.solves[u].idx * W + j] = 1;
      rollback(got, W, sq.solves, t);
      CHECK(got == want);
    }
  }
  // 5. the verdicts: square `bad` fails at the middle check of its order (root for even `bad`,
  // flag for odd; an axis is checked once), every other square passes
  std::vector<uint8_t> exp_r((size_t)n * W * kRoot), exp_c((size_t)n * W * kRoot);
  for (size_t i = 0; i < exp_r.size(); i++) {
    exp_r[i] = (uint8_t)(i * 7 + 1);
    exp_c[i] = (uint8_t)(i * 13 + 5);
  }
  for (uint32_t bad = 0; bad < n; bad++) {
    const std::vector<Check>& border = bp.sq[bad].order;
    std::vector<uint8_t> got_all(exp_r);
    got_all.insert(got_all.end(), exp_c.begin(), exp_c.end());
    std::vector<int32_t> flags((size_t)n * 2 * W, 0);
    long want = -1;
    cel_status want_code = CEL_OK;
    if (!border.empty()) {
      want = (long)(border.size() / 2);
      const Check& c = border[(size_t)want];
      if (bad % 2 == 0) got_all[(((size_t)c.is_col * n + bad) * W + (size_t)c.idx) * kRoot + 3] ^= 0x40;
      else flags[((size_t)bad * 2 + (size_t)c.is_col) * W + (size_t)c.idx] = 1;
      want_code = bad % 2 == 0 && c.kind == Check::SANITY ? CEL_EBADROOT : CEL_EBYZANTINE;
    }
    std::vector<uint8_t> got(2 * (size_t)W * kRoot);
    for (uint32_t q = 0; q < n; q++) {
      square_roots(got_all.data(), n, W, q, got.data());
      const uint8_t* const exp[2] = {exp_r.data() + (size_t)q * W * kRoot, exp_c.data() + (size_t)q * W * kRoot};
      cel_status code = CEL_OK;
      const long f = first_failure(bp.sq[q].order.data(), bp.sq[q].order.size(), {got.data(), kRoot, RootRecords::BY_AXIS},
                                   exp, flags.data() + (size_t)q * 2 * W, W, &code);
      if (q == bad) {
        CHECK(f == want);
        if (want >= 0) CHECK(code == want_code);
      } else {
        CHECK(f == -1);
      }
    }
  }
  cn->batches++;
}

int main() {
  for (uint32_t W = 2; W <= 256; W *= 2) {
    Counts cn{0, 0, 0};
    cur_w = W;
    const std::vector<std::vector<uint8_t>> all = masks_of(W);
    for (uint32_t b = 0; b < 5; b++) {
      cur_batch = b;
      check_batch(all, batch_of(b, (uint32_t)all.size()), W, &cn);
    }
    std::printf("W = %3u: %llu batches, %llu passes, %llu entries\n", W, (unsigned long long)cn.batches,
                (unsigned long long)cn.passes, (unsigned long long)cn.entries);
  }
  std::printf("repair batch plan check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
