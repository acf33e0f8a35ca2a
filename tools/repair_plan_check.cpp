// Stand-alone host check of the repair's planner (celestia-app_amd/csrc/repair_plan.hpp): no
// HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/repair_plan_check.cpp -o repair_plan_check && ./repair_plan_check
// For every width W = 2 .. 256 (one partial word, exactly one word, several words) it takes
// random masks at survival p = 0.3, 0.5, 0.55, 0.7, 0.9 (splitmix64 by cell index, fixed seeds)
// and the structured masks of the GPU tests (one quadrant only, the left half, all but one
// cell, all present), and steps the repair's own pass schedule (SquarePasses: next, apply) over
// each, beside a byte mask on which every solve is applied cell by cell:
// 1. the first-row scan = {i : k <= known cells of row i < W};
// 2. the sanity lists and checks, every pass's direction and list, and after every apply
//    cnt[0], cnt[1], total and both bitsets, against a recount of the byte mask;
// 3. orth[t] = the orthogonal axes whose last missing cell solve t filled, ascending;
// 4. closure: the passes and plan_sweeps end with the same `solved` and the same known cells;
// 5. rollback(hm, W, solves, t) = the byte mask before solve t, for t = 0, the middle, the end.
// Then the order replay on synthetic results: one failing axis of each kind, the earliest of
// two, none, and the same through root records in list order (repair_exact's layout).
// tests/test_repair_plan_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "repair_plan.hpp"

using namespace cel::repair;

static int fails = 0;
static uint32_t cur_w = 0, cur_mask = 0;
#define CHECK(c)                                                                                                   \
  do {                                                                                                             \
    if (!(c)) {                                                                                                    \
      if (fails < 20) std::printf("FAIL %s:%d: %s (W = %u, mask %u)\n", __FILE__, __LINE__, #c, cur_w, cur_mask);  \
      fails++;                                                                                                     \
    }                                                                                                              \
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
constexpr uint32_t kReps = 4;  // random masks per p

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

static uint32_t known(const std::vector<uint8_t>& m, uint32_t W, int is_col, uint32_t i) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < W; j++) c += m[is_col ? (size_t)j * W + i : (size_t)i * W + j] != 0;
  return c;
}

// solve (is_col, i) applied to m cell by cell; the orthogonal axes it completes, ascending
static std::vector<int32_t> apply_solve(std::vector<uint8_t>& m, uint32_t W, int is_col, uint32_t i) {
  std::vector<int32_t> done;
  for (uint32_t j = 0; j < W; j++) {
    uint8_t& cell = m[is_col ? (size_t)j * W + i : (size_t)i * W + j];
    if (cell) continue;
    cell = 1;
    if (known(m, W, !is_col, j) == W) done.push_back((int32_t)j);
  }
  return done;
}

// the same without the recounts
static void fill_axis(std::vector<uint8_t>& m, uint32_t W, int is_col, uint32_t i) {
  for (uint32_t j = 0; j < W; j++) m[is_col ? (size_t)j * W + i : (size_t)i * W + j] = 1;
}

static void check_bits(const MaskBits& mb, const std::vector<uint8_t>& m) {
  const uint32_t W = mb.W;
  uint64_t total = 0;
  CHECK(mb.nw == (W + 63) / 64);
  for (int d = 0; d < 2; d++) {
    CHECK(mb.cnt[d].size() == W && mb.bits[d].size() == (size_t)W * mb.nw);
    for (uint32_t i = 0; i < W; i++) {
      CHECK(mb.cnt[d][i] == known(m, W, d, i));
      for (uint32_t q = 0; q < mb.nw; q++) {
        uint64_t want = 0;  // no bit at or above W
        for (uint32_t j = q * 64; j < W && j < (q + 1) * 64; j++)
          want |= (uint64_t)(m[d ? (size_t)j * W + i : (size_t)i * W + j] != 0) << (j % 64);
        CHECK(mb.bits[d][(size_t)i * mb.nw + q] == want);
      }
    }
  }
  for (uint8_t c : m) total += c != 0;
  CHECK(mb.total == total);
}

struct Counts {
  uint64_t masks, passes, solves;
};

static void check_mask(const std::vector<uint8_t>& hm, uint32_t W, Counts* n) {
  const uint32_t k = W / 2;
  const size_t cells = (size_t)W * W;
  // 1. the first-row scan
  std::vector<int32_t> want_first;
  for (uint32_t i = 0; i < W; i++) {
    const uint32_t c = known(hm, W, 0, i);
    if (c >= k && c < W) want_first.push_back((int32_t)i);
  }
  CHECK(first_row_pass(hm, k) == want_first);
  // 2, 3. the passes: the repair's stepper beside the rounds (rows, then columns) of the byte mask
  SquarePasses sp(hm.data(), k);
  const MaskBits& mb = sp.mb;
  const std::vector<Check>& order = sp.order;
  const std::vector<Solve>& solves = sp.solves;
  std::vector<uint8_t> m(hm);
  check_bits(mb, m);
  // the sanity checks: for i: row i, column i, every complete axis; they open the order
  std::vector<int32_t> want_sanity[2];
  size_t nsanity = 0;
  for (uint32_t i = 0; i < W; i++)
    for (int d = 0; d < 2; d++) {
      if (known(m, W, d, i) != W) continue;
      want_sanity[d].push_back((int32_t)i);
      CHECK(nsanity < order.size() && order[nsanity].kind == Check::SANITY && order[nsanity].is_col == d &&
            order[nsanity].idx == (int32_t)i && order[nsanity].solve == -1);
      nsanity++;
    }
  CHECK(order.size() == nsanity && sp.sanity[0] == want_sanity[0] && sp.sanity[1] == want_sanity[1]);
  std::vector<int32_t> list, got_list, orth;
  int got_col = -1;
  bool solved = false, first = true;
  for (;;) {
    bool progress = false;
    for (int is_col = 0; is_col < 2; is_col++) {
      list.clear();  // from the byte mask; check_bits has compared mb.cnt with it
      for (uint32_t i = 0; i < W; i++) {
        const uint32_t c = known(m, W, is_col, i);
        if (c >= k && c < W) list.push_back((int32_t)i);
      }
      if (first && !is_col) CHECK(list == want_first);  // the pass the repair issues early
      if (list.empty()) continue;  // the stepper skips an empty pass
      first = false;
      const bool stepped = sp.next(&got_col, got_list);
      CHECK(stepped && got_col == is_col && got_list == list);
      if (!stepped) return;
      std::vector<std::vector<int32_t>> want_orth;
      std::vector<int32_t> all_orth;
      for (int32_t i : list) {
        want_orth.push_back(apply_solve(m, W, is_col, (uint32_t)i));
        all_orth.insert(all_orth.end(), want_orth.back().begin(), want_orth.back().end());
      }
      std::sort(all_orth.begin(), all_orth.end());
      const size_t o0 = order.size(), s0 = solves.size();
      sp.apply(orth);
      CHECK(sp.by_solve == want_orth);
      check_bits(mb, m);
      CHECK(orth == all_orth);
      CHECK(solves.size() == s0 + list.size() && order.size() == o0 + list.size() + all_orth.size());
      n->passes++;
      n->solves += list.size();
      progress = true;
    }
    if (mb.total == cells) {
      solved = true;
      break;
    }
    if (!progress) break;
  }
  CHECK(!sp.next(&got_col, got_list) && sp.solved() == solved);
  // the log: every SOLVE names its own solve, followed by its ORTH axes
  for (size_t o = nsanity, s = 0; o < order.size(); o++) {
    if (order[o].kind == Check::SOLVE) {
      CHECK(s < solves.size() && order[o].solve == (int32_t)s && order[o].idx == solves[s].idx &&
            order[o].is_col == solves[s].is_col);
      s++;
    } else {
      CHECK(order[o].kind == Check::ORTH && s > 0 && order[o].solve == (int32_t)s - 1 &&
            order[o].is_col == !solves[s - 1].is_col);
    }
  }
  // 4. closure: rsmt2d's sweeps reach the same cells
  const SweepPlan p = plan_sweeps(hm, k);
  std::vector<uint8_t> ms(hm);
  for (const Solve& s : p.solves) fill_axis(ms, W, s.is_col, (uint32_t)s.idx);
  CHECK(p.solved == solved);
  CHECK(ms == m);
  for (int d = 0; d < 2; d++)
    for (uint32_t i = 0; i < W; i++) CHECK(p.cnt[d][i] == known(ms, W, d, i));
  CHECK(p.level.size() == p.solves.size());
  // 5. rollback
  const size_t S = solves.size();
  for (size_t t : {(size_t)0, S / 2, S}) {
    std::vector<uint8_t> want(hm), got(hm);
    for (size_t u = 0; u < t; u++) fill_axis(want, W, solves[u].is_col, (uint32_t)solves[u].idx);
    rollback(got, W, solves, t);
    CHECK(got == want);
  }
  n->masks++;
}

// The order replay over synthetic results at width W: order = SANITY row 0, SANITY column 1,
// SOLVE row 2, ORTH column 3, SOLVE column 4, ORTH row 5.
static void check_replay() {
  const uint32_t W = 8;
  cur_w = W;
  cur_mask = 0;
  const std::vector<Check> order = {{Check::SANITY, 0, 0, -1}, {Check::SANITY, 1, 1, -1}, {Check::SOLVE, 0, 2, 0},
                                    {Check::ORTH, 1, 3, 0},    {Check::SOLVE, 1, 4, 1},   {Check::ORTH, 0, 5, 1}};
  std::vector<uint8_t> exp_r((size_t)W * kRoot), exp_c((size_t)W * kRoot);
  for (size_t i = 0; i < exp_r.size(); i++) {
    exp_r[i] = (uint8_t)(i * 7 + 1);
    exp_c[i] = (uint8_t)(i * 13 + 5);
  }
  const uint8_t* const exp[2] = {exp_r.data(), exp_c.data()};
  struct Bad {
    long at;  // index into order, -1: none
    bool root;
  };
  struct Case {
    Bad a, b;
    long want;
    cel_status code;
  };
  const Case cases[] = {
      {{-1, false}, {-1, false}, -1, CEL_OK},
      {{0, true}, {-1, false}, 0, CEL_EBADROOT},
      {{1, false}, {-1, false}, 1, CEL_EBYZANTINE},
      {{2, true}, {-1, false}, 2, CEL_EBYZANTINE},
      {{2, false}, {-1, false}, 2, CEL_EBYZANTINE},
      {{3, true}, {-1, false}, 3, CEL_EBYZANTINE},
      {{3, false}, {-1, false}, 3, CEL_EBYZANTINE},
      {{4, true}, {-1, false}, 4, CEL_EBYZANTINE},
      {{5, false}, {-1, false}, 5, CEL_EBYZANTINE},
      {{5, false}, {1, true}, 1, CEL_EBADROOT},    // the earlier one wins, with its own status
      {{1, true}, {0, false}, 0, CEL_EBYZANTINE},  // a complete axis with a set flag is byzantine
      {{4, true}, {2, false}, 2, CEL_EBYZANTINE},
  };
  for (const Case& cs : cases) {
    cur_mask++;
    std::vector<uint8_t> got((size_t)2 * W * kRoot);
    std::memcpy(got.data(), exp_r.data(), exp_r.size());
    std::memcpy(got.data() + exp_r.size(), exp_c.data(), exp_c.size());
    std::vector<int32_t> flags((size_t)2 * W, 0);
    // an axis outside the order may fail as it likes: row 7's flag, column 6's root
    flags[7] = 1;
    got[((size_t)W + 6) * kRoot + kRoot - 1] ^= 0x80;
    for (const Bad& bad : {cs.a, cs.b}) {
      if (bad.at < 0) continue;
      const Check& c = order[(size_t)bad.at];
      if (bad.root) got[((size_t)c.is_col * W + c.idx) * kRoot + (size_t)bad.at] ^= 1;
      else flags[(size_t)c.is_col * W + c.idx] = 1;
    }
    cel_status code = CEL_OK;
    CHECK(first_failure(order.data(), order.size(), {got.data(), kRoot, RootRecords::BY_AXIS}, exp, flags.data(), W, &code) == cs.want);
    if (cs.want >= 0) CHECK(code == cs.code);
    // the same results as root records of 96 bytes in list order, by direction, and only the
    // SOLVE / ORTH tail of the order: where repair_exact finds them
    std::vector<uint8_t> rec((size_t)2 * W * 96, 0xEE);
    size_t pos[2] = {0, 0};
    for (size_t o = 2; o < order.size(); o++) {
      const Check& c = order[o];
      std::memcpy(rec.data() + ((size_t)c.is_col * W + pos[c.is_col]++) * 96,
                  got.data() + ((size_t)c.is_col * W + c.idx) * kRoot, kRoot);
    }
    long want_tail = -1;
    for (const Bad& bad : {cs.a, cs.b})
      if (bad.at >= 2 && (want_tail < 0 || bad.at - 2 < want_tail)) want_tail = bad.at - 2;
    code = CEL_OK;
    const long f = first_failure(order.data() + 2, order.size() - 2, {rec.data(), 96, RootRecords::BY_RANK}, exp, flags.data(),
                                 W, &code);
    CHECK(f == want_tail);
    if (want_tail >= 0) CHECK(code == CEL_EBYZANTINE);
  }
  // normalise_mask: any non-zero byte is a present cell
  const uint8_t raw[6] = {0, 1, 2, 0x80, 0, 0xFF};
  CHECK(normalise_mask(raw, 6) == (std::vector<uint8_t>{0, 1, 1, 1, 0, 1}));
}

int main() {
  for (uint32_t W = 2; W <= 256; W *= 2) {
    Counts n{0, 0, 0};
    cur_w = W;
    cur_mask = 0;
    for (const std::vector<uint8_t>& m : masks_of(W)) {
      check_mask(m, W, &n);
      cur_mask++;
    }
    std::printf("W = %3u: %llu masks, %llu passes, %llu solves\n", W, (unsigned long long)n.masks,
                (unsigned long long)n.passes, (unsigned long long)n.solves);
  }
  check_replay();
  std::printf("repair plan check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
