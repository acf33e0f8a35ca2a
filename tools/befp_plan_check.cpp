// Stand-alone host check of the fraud proofs' planner (celestia-app_amd/csrc/befp_plan.hpp): no
// HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/befp_plan_check.cpp -o befp_plan_check && ./befp_plan_check
// For every width W = 2 .. 64 (k = W / 2):
// 1. classify: every MALFORMED cause alone (axis, index, position, entry axis, a repeated
//    position, more than W entries in a buffer of exactly W + 1), TOO_FEW at k - 1 entries and
//    not at k, and the order of the rule (malformed before too few);
// 2. entry_at: the cell lies on the accused axis and the (root, leaf) pair addresses that cell;
// 3. plan_verify over a batch that mixes every outcome with empty proofs, node counts that
//    differ per entry and offsets that do not start at zero: verdicts, the live list and the
//    packed entry / node offsets against sums taken here; decreasing offsets are refused;
// 4. select_positions over the masks of tools/repair_plan_check.cpp (random at five survival
//    rates, one quadrant, the left half, all but one cell, all present) for six accused axes: a
//    known cell with a complete orthogonal axis is taken, any other position is not;
// 5. proof_records against nmt ProveRange walked recursively, and compact_entries.
// tests/test_befp_plan_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <cstring>
#include <vector>

#include "befp_plan.hpp"

using namespace cel::befp;

static int fails = 0;
static uint32_t cur_w = 0;
#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      if (fails < 20) std::printf("FAIL %s:%d: %s (W = %u)\n", __FILE__, __LINE__, #c, cur_w); \
      fails++;                                                                                \
    }                                                                                         \
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
constexpr uint32_t kReps = 4;

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

// k good entries: positions 0 .. ne - 1, alternating entry axes
static void good_entries(uint32_t ne, std::vector<uint32_t>* pos, std::vector<uint8_t>* ea) {
  pos->resize(ne + 1);  // never empty: data() is a valid pointer
  ea->resize(ne + 1);
  for (uint32_t e = 0; e < ne; e++) {
    (*pos)[e] = e;
    (*ea)[e] = e & 1;
  }
}

static void check_classify(uint32_t W) {
  const uint32_t k = W / 2;
  std::vector<uint32_t> pos;
  std::vector<uint8_t> ea;
  good_entries(k, &pos, &ea);
  CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kDevice);
  CHECK(classify(k, 1, W - 1, pos.data(), ea.data(), k) == kDevice);
  CHECK(classify(k, 0, 0, pos.data(), ea.data(), k - 1) == kTooFew);
  CHECK(classify(k, 0, 0, pos.data(), ea.data(), 0) == kTooFew);
  CHECK(classify(k, 2, 0, pos.data(), ea.data(), k) == kMalformed);
  CHECK(classify(k, 0xFF, 0, pos.data(), ea.data(), k) == kMalformed);
  CHECK(classify(k, 0, W, pos.data(), ea.data(), k) == kMalformed);
  CHECK(classify(k, 1, 0xFFFFFFFFu, pos.data(), ea.data(), k) == kMalformed);
  CHECK(classify(k, 2, 0, pos.data(), ea.data(), 0) == kMalformed);  // malformed before too few
  for (uint32_t at = 0; at < k; at++) {  // one bad field in entry `at`
    good_entries(k, &pos, &ea);
    pos[at] = W;
    CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kMalformed);
    pos[at] = 0xFFFFFFFFu;
    CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kMalformed);
    pos[at] = W - 1;  // the last position of the axis is a good one (no other entry is there: W - 1 >= k)
    CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kDevice);
    good_entries(k, &pos, &ea);
    ea[at] = 2;
    CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kMalformed);
    if (at > 0) {
      good_entries(k, &pos, &ea);
      pos[at] = pos[at - 1];
      CHECK(classify(k, 0, 0, pos.data(), ea.data(), k) == kMalformed);
      CHECK(classify(k, 0, 0, pos.data(), ea.data(), at) == kTooFew);  // the entries before the repeat
    }
  }
  // a repeat among fewer than k entries is malformed, not too few
  if (k >= 3) {
    good_entries(k - 1, &pos, &ea);
    pos[k - 2] = 0;
    CHECK(classify(k, 0, 0, pos.data(), ea.data(), k - 1) == kMalformed);
  }
  // all W positions once: the largest good proof; one more entry must repeat one
  std::vector<uint32_t> full(W + 1);
  std::vector<uint8_t> fa(W + 1, 1);
  for (uint32_t e = 0; e < W; e++) full[e] = W - 1 - e;
  full[W] = 0;
  CHECK(classify(k, 1, k, full.data(), fa.data(), W) == kDevice);
  CHECK(classify(k, 1, k, full.data(), fa.data(), W + 1) == kMalformed);
  // a count far beyond the buffer: the repeat ends the scan inside the W + 1 entries
  CHECK(classify(k, 1, k, full.data(), fa.data(), (uint64_t)1 << 40) == kMalformed);
}

static void check_entry_at(uint32_t W) {
  const uint32_t k = W / 2;
  for (uint32_t axis = 0; axis < 2; axis++)
    for (uint32_t index = 0; index < W; index++)
      for (uint32_t p = 0; p < W; p++)
        for (uint32_t ea = 0; ea < 2; ea++) {
          const EntryAt a = entry_at(k, axis, index, p, ea);
          CHECK((axis ? a.col : a.row) == index && (axis ? a.row : a.col) == p);
          CHECK(a.root_axis == ea && a.root_index < W && a.leaf < W);
          // the pair (tree, leaf) names the cell
          CHECK((ea ? a.leaf : a.root_index) == a.row && (ea ? a.root_index : a.leaf) == a.col);
          CHECK(a.q0 == (a.row < k && a.col < k));
        }
}

static void check_plan(uint32_t W) {
  const uint32_t k = W / 2;
  // proofs: empty, k entries, malformed (axis), k - 1 entries, 2k entries, empty, malformed
  // (repeat), k entries
  struct P {
    uint8_t axis;
    uint32_t index, ne;
    int bad;  // 0 none, 1 repeat the first position at the end
    uint8_t want;
  };
  std::vector<P> ps = {{0, 0, 0, 0, kTooFew},       {0, 1, k, 0, kDevice},     {2, 0, k, 0, kMalformed},
                       {1, 0, k - 1, 0, kTooFew},   {1, W - 1, W, 0, kDevice}, {1, 0, 0, 0, kTooFew},
                       {0, 0, k + 1, 1, kMalformed}, {0, k, k, 0, kDevice}};
  const uint32_t n = (uint32_t)ps.size();
  const uint64_t base_e = 5, base_n = 11;  // offsets that do not start at zero
  std::vector<uint64_t> ent_off(n + 1);
  ent_off[0] = base_e;
  for (uint32_t i = 0; i < n; i++) ent_off[i + 1] = ent_off[i] + ps[i].ne;
  const uint64_t E = ent_off[n];
  std::vector<uint32_t> pos(E + 1, 0);
  std::vector<uint8_t> ea(E + 1, 0), axes(n);
  std::vector<uint32_t> index(n);
  std::vector<uint64_t> node_off(E + 2, 0);
  for (uint64_t e = 0; e <= E; e++) node_off[e + 1] = node_off[e] + (e < base_e ? 1 : (e * 7 + 3) % 5);  // 0 .. 4 nodes
  for (uint64_t e = 0; e < node_off.size(); e++) node_off[e] += base_n;
  for (uint32_t i = 0; i < n; i++) {
    axes[i] = ps[i].axis;
    index[i] = ps[i].index;
    for (uint32_t j = 0; j < ps[i].ne; j++) {
      pos[ent_off[i] + j] = (j + i) % W;  // distinct: ne <= W
      ea[ent_off[i] + j] = (uint8_t)((j + i) & 1);
    }
    if (ps[i].bad == 1) pos[ent_off[i] + ps[i].ne - 1] = pos[ent_off[i]];
  }
  VerifyPlan plan;
  CHECK(plan_verify(n, k, axes.data(), index.data(), ent_off.data(), pos.data(), ea.data(), node_off.data(), &plan));
  CHECK(plan.verdict.size() == n);
  std::vector<uint32_t> want_live;
  std::vector<uint64_t> want_e(1, 0), want_n(1, 0);
  for (uint32_t i = 0; i < n; i++) {
    // k = 1: k - 1 entries is an empty proof, still too few; the repeat needs two entries
    CHECK(plan.verdict[i] == ps[i].want);
    if (ps[i].want != kDevice) continue;
    want_live.push_back(i);
    want_e.push_back(want_e.back() + ps[i].ne);
    uint64_t nn = 0;
    for (uint64_t e = ent_off[i]; e < ent_off[i + 1]; e++) nn += node_off[e + 1] - node_off[e];
    want_n.push_back(want_n.back() + nn);
  }
  CHECK(plan.live == want_live && plan.ent0 == want_e && plan.node0 == want_n);
  CHECK(plan.entries() == want_e.back() && plan.nodes() == want_n.back());
  // a batch of empty proofs only
  std::vector<uint64_t> zero(4, 9);
  VerifyPlan empty;
  CHECK(plan_verify(3, k, axes.data(), index.data(), zero.data(), nullptr, nullptr, nullptr, &empty));
  CHECK(empty.live.empty() && empty.entries() == 0 && empty.nodes() == 0);
  CHECK(empty.verdict == (std::vector<uint8_t>{kTooFew, kTooFew, kMalformed}));
  // decreasing offsets
  std::vector<uint64_t> dec(ent_off);
  dec[2] = dec[1] - 1;
  CHECK(!plan_verify(n, k, axes.data(), index.data(), dec.data(), pos.data(), ea.data(), node_off.data(), &plan));
  std::vector<uint64_t> decn(node_off);
  decn[base_e + 1] = decn[base_e] - 1;
  CHECK(!plan_verify(n, k, axes.data(), index.data(), ent_off.data(), pos.data(), ea.data(), decn.data(), &plan));
}

struct Counts {
  uint64_t masks, taken, skipped;
};

static void check_select(uint32_t W, Counts* n) {
  const uint32_t k = W / 2;
  const uint32_t idx[3] = {0, k, W - 1};
  for (const std::vector<uint8_t>& m : masks_of(W)) {
    for (uint32_t axis = 0; axis < 2; axis++)
      for (uint32_t index : idx) {
        const std::vector<uint32_t> got = select_positions(m.data(), W, axis, index);
        std::vector<uint32_t> want;
        for (uint32_t j = 0; j < W; j++) {
          const bool cell = m[axis ? (size_t)j * W + index : (size_t)index * W + j] != 0;
          const bool complete = known(m, W, !axis, j) == W;
          if (cell && complete) want.push_back(j);
          else if (cell) n->skipped++;
        }
        CHECK(got == want);
        n->taken += want.size();
      }
    CHECK(select_positions(m.data(), W, 2, 0).empty() && select_positions(m.data(), W, 0, W).empty());
    n->masks++;
  }
}

// nmt ProveRange(leaf, leaf + 1) over 2^L leaves: (level, pos) of the maximal subtrees outside
static void walk(uint32_t s, uint32_t e, uint32_t leaf, std::vector<std::pair<uint32_t, uint32_t>>* out) {
  if (e <= leaf || s > leaf) {
    uint32_t l = 0;
    while ((1u << l) < e - s) l++;
    out->push_back({l, s >> l});
    return;
  }
  if (e - s == 1) return;
  const uint32_t mid = s + (e - s) / 2;
  walk(s, mid, leaf, out);
  walk(mid, e, leaf, out);
}

static void check_records(uint32_t W) {
  const uint32_t L = log2_width(W), count = 3;
  CHECK((1u << L) == W);
  CHECK(trees_level_rec(W, count, L + 1) == (uint64_t)count * (2 * W - 1));
  for (uint32_t a = 0; a < count; a++) {
    CHECK(root_record(W, count, a) == (uint64_t)count * (2 * W - 2) + a);
    for (uint32_t leaf = 0; leaf < W; leaf++) {
      std::vector<int32_t> rec(L + 1, -7);
      proof_records(W, count, a, leaf, rec.data());
      std::vector<std::pair<uint32_t, uint32_t>> want;
      walk(0, W, leaf, &want);
      CHECK(want.size() == L && rec[L] == -7);
      for (uint32_t j = 0; j < L && j < want.size(); j++) {
        uint64_t at = 0;  // level-major: the levels below, then tree a's run, then the node
        for (uint32_t l = 0; l < want[j].first; l++) at += (uint64_t)count * (W >> l);
        CHECK((uint64_t)rec[j] == at + (uint64_t)a * (W >> want[j].first) + want[j].second);
      }
    }
  }
  // compact_entries: the kept ones move up in order, whole
  const uint32_t nc = W;
  std::vector<uint8_t> ok(nc), shares((size_t)nc * 8), nodes((size_t)nc * 6);
  std::vector<uint32_t> pos(nc), want_pos;
  for (uint32_t a = 0; a < nc; a++) {
    ok[a] = (a * 5 + 1) % 3 != 0;
    pos[a] = 100 + a;
    std::memset(&shares[(size_t)a * 8], (int)a, 8);
    std::memset(&nodes[(size_t)a * 6], (int)(a + 64), 6);
    if (ok[a]) want_pos.push_back(100 + a);
  }
  const uint32_t m = compact_entries(ok.data(), nc, pos.data(), shares.data(), 8, nodes.data(), 6);
  CHECK(m == want_pos.size());
  for (uint32_t e = 0; e < m && e < want_pos.size(); e++) {
    const uint32_t a = want_pos[e] - 100;
    CHECK(pos[e] == want_pos[e]);
    for (uint32_t b = 0; b < 8; b++) CHECK(shares[(size_t)e * 8 + b] == (uint8_t)a);
    for (uint32_t b = 0; b < 6; b++) CHECK(nodes[(size_t)e * 6 + b] == (uint8_t)(a + 64));
  }
}

int main() {
  CHECK(valid_width(1) && valid_width(512) && !valid_width(0) && !valid_width(3) && !valid_width(1024));
  for (uint32_t W = 2; W <= 64; W *= 2) {
    cur_w = W;
    Counts n{0, 0, 0};
    check_classify(W);
    check_entry_at(W);
    check_plan(W);
    check_select(W, &n);
    check_records(W);
    std::printf("W = %2u: %llu masks, %llu taken, %llu skipped\n", W, (unsigned long long)n.masks,
                (unsigned long long)n.taken, (unsigned long long)n.skipped);
  }
  std::printf("befp plan check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
