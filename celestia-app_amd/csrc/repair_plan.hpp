// The repair's host planner (api_repair.cpp): everything rsmt2d's Repair decides from the
// presence mask alone. The pass-parallel schedule's bookkeeping (MaskBits), rsmt2d's own
// sweep order (plan_sweeps), the log of checks both leave behind and its replay over the
// roots and flags the device sends back, and the pass schedule as a stepper, of one square
// (SquarePasses) and merged over a batch of squares (BatchPasses): the repair drives either
// through the same next() / apply(). Plain C++ with no HIP in it: tools/repair_plan_check.cpp
// and tools/repair_batch_plan_check.cpp include this header alone and step it on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/celestia_eds.h"

namespace cel {
namespace repair {

constexpr size_t kRoot = CEL_NMT_NODE_SIZE;

// One check of the replay, in rsmt2d's order (oracle/eds.c orc_repair):
//   SANITY  an axis complete before the repair: root (else "bad root input"), encoding
//   SOLVE   an axis decoded by solve `solve`: encoding, root
//   ORTH    an axis that solve `solve` completed: root, encoding
struct Check {
  enum Kind { SANITY, SOLVE, ORTH } kind;
  int is_col;
  int32_t idx;
  int32_t solve;  // index into the solve log (-1 for SANITY)
};
struct Solve {
  int is_col;
  int32_t idx;
};

// The caller's presence bytes as 0 / 1.
inline std::vector<uint8_t> normalise_mask(const uint8_t* present, size_t cells) {
  std::vector<uint8_t> hm(cells);
  for (size_t i = 0; i < cells; i++) hm[i] = present[i] != 0;
  return hm;
}

// The rows the first pass solves (k <= known cells < 2k), ascending, from the byte mask
// alone: the repair enqueues their decode before it builds the bitsets.
inline std::vector<int32_t> first_row_pass(const uint8_t* hm, uint32_t k) {
  const uint32_t W = 2 * k;
  std::vector<int32_t> first;
  for (uint32_t i = 0; i < W; i++) {  // hm bytes are 0 / 1: a word's popcount is its count
    const uint8_t* r = hm + (size_t)i * W;
    uint32_t c = 0;
    uint32_t j = 0;
    for (; j + 8 <= W; j += 8) {
      uint64_t x;
      std::memcpy(&x, r + j, 8);
      c += (uint32_t)__builtin_popcountll(x);
    }
    for (; j < W; j++) c += r[j];
    if (c >= k && c < W) first.push_back((int32_t)i);
  }
  return first;
}
inline std::vector<int32_t> first_row_pass(const std::vector<uint8_t>& hm, uint32_t k) {
  return first_row_pass(hm.data(), k);
}

// a[i] bit j <-> a[j] bit i
inline void transpose64(uint64_t* a) {
  uint64_t m = 0x00000000FFFFFFFFull;
  for (int j = 32; j != 0; j >>= 1, m ^= (m << j)) {
    for (int k = 0; k < 64; k = ((k | j) + 1) & ~j) {
      const uint64_t t = ((a[k] >> j) ^ a[k | j]) & m;
      a[k | j] ^= t;
      a[k] ^= t << j;
    }
  }
}

// The presence mask as bitsets by row and by column (bit j of axis i = cell j of it) with
// per-axis counts, so a solve's bookkeeping visits only the cells it fills.
struct MaskBits {
  uint32_t W, nw;
  std::vector<uint64_t> bits[2];  // [is_col][axis * nw + word]
  std::vector<uint32_t> cnt[2];
  uint64_t total = 0;
  MaskBits(const std::vector<uint8_t>& hm, uint32_t w) : MaskBits(hm.data(), w) {}
  MaskBits(const uint8_t* hm, uint32_t w) : W(w), nw((w + 63) / 64) {
    const uint32_t P = nw * 64;  // padded to whole 64x64 tiles for the transpose
    std::vector<uint64_t> rows((size_t)P * nw, 0), cols((size_t)P * nw, 0);
    for (uint32_t i = 0; i < W; i++) {
      const uint8_t* r = hm + (size_t)i * W;
      for (uint32_t j = 0; j < W; j += 8) {
        uint64_t x = 0;
        const uint32_t n = W - j < 8 ? W - j : 8;
        std::memcpy(&x, r + j, n);  // bytes 0 / 1
        rows[(size_t)i * nw + j / 64] |= ((x * 0x0102040810204080ull) >> 56) << (j % 64);
      }
    }
    // cols = rows transposed, tile by tile
    uint64_t t[64];
    for (uint32_t bi = 0; bi < nw; bi++)
      for (uint32_t bj = 0; bj < nw; bj++) {
        for (int r = 0; r < 64; r++) t[r] = rows[(size_t)(bi * 64 + r) * nw + bj];
        transpose64(t);
        for (int r = 0; r < 64; r++) cols[(size_t)(bj * 64 + r) * nw + bi] = t[r];
      }
    rows.resize((size_t)W * nw);
    cols.resize((size_t)W * nw);
    bits[0] = std::move(rows);
    bits[1] = std::move(cols);
    for (int d = 0; d < 2; d++) {
      cnt[d].assign(W, 0);
      for (uint32_t i = 0; i < W; i++) {
        uint32_t c = 0;
        for (uint32_t q = 0; q < nw; q++) c += (uint32_t)__builtin_popcountll(bits[d][(size_t)i * nw + q]);
        cnt[d][i] = c;
      }
    }
    for (uint32_t i = 0; i < W; i++) total += cnt[0][i];
  }
  // A pass: every axis of `list` (direction is_col, ascending) gets all its cells.
  // orth[t] = the orthogonal axes that solve list[t] completes, ascending: those whose
  // missing cells all lie in listed axes, the last of them in list[t] (rsmt2d fills the
  // axes one by one in list order). Word operations over the bitsets, O(W^2 / 64).
  void fill_pass(int is_col, const std::vector<int32_t>& list, std::vector<std::vector<int32_t>>& orth) {
    std::vector<uint64_t> S(nw, 0);
    std::vector<int32_t> pos(W, -1);
    for (size_t t = 0; t < list.size(); t++) {
      S[(uint32_t)list[t] / 64] |= 1ull << ((uint32_t)list[t] % 64);
      pos[list[t]] = (int32_t)t;
    }
    orth.assign(list.size(), {});
    for (uint32_t j = 0; j < W; j++) {
      if (cnt[!is_col][j] == W) continue;
      uint64_t* a = bits[!is_col].data() + (size_t)j * nw;
      bool inside = true;
      int32_t last = -1;
      uint32_t c = 0;
      for (uint32_t q = 0; q < nw; q++) {
        const uint64_t valid = (q + 1) * 64 <= W ? ~0ull : ((1ull << (W % 64)) - 1);
        const uint64_t miss = ~a[q] & valid;
        if (miss & ~S[q]) inside = false;
        if (miss) last = (int32_t)(q * 64 + 63 - __builtin_clzll(miss));
        a[q] |= S[q];
        c += (uint32_t)__builtin_popcountll(a[q] & valid);
      }
      total += c - cnt[!is_col][j];
      cnt[!is_col][j] = c;
      if (inside && last >= 0) orth[pos[last]].push_back((int32_t)j);
    }
    for (int32_t i : list) {
      uint64_t* a = bits[is_col].data() + (size_t)i * nw;
      for (uint32_t q = 0; q < nw; q++) a[q] = (q + 1) * 64 <= W ? ~0ull : ((1ull << (W % 64)) - 1);
      cnt[is_col][i] = W;
    }
  }
};

// The sequential view of a pass fill_pass has just applied: solve list[t] fills its missing
// cells, completing the orthogonal axes by_solve[t]. Appends the solves and their checks to
// the logs; orth = every orthogonal axis the pass completed, ascending.
inline void log_pass(int is_col, const std::vector<int32_t>& list, const std::vector<std::vector<int32_t>>& by_solve,
                     std::vector<Check>& order, std::vector<Solve>& solves, std::vector<int32_t>& orth) {
  orth.clear();
  for (size_t t = 0; t < list.size(); t++) {
    const int32_t si = (int32_t)solves.size();
    order.push_back({Check::SOLVE, is_col, list[t], si});
    for (int32_t j : by_solve[t]) {
      order.push_back({Check::ORTH, !is_col, j, si});
      orth.push_back(j);
    }
    solves.push_back({is_col, list[t]});
  }
  std::sort(orth.begin(), orth.end());
}

// hm := the presence mask before solve `upto` of `solves` (each solve completes its axis)
inline void rollback(std::vector<uint8_t>& hm, uint32_t W, const std::vector<Solve>& solves, size_t upto) {
  for (size_t t = 0; t < upto; t++) {
    const uint32_t i = (uint32_t)solves[t].idx;
    if (solves[t].is_col)
      for (uint32_t j = 0; j < W; j++) hm[(size_t)j * W + i] = 1;
    else
      std::memset(hm.data() + (size_t)i * W, 1, W);
  }
}

// rsmt2d's sweeps over the mask alone (every solve completes its axis): the solve
// sequence, each solve's level (one more than the highest level among the solves that
// filled a cell it reads) and the check order (SOLVE, then the ORTH axes it completes,
// ascending); cnt = known cells per axis at the end.
struct SweepPlan {
  std::vector<Solve> solves;
  std::vector<int32_t> level;
  std::vector<Check> order;
  std::vector<uint32_t> cnt[2];
  int32_t nlevels = 0;
  bool solved = false;
};

inline SweepPlan plan_sweeps(const std::vector<uint8_t>& hm, uint32_t k) {
  const uint32_t W = 2 * k;
  const size_t cells = (size_t)W * W;
  SweepPlan p;
  std::vector<uint8_t> m(hm);
  p.cnt[0].assign(W, 0);
  p.cnt[1].assign(W, 0);
  auto& cnt = p.cnt;
  size_t total = 0;
  for (uint32_t i = 0; i < W; i++)
    for (uint32_t j = 0; j < W; j++)
      if (m[(size_t)i * W + j]) {
        cnt[0][i]++;
        cnt[1][j]++;
        total++;
      }
  std::vector<int32_t> lvl_of(cells, 0);
  p.solved = total == cells;
  while (!p.solved) {
    bool progress = false;
    for (uint32_t i = 0; i < W; i++)
      for (int d = 0; d < 2; d++) {
        if (cnt[d][i] == W || cnt[d][i] < k) continue;
        const size_t base_c = d ? i : (size_t)i * W, step = d ? W : 1;
        int32_t L = 0;
        for (uint32_t j = 0; j < W; j++) {
          const size_t c = base_c + j * step;
          if (m[c] && lvl_of[c] > L) L = lvl_of[c];
        }
        L++;
        const int32_t si = (int32_t)p.solves.size();
        p.order.push_back({Check::SOLVE, d, (int32_t)i, si});
        for (uint32_t j = 0; j < W; j++) {
          const size_t c = base_c + j * step;
          if (m[c]) continue;
          if (cnt[!d][j] == W - 1) p.order.push_back({Check::ORTH, !d, (int32_t)j, si});
          m[c] = 1;
          lvl_of[c] = L;
          cnt[!d][j]++;
          total++;
        }
        cnt[d][i] = W;
        p.solves.push_back({d, (int32_t)i});
        p.level.push_back(L);
        if (L > p.nlevels) p.nlevels = L;
        progress = true;
      }
    if (total == cells) p.solved = true;
    if (!progress) break;
  }
  return p;
}

// One check against what the device found: the axis's root as computed, its expected root
// (kRoot bytes each) and its encoding-check flag. CEL_OK, or the status rsmt2d fails with:
// "bad root input" for a complete axis whose root differs, byzantine for everything else.
inline cel_status check_status(Check::Kind kind, const uint8_t* got, const uint8_t* exp, int32_t flag) {
  if (std::memcmp(got, exp, kRoot) != 0) return kind == Check::SANITY ? CEL_EBADROOT : CEL_EBYZANTINE;
  return flag ? CEL_EBYZANTINE : CEL_OK;
}

// The replay of n checks in rsmt2d's order: the first that fails (index into order, -1 if
// none) and its status. exp[is_col]: the expected roots, kRoot bytes per axis; flags:
// [2][W] by (direction, axis); got: the device's roots, [2][W] records of got.stride bytes
// by direction, an axis's record at its index (BY_AXIS: every root of the square) or at its
// rank among the checks of its direction in `order` (BY_RANK: repair_exact's gathered axes).
struct RootRecords {
  const uint8_t* at;
  size_t stride;
  enum { BY_AXIS, BY_RANK } slot;
};
inline long first_failure(const Check* order, size_t n, const RootRecords& got, const uint8_t* const exp[2],
                          const int32_t* flags, uint32_t W, cel_status* code) {
  size_t rank[2] = {0, 0};
  for (size_t t = 0; t < n; t++) {
    const Check& c = order[t];
    const size_t at = (size_t)c.is_col * W + (got.slot == RootRecords::BY_RANK ? rank[c.is_col]++ : (size_t)c.idx);
    *code = check_status(c.kind, got.at + at * got.stride, exp[c.is_col] + (size_t)c.idx * kRoot,
                         flags[(size_t)c.is_col * W + c.idx]);
    if (*code != CEL_OK) return (long)t;
  }
  return -1;
}

// ------------------------------------------------------------------ batch of squares
//
// The repair of n squares in one call (cel_dev_repair_batch) merges their pass schedules by
// round and direction: global pass (round r, rows) is every square's row list of round r, one
// after another in square order, and likewise the columns. A square with nothing to solve in
// a pass is absent from it, so each square's projection of the merged passes is its own
// schedule, pass for pass, and the checks, the solve log and the rollback stay per square.

// An entry of a merged pass, as the batch kernels read it (rs_decode_axis.hip, rs_axis.hip):
// axis in bits 0..8, square in bits 9..29, direction in bit 30.
constexpr uint32_t kEntryAxisBits = 9, kEntrySquareBits = 21;
inline int32_t pack_entry(uint32_t square, uint32_t axis, int is_col) {
  return (int32_t)(axis | (square << kEntryAxisBits) | ((uint32_t)(is_col != 0) << 30));
}
inline uint32_t entry_axis(int32_t e) { return (uint32_t)e & ((1u << kEntryAxisBits) - 1); }
inline uint32_t entry_square(int32_t e) { return ((uint32_t)e >> kEntryAxisBits) & ((1u << kEntrySquareBits) - 1); }
inline int entry_is_col(int32_t e) { return (int)(((uint32_t)e >> 30) & 1u); }
inline bool entries_fit(uint32_t n, uint32_t W) { return W <= (1u << kEntryAxisBits) && n <= (1u << kEntrySquareBits); }

// The first row pass of every square (first_row_pass per mask, packed): what the batch
// enqueues before any square's bookkeeping exists. masks: [n][W * W] bytes 0 / 1.
inline std::vector<int32_t> first_row_pass_batch(const std::vector<uint8_t>& masks, uint32_t n, uint32_t k) {
  const size_t cells = (size_t)4 * k * k;
  std::vector<int32_t> first;
  for (uint32_t q = 0; q < n; q++) {
    for (int32_t i : first_row_pass(masks.data() + q * cells, k)) first.push_back(pack_entry(q, (uint32_t)i, 0));
  }
  return first;
}

// One square's pass schedule as a stepper: every solvable row, then every solvable column,
// until the square is solved or stuck. The constructor builds the bitsets and the sanity
// checks (preRepairSanityCheck: for i: row i, column i; they open `order`). next() gives the
// next non-empty pass from the counts alone (cheap: the caller enqueues its decode at once);
// apply() is then the sequential view of that pass (fill_pass, log_pass) and gives the
// orthogonal axes it completed, in direction !is_col. Plain axis indices, as the
// single-square kernels read them.
struct SquarePasses {
  uint32_t k, W;
  MaskBits mb;
  std::vector<int32_t> sanity[2];  // the axes complete at the start, by direction
  std::vector<Check> order;
  std::vector<Solve> solves;
  std::vector<int32_t> cur;                    // the pass solvable() found last
  std::vector<std::vector<int32_t>> by_solve;  // the orthogonal axes each of its solves completed
  SquarePasses(const uint8_t* hm, uint32_t k_) : k(k_), W(2 * k_), mb(hm, 2 * k_) {
    for (uint32_t i = 0; i < W; i++)
      for (int is_col = 0; is_col < 2; is_col++)
        if (mb.cnt[is_col][i] == W) {
          order.push_back({Check::SANITY, is_col, (int32_t)i, -1});
          sanity[is_col].push_back((int32_t)i);
        }
  }
  bool solved() const { return mb.total == (uint64_t)W * W; }
  // cur = what a pass in direction is_col solves now; false when that is nothing. A batch
  // asks every square for the direction of the merged pass.
  bool solvable(int is_col) {
    dir = is_col;
    cur.clear();
    if (solved()) return false;
    for (uint32_t i = 0; i < W; i++)
      if (mb.cnt[is_col][i] >= k && mb.cnt[is_col][i] < W) cur.push_back((int32_t)i);
    return !cur.empty();
  }
  // false: solved or stuck
  bool next(int* is_col, std::vector<int32_t>& list) {
    for (uint32_t tries = 0; tries < 2; tries++) {
      if (solvable(dir)) {
        *is_col = dir;
        list = cur;
        return true;
      }
      dir ^= 1;
    }
    return false;
  }
  void apply(std::vector<int32_t>& orth) {
    mb.fill_pass(dir, cur, by_solve);
    log_pass(dir, cur, by_solve, order, solves, orth);
    dir ^= 1;
  }

 private:
  int dir = 0;  // direction of cur, then of the pass next() looks at first
};

// The merged schedule of n squares, pass by pass, with SquarePasses' surface: next() gives the
// next non-empty global pass, apply() runs every listed square's bookkeeping. Entries, sanity
// lists and orthogonal axes are packed. Serial per square.
struct BatchPasses {
  uint32_t n, k, W;
  std::vector<SquarePasses> sq;
  std::vector<int32_t> sanity[2];  // packed, by direction
  BatchPasses(const std::vector<uint8_t>& masks, uint32_t n_, uint32_t k_) : n(n_), k(k_), W(2 * k_) {
    const size_t cells = (size_t)W * W;
    sq.reserve(n);
    for (uint32_t q = 0; q < n; q++) {
      sq.emplace_back(masks.data() + q * cells, k);
      for (int d = 0; d < 2; d++)
        for (int32_t i : sq[q].sanity[d]) sanity[d].push_back(pack_entry(q, (uint32_t)i, d));
    }
  }
  // false: no square has anything left to solve (each is solved or stuck)
  bool next(int* is_col, std::vector<int32_t>& entries) {
    for (uint32_t tries = 0; tries < 2; tries++, dir ^= 1) {
      entries.clear();
      for (uint32_t q = 0; q < n; q++)
        if (sq[q].solvable(dir))
          for (int32_t i : sq[q].cur) entries.push_back(pack_entry(q, (uint32_t)i, dir));
      if (!entries.empty()) {
        *is_col = dir;
        return true;
      }
    }
    return false;
  }
  void apply(std::vector<int32_t>& orth) {
    orth.clear();
    std::vector<int32_t> o;
    for (uint32_t q = 0; q < n; q++) {
      if (sq[q].cur.empty()) continue;
      sq[q].apply(o);
      for (int32_t j : o) orth.push_back(pack_entry(q, (uint32_t)j, !dir));
    }
    dir ^= 1;
  }

 private:
  int dir = 0;  // direction of the pass next() looks at first
};

// Square i's root records, [2][W] by (direction, axis) as first_failure reads them BY_AXIS, out
// of the batch commit's: [n][W] row roots, then [n][W] column roots, kRoot bytes each.
inline void square_roots(const uint8_t* all, uint32_t n, uint32_t W, uint32_t i, uint8_t* out) {
  const size_t axis_b = (size_t)W * kRoot;
  std::memcpy(out, all + i * axis_b, axis_b);
  std::memcpy(out + axis_b, all + ((size_t)n + i) * axis_b, axis_b);
}

// The whole merged schedule at once (cel_debug_repair_batch_plan, tools/repair_batch_plan_check.cpp).
struct BatchPass {
  int is_col;
  std::vector<int32_t> entries, orth;
};
inline std::vector<BatchPass> plan_batch(BatchPasses& bp) {
  std::vector<BatchPass> passes;
  BatchPass p;
  while (bp.next(&p.is_col, p.entries)) {
    bp.apply(p.orth);
    passes.push_back(p);
  }
  return passes;
}

}  // namespace repair
}  // namespace cel
