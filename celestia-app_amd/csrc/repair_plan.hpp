// The repair's host planner (api_repair.cpp): everything rsmt2d's Repair decides from the
// presence mask alone. The pass-parallel schedule's bookkeeping (MaskBits), rsmt2d's own
// sweep order (plan_sweeps), the log of checks both leave behind and its replay over the
// roots and flags the device sends back. Plain C++ with no HIP in it:
// tools/repair_plan_check.cpp includes this header alone and walks it on the host.
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
inline std::vector<int32_t> first_row_pass(const std::vector<uint8_t>& hm, uint32_t k) {
  const uint32_t W = 2 * k;
  std::vector<int32_t> first;
  for (uint32_t i = 0; i < W; i++) {  // hm bytes are 0 / 1: a word's popcount is its count
    const uint8_t* r = hm.data() + (size_t)i * W;
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
  MaskBits(const std::vector<uint8_t>& hm, uint32_t w) : W(w), nw((w + 63) / 64) {
    const uint32_t P = nw * 64;  // padded to whole 64x64 tiles for the transpose
    std::vector<uint64_t> rows((size_t)P * nw, 0), cols((size_t)P * nw, 0);
    for (uint32_t i = 0; i < W; i++) {
      const uint8_t* r = hm.data() + (size_t)i * W;
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

}  // namespace repair
}  // namespace cel
