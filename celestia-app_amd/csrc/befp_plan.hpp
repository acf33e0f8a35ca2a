// Host planning of bad-encoding fraud proofs (api_befp.cpp), plain C++ with no HIP in it:
// tools/befp_plan_check.cpp includes this header alone and walks it on the host.
//   verifier  the verdicts that need no device (malformed, too few entries), which proofs go
//             to the device and where their entries and nodes lie in the packed upload, and
//             each entry's place in the square: the tree it is proved in, its leaf, its
//             namespace rule;
//   producer  which positions of the accused axis qualify from the presence mask, the node
//             records of a single-leaf proof in nmt order, and where the outputs go.
// A proof accuses axis (axis, index) of a 2k x 2k square, axis 0 a row, 1 a column. Entry
// `position` of it is cell (index, position) of an accused row, (position, index) of an accused
// column, proved in the cell's row tree (entry_axis 0) or column tree (entry_axis 1): the
// convention of cel_dev_place_samples.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cel {
namespace befp {

// The verdict bytes (CEL_BEFP_* of include/celestia_eds.h).
constexpr uint8_t kNotFraud = 0, kFraud = 1, kBadShare = 2, kTooFew = 3, kMalformed = 4;
constexpr uint8_t kDevice = 0xFF;  // plan only: the device decides (bad share, fraud, not fraud)

inline bool valid_width(uint32_t k) { return k && !(k & (k - 1)) && k <= 512; }

inline uint32_t log2_width(uint32_t W) {
  uint32_t L = 0;
  while ((1u << L) < W) L++;
  return L;
}

// ------------------------------------------------------------------ verifier

// Steps 1 and 2 of the verdict rule over the ne entries of one proof: kMalformed, kTooFew,
// or kDevice. Reads at most 2k + 1 entries: among that many in-range positions two are equal.
inline uint8_t classify(uint32_t k, uint32_t axis, uint32_t index, const uint32_t* positions, const uint8_t* ent_axes,
                        uint64_t ne) {
  const uint32_t W = 2 * k;
  if (axis > 1 || index >= W) return kMalformed;
  uint64_t seen[(2 * 512 + 63) / 64] = {};
  for (uint64_t e = 0; e < ne; e++) {
    const uint32_t p = positions[e];
    if (p >= W || ent_axes[e] > 1) return kMalformed;
    if (seen[p >> 6] >> (p & 63) & 1u) return kMalformed;
    seen[p >> 6] |= (uint64_t)1 << (p & 63);
  }
  return ne < k ? kTooFew : kDevice;
}

// Where one entry lies: its cell, the tree it is proved in (root `root_index` of the row roots
// when root_axis == 0, of the column roots when 1), its leaf there, and the wrapper's namespace
// rule (nmt_wrapper.go:100-107): q0 = the share's own namespace, else the parity namespace.
struct EntryAt {
  uint32_t row, col;
  uint32_t root_axis, root_index, leaf;
  bool q0;
};
inline EntryAt entry_at(uint32_t k, uint32_t axis, uint32_t index, uint32_t position, uint32_t entry_axis) {
  EntryAt a;
  a.row = axis ? position : index;
  a.col = axis ? index : position;
  a.root_axis = entry_axis;
  a.root_index = entry_axis ? a.col : a.row;
  a.leaf = entry_axis ? a.row : a.col;
  a.q0 = a.row < k && a.col < k;
  return a;
}

// The batch as the device sees it: the proofs that passed steps 1 and 2 ("live"), packed in
// order. Live proof s is proof live[s]; its entries are packed entries [ent0[s], ent0[s + 1]),
// its nodes packed nodes [node0[s], node0[s + 1]) (the caller's nodes node_off[ent_off[i]] ..
// node_off[ent_off[i + 1]] moved as one run).
struct VerifyPlan {
  std::vector<uint8_t> verdict;  // [n] kMalformed, kTooFew or kDevice
  std::vector<uint32_t> live;
  std::vector<uint64_t> ent0, node0;  // [live.size() + 1]
  uint64_t entries() const { return ent0.back(); }
  uint64_t nodes() const { return node0.back(); }
};

// false: decreasing offsets (the call's CEL_EINVAL). Offsets of proofs that never reach the
// device are still checked: they are the caller's own framing, not the peer's input.
inline bool plan_verify(uint32_t n, uint32_t k, const uint8_t* axes, const uint32_t* index, const uint64_t* ent_off,
                        const uint32_t* positions, const uint8_t* ent_axes, const uint64_t* node_off, VerifyPlan* out) {
  out->verdict.assign(n, kMalformed);
  out->live.clear();
  out->ent0.assign(1, 0);
  out->node0.assign(1, 0);
  for (uint32_t i = 0; i < n; i++)
    if (ent_off[i + 1] < ent_off[i]) return false;
  for (uint64_t e = ent_off[0]; e < ent_off[n]; e++)
    if (node_off[e + 1] < node_off[e]) return false;
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t e0 = ent_off[i], ne = ent_off[i + 1] - e0;
    // an empty proof's arrays may be null
    const uint8_t v = classify(k, axes[i], index[i], ne ? positions + e0 : nullptr, ne ? ent_axes + e0 : nullptr, ne);
    out->verdict[i] = v;
    if (v != kDevice) continue;
    out->live.push_back(i);
    out->ent0.push_back(out->ent0.back() + ne);
    out->node0.push_back(out->node0.back() + (node_off[e0 + ne] - node_off[e0]));
  }
  return true;
}

// ------------------------------------------------------------------ producer

// The positions of accused axis (axis, index) that the producer takes, ascending: the cell is
// known and its orthogonal axis (column j of an accused row, row j of an accused column) is
// complete in `present` (W * W bytes, non-zero = known). Whether that axis's root matches the
// header is the device's part.
inline std::vector<uint32_t> select_positions(const uint8_t* present, uint32_t W, uint32_t axis, uint32_t index) {
  std::vector<uint32_t> out;
  if (axis > 1 || index >= W) return out;
  for (uint32_t j = 0; j < W; j++) {
    if (!present[axis ? (size_t)j * W + index : (size_t)index * W + j]) continue;
    bool complete = true;
    for (uint32_t t = 0; t < W && complete; t++)
      complete = present[axis ? (size_t)j * W + t : (size_t)t * W + j] != 0;
    if (complete) out.push_back(j);
  }
  return out;
}

// First record of level l of the trees of `count` gathered axes (launch_axes_trees:
// level-major, level l = [count][W >> l]); l = L + 1 gives the record count.
inline uint64_t trees_level_rec(uint32_t W, uint32_t count, uint32_t l) {
  uint64_t at = 0;
  for (uint32_t i = 0; i < l; i++) at += (uint64_t)count * (W >> i);
  return at;
}

// The L = log2(W) records of the single-leaf proof of `leaf` in gathered tree `a` of `count`,
// in nmt order (ProveRange lists the maximal subtrees outside the range left to right): the
// left siblings along the leaf's path from the top down, then the right ones from the bottom up.
inline void proof_records(uint32_t W, uint32_t count, uint32_t a, uint32_t leaf, int32_t* rec) {
  const uint32_t L = log2_width(W);
  uint32_t j = 0;
  for (uint32_t l = L; l-- > 0;)
    if ((leaf >> l) & 1u) rec[j++] = (int32_t)(trees_level_rec(W, count, l) + (uint64_t)a * (W >> l) + ((leaf >> l) ^ 1u));
  for (uint32_t l = 0; l < L; l++)
    if (!((leaf >> l) & 1u)) rec[j++] = (int32_t)(trees_level_rec(W, count, l) + (uint64_t)a * (W >> l) + ((leaf >> l) ^ 1u));
}

// The root record of gathered tree a.
inline uint64_t root_record(uint32_t W, uint32_t count, uint32_t a) { return trees_level_rec(W, count, log2_width(W)) + a; }

// The candidates whose root matched (ok[a] != 0) moved to the front of the outputs, in order:
// positions [count], shares [count][share_b], nodes [count][L * node_b]. Returns how many.
inline uint32_t compact_entries(const uint8_t* ok, uint32_t count, uint32_t* positions, uint8_t* shares, size_t share_b,
                                uint8_t* nodes, size_t nodes_b) {
  uint32_t m = 0;
  for (uint32_t a = 0; a < count; a++) {
    if (!ok[a]) continue;
    if (m != a) {
      positions[m] = positions[a];
      for (size_t b = 0; b < share_b; b++) shares[m * share_b + b] = shares[a * share_b + b];
      for (size_t b = 0; b < nodes_b; b++) nodes[m * nodes_b + b] = nodes[a * nodes_b + b];
    }
    m++;
  }
  return m;
}

}  // namespace befp
}  // namespace cel
