// Host-side pieces shared by the three NMT translation units (nmt_kernels.hip, nmt_slab.hip,
// nmt_trees.hip): the strided level job and its reducer, the launchers of kernels one file
// defines and another uses, and the ORDER x PF dispatch of the leaf kernels.
#pragma once
#include <type_traits>

#include "cel_internal.hpp"

namespace cel {

// One tree level of one tree set: `trees` trees of `nin` nodes, tree t's node l at
// in[t * tstride + l * lstride] (records), reduced into out[t][nin / 2] (compact).
// nin < 2: nothing to do (an empty job).
struct LevelJob {
  const uint32_t* in;
  uint32_t* out;
  uint32_t nin, trees, tstride, lstride;
};

// nmt_slab.hip. One level of two independent tree sets in one launch.
void launch_level_pair(const LevelJob& a, const LevelJob& b, hipStream_t s);
// The reducer: two tree sets reduced level by level in lockstep, one launch per level. Set
// j's first level is strided as its job says, later levels are compact in its own ping /
// pong buffers (trees * nin / 2 records each), and its last level writes one record per
// tree into roots_j. A set of single-node trees is left alone: its caller copies it.
void reduce_trees_pair(LevelJob a, uint32_t* ping_a, uint32_t* pong_a, uint32_t* roots_a, LevelJob b,
                       uint32_t* ping_b, uint32_t* pong_b, uint32_t* roots_b, hipStream_t s);
// The same for one set.
inline void reduce_trees(const LevelJob& a, uint32_t* ping, uint32_t* pong, uint32_t* roots, hipStream_t s) {
  reduce_trees_pair(a, ping, pong, roots, LevelJob{}, nullptr, nullptr, nullptr, s);
}

// nmt_kernels.hip. p[0..n) = v.
void launch_fill_i32(int32_t* p, uint32_t n, int32_t v, uint32_t block, hipStream_t s);
// RFC-6962 leaf digests of n node records into leafd ([n][8]), and the records packed to
// 90 bytes: the first n / 2 into row_out, the rest into col_out.
void launch_dah_leaves(const uint32_t* items, uint32_t n, uint32_t* leafd, uint8_t* row_out, uint8_t* col_out,
                       hipStream_t s);
// RFC-6962 roots of `lists` lists of n 96-byte records (one workgroup each; leafd: their
// leaf digests if already hashed, else nullptr) into dah ([lists][32]); status[g] (optional)
// from bad_axis[g]. out_src / host_out / out_bytes: k_merkle's copy-out (one list).
void launch_merkle(const uint32_t* items, const uint32_t* leafd, uint32_t n, uint32_t lists, uint8_t* dah,
                   const int32_t* bad_axis, int32_t* status, hipStream_t s, const uint8_t* out_src = nullptr,
                   uint8_t* host_out = nullptr, uint32_t out_bytes = 0);

// A leaf launch of this many lanes leaves at most two waves per SIMD (1024 SIMDs): load
// latency is then exposed and the prefetching leaf hash (leaf_hash<true>) pays.
inline bool latency_bound(uint64_t lanes) { return lanes <= 2ull * 1024 * 64; }

// The leaf kernels' two template flags from their run-time values: f(order, pf) gets them
// as std::bool_constant values.
template <class F>
void dispatch_order_pf(bool order, bool pf, F&& f) {
  if (pf) {
    if (order) f(std::true_type{}, std::true_type{});
    else f(std::false_type{}, std::true_type{});
  } else {
    if (order) f(std::true_type{}, std::false_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

}  // namespace cel
