// Host-only arithmetic of blob share commitments (go-square v1.1.0 inclusion / shares) and
// the device plan of a batch of blobs (api_commit.cpp -> blob_commit.hip). Nothing in here
// needs HIP or another file of the library: square.cpp, inclusion_paths.cpp and a
// stand-alone host build (tools/blob_plan_check.cpp) all include it; under hipcc root_at is
// also a device function.
//
//   sparse_shares_needed  shares.SparseSharesNeeded
//   subtree_width         inclusion.SubTreeWidth
//   mountain_range        inclusion.MerkleMountainRangeSizes
//
// Device layout of a batch. Every share of every blob owns one leaf slot; a blob's first
// slot is a multiple of its subtree width w (a power of two, <= 1024), so every subtree of
// the blob is aligned to its own size in the slot space as well, and no subtree of <= 256
// leaves straddles a 256-slot tile. Node j of level L of a blob lives in place at slot
// first + (j << L). A level-L node j exists iff 2^L <= w and (j + 1) << L <= n, so after
// the last level the subtree roots sit at their leftmost leaf's slot:
//   the n / w full trees at first + i * w, then, for each set bit b of r = n mod w from
//   high to low, one tree of 2^b leaves at first + (n - r) + (r with bits <= b cleared).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define CEL_BLOB_HD __host__ __device__
#else
#define CEL_BLOB_HD
#endif

namespace cel {
namespace blob {

constexpr uint32_t kSparseFirst = 478;        // share 0: ns | info | sequence length(4) | data
constexpr uint32_t kSparseCont = 482;         // share j >= 1: ns | info | data
constexpr uint32_t kMaxShares = 1u << 20;     // per blob on the device path (w <= 1024)
constexpr uint32_t kTile = 256;               // leaf slots per workgroup of the leaf stage
constexpr uint32_t kNoBlob = 0xFFFFFFFFu;     // slot table entry of an alignment gap
constexpr uint64_t kMaxSlots = 1ull << 31;    // per device batch (slot indices are 32-bit)

inline uint32_t pow2ceil(uint64_t n) {
  uint32_t r = 1;
  while (r < n) r <<= 1;
  return r;
}
inline uint32_t log2u(uint32_t n) {
  uint32_t l = 0;
  while ((1u << l) < n) l++;
  return l;
}
inline uint64_t sparse_shares_needed(uint64_t len) {
  if (len == 0) return 0;
  if (len <= kSparseFirst) return 1;
  return 1 + (len - kSparseFirst + kSparseCont - 1) / kSparseCont;
}
// inclusion.BlobMinSquareSize: RoundUpPowerOfTwo(ceil(sqrt(shares)))
inline uint32_t blob_min_square_size(uint64_t shares) {
  return pow2ceil((uint64_t)std::ceil(std::sqrt((double)shares)));
}
// inclusion.SubTreeWidth: min(RoundUpPowerOfTwo(ceil(shares / threshold)), BlobMinSquareSize)
inline uint32_t subtree_width(uint32_t shares, uint32_t threshold) {
  const uint32_t s = pow2ceil(((uint64_t)shares + threshold - 1) / threshold);
  const uint32_t m = blob_min_square_size(shares);
  return s < m ? s : m;
}
// Number of subtree roots of n shares at width w.
inline uint32_t root_count(uint32_t n, uint32_t w) { return n / w + (uint32_t)__builtin_popcount(n % w); }
// inclusion.MerkleMountainRangeSizes(n, w)
inline void mountain_range(uint32_t n, uint32_t w, std::vector<uint32_t>& sizes) {
  sizes.clear();
  for (uint32_t i = 0; i < n / w; i++) sizes.push_back(w);
  const uint32_t r = n % w;
  for (int b = 31; b >= 0; b--)
    if (r & (1u << b)) sizes.push_back(1u << b);
}

// One blob on the device (64 bytes).
struct Rec {
  uint32_t ns[8];   // the 29 namespace bytes (little-endian dwords), then 3 zero bytes
  uint64_t off;     // byte offset of the blob's data in the data buffer
  uint32_t len;     // data bytes
  uint32_t n;       // shares
  uint32_t first;   // first leaf slot, a multiple of 1 << wlog
  uint32_t wlog;    // log2 of the subtree width
  uint32_t root0;   // index of the blob's first root digest
  uint32_t nroots;
};
static_assert(sizeof(Rec) == 64, "device blob record");

struct Plan {
  std::vector<Rec> recs;
  uint64_t slots = 0;      // leaf slots, a multiple of kTile
  uint64_t roots = 0;      // subtree roots of all blobs
  uint32_t max_wlog = 0;
  uint32_t max_roots = 0;  // of one blob
};

// Appends one blob to the plan. The caller has checked 1 <= len and n <= kMaxShares.
inline void plan_add(Plan& p, const uint8_t* ns29, uint64_t off, uint64_t len, uint32_t threshold) {
  Rec r;
  std::memset(&r, 0, sizeof r);
  std::memcpy(r.ns, ns29, 29);
  r.off = off;
  r.len = (uint32_t)len;
  r.n = (uint32_t)sparse_shares_needed(len);
  const uint32_t w = subtree_width(r.n, threshold);
  r.wlog = log2u(w);
  const uint64_t first = (p.slots + w - 1) / w * w;
  r.first = (uint32_t)first;
  r.root0 = (uint32_t)p.roots;
  r.nroots = root_count(r.n, w);
  p.slots = first + r.n;
  p.roots += r.nroots;
  if (r.wlog > p.max_wlog) p.max_wlog = r.wlog;
  if (r.nroots > p.max_roots) p.max_roots = r.nroots;
  p.recs.push_back(r);
}

// Rounds the slot space up to whole tiles and fills the slot -> blob table (slots entries).
inline void plan_finish(Plan& p, uint32_t* slot_blob) {
  p.slots = (p.slots + kTile - 1) / kTile * kTile;
  uint64_t s = 0;
  for (size_t b = 0; b < p.recs.size(); b++) {
    const Rec& r = p.recs[b];
    for (; s < r.first; s++) slot_blob[s] = kNoBlob;
    for (uint32_t j = 0; j < r.n; j++) slot_blob[s++] = (uint32_t)b;
  }
  for (; s < p.slots; s++) slot_blob[s] = kNoBlob;
}

// Root index (within the blob) of the subtree whose leftmost leaf is share s of a blob of n
// shares at width 1 << wlog, and its level; false if no subtree starts at s. One copy for
// the host (planner checks) and the device (blob_commit.hip evaluates it per slot).
CEL_BLOB_HD inline bool root_at(uint32_t n, uint32_t wlog, uint32_t s, uint32_t* index, uint32_t* level) {
  const uint32_t w = 1u << wlog, full = n >> wlog, r = n & (w - 1);
  if (s < (full << wlog)) {
    if (s & (w - 1)) return false;
    *index = s >> wlog;
    *level = wlog;
    return true;
  }
  const uint32_t t = s - (full << wlog);  // offset in the tail
  if (t >= r || (t & r) != t) return false;
  const uint32_t rest = r - t;            // r's bits below t's lowest set bit, if t is a prefix of r
  if (t && rest >= (t & (0u - t))) return false;
  *index = full + (uint32_t)__builtin_popcount(t);
  *level = 31u - (uint32_t)__builtin_clz(rest);
  return true;
}

}  // namespace blob
}  // namespace cel
