// Internal declarations shared by the HIP kernels and the C-ABI host layer.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/celestia_eds.h"
#include "extend_plan.hpp"

namespace cel {

constexpr uint32_t kShare = CEL_SHARE_SIZE;
constexpr uint32_t kNs = CEL_NAMESPACE_SIZE;
constexpr uint32_t kNode = CEL_NMT_NODE_SIZE;
constexpr uint32_t kNodeWords = 24;  // 90-byte node padded to 96 B (24 dwords) on the device
constexpr uint32_t kMaxGf8Width = 128;   // k <= 128 -> 2k <= 256 shards -> GF(2^8)
constexpr uint32_t kMaxGf16Width = 2048; // LDS holds 2048 shards x 64 B per workgroup

// One RS encode launch: `axes` independent axes of n data shards each, for `nsq`
// squares. Shard i of axis a of square s lives at
//   in + s*in_sq + a*in_axis + i*in_shard        (len bytes)
// and its parity shard i goes to out + s*out_sq + a*out_axis + i*out_shard.
struct RsGeom {
  const uint8_t* in;
  uint8_t* out;
  uint64_t in_sq, in_axis, in_shard;
  uint64_t out_sq, out_axis, out_shard;
  // Optional copy of the data shards (the row pass writes Q0 into the EDS while it
  // has them in registers): dcopy + s*dc_sq + a*dc_axis + i*dc_shard. nullptr = none.
  uint8_t* dcopy;
  uint64_t dc_sq, dc_axis, dc_shard;
  // Blocked shard placement (row-sharded mode: the row pass writes straight into the
  // all-to-all send layout). When blk_log != 0, output / dcopy shard j goes to
  //   ((j >> blk_log) * *_blk) + (j & ((1 << blk_log) - 1)) * *_shard
  // instead of j * *_shard. Only the GF(2^16) register kernel supports it.
  uint32_t blk_log;
  uint64_t out_blk, dc_blk;
  uint32_t n;     // data shards per axis (power of two)
  uint32_t len;   // bytes per shard (multiple of 64)
  uint32_t axes;  // axes per square
  uint32_t nsq;   // squares
  // Check mode (GF(2^16) register kernel, n = 256/512, nsq == 1): nothing is stored; the
  // computed parity is compared with the bytes at `out` and a mismatch in axis a sets
  // chk_flags[chk_idx ? chk_idx[a] : a]. nullptr = encode.
  int32_t* chk_flags;
  const int32_t* chk_idx;
  // Check mode only: axis a of the launch is axis chk_axes[a] of the square (in/out bases
  // in + chk_axes[a]*in_axis, out + chk_axes[a]*out_axis), so the check reads the square in
  // place. nullptr = axis a.
  const int32_t* chk_axes;
};

struct DeviceTables {
  uint32_t* tw8 = nullptr;     // [255][8] GF(2^8) twiddle product tables, indexed by skew index
  uint16_t* exp16 = nullptr;   // [65536]
  uint16_t* log16 = nullptr;   // [65536]
  uint32_t* mul8 = nullptr;    // [256][8] GF(2^8) product tables indexed by log value (decoder)
  uint32_t* tw16 = nullptr;    // [4095][8] GF(2^16) bit-plane twiddles: products c*b_i in tower coordinates
  uint16_t* tower16 = nullptr; // [256 + 256 + 16] Cantor -> tower coordinates (lo, hi byte), b_i (decoder)
};

// Every workspace region starts on a 256-byte boundary.
constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bump-carver of a workspace: take<T>(bytes) returns the next region and advances by
// align256(bytes). Each path carves its workspace in one function; run on a null base
// (every pointer null, no arithmetic on it) the same function gives the workspace's size.
struct Carver {
  uint8_t* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<uint8_t*>(b)) {}
  template <class T>
  T* take(size_t bytes) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(bytes);
    return p;
  }
  // Another use of the same memory, `bytes` long from the base, lies over the regions taken
  // so far: the workspace holds whichever is longer.
  void overlay(size_t bytes) {
    if (off < align256(bytes)) off = align256(bytes);
  }
  size_t size() const { return off; }
};

// Block size 2^J of the GF(2^16) decoder's products by twiddles below 2^r (Cantor
// representation): such a twiddle lies in GF(2^(2^J)), the smallest Cantor subfield holding
// span(beta_0 .. beta_{r-1}).
constexpr uint32_t decode16_level(uint32_t r) { return r <= 1 ? 0 : r <= 2 ? 1 : r <= 4 ? 2 : r <= 8 ? 3 : 4; }

// roctx range over a phase's launches (rocprofv3 --marker-trace shows them on the host
// timeline; the launches themselves are asynchronous, so a range brackets their enqueue).
struct Range {
  explicit Range(const char* name) { roctxRangePushA(name); }
  ~Range() { roctxRangePop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};

// XCD-aware workgroup order. Workgroups are dealt round-robin over the 8 XCDs
// (MI355X_MICROARCH.md, "Workgroup dispatch"), so workgroup b shares an L2 with b + 8.
// Map them so that each XCD works through one contiguous range of logical ids: the
// column passes then stream adjacent column blocks through each XCD's L2 channels instead
// of one fixed residue of column offsets per XCD. A bijection of [0, nb) for any nb;
// for speed only (nothing relies on where a workgroup runs).
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb) {
  const uint32_t q = nb >> 3, r = nb & 7u, x = b & 7u;
  return x * q + (x < r ? x : r) + (b >> 3);
}

hipError_t upload_tables(DeviceTables* t);
void free_tables(DeviceTables* t);

// Kernel launchers, all asynchronous on `s`. Declared here: the rs_*.hip files (encode,
// decode, encoding check), nmt_kernels.hip (the EDS commit), nmt_slab.hip (the row-sharded
// mode), nmt_trees.hip (single trees, axes roots, exported trees, byte slices),
// repair_kernels.hip, blob_commit.hip, square_build.hip and probe_kernels.hip. The proof
// kernels declare theirs beside their layouts: nmt_verify.hpp, nmt_prove.hpp,
// nmt_namespace.hpp.
hipError_t launch_rs_encode(const RsGeom& g, const DeviceTables& t, hipStream_t s);
// The geometry of `axes` whole axes of nsq resident squares encoded in place: rows
// (is_col == 0) or columns from axis 0 on, data half in, parity half out.
RsGeom square_axis_geom(uint8_t* eds, uint32_t k, int is_col, uint32_t axes, uint32_t nsq);
hipError_t launch_rs_encode_bitslice(const RsGeom& g, hipStream_t s);  // GF(2^8), n <= 16
hipError_t launch_rs_encode_axis(const RsGeom& g, hipStream_t s);       // GF(2^8), 32 <= n <= 128
// Two launches' worth of GF(2^8) axes (same n, len, axes count and squares, no data copy) in
// one launch with their tiles interleaved per square (rs_axis.hip, k_rs_axis_gf8_pair).
hipError_t launch_rs_encode_axis_pair(const RsGeom& g1, const RsGeom& g2, hipStream_t s);
// Encoding check of listed axes in place in a resident EDS (flags[axis] |= 1 on mismatch),
// GF(2^8), k = 32, 64, 128.
hipError_t launch_rs_check_axes(const uint8_t* eds, uint32_t k, const int32_t* idx, int is_col, uint32_t naxes,
                                int32_t* flags, hipStream_t s);
hipError_t launch_rs_encode_gf16x(const RsGeom& g, hipStream_t s);     // GF(2^16), n = 256 / 512
// Full 2D extension of nsq squares: Q0 rows -> Q1, then all 2k columns -> Q2|Q3.
// ods == nullptr means Q0 is already in place inside eds.
hipError_t launch_extend(const uint8_t* ods, uint8_t* eds, uint32_t k, uint32_t nsq,
                         const DeviceTables& t, hipStream_t s);
// The two passes apart, for one square's latency path: Q0 rows [row0, row1) -> Q1 (Q0
// read in place in the EDS, or from a contiguous k x k ODS `ods` and then also written into
// Q0), and all 2k columns -> Q2|Q3 of nsq squares.
hipError_t launch_extend_rows(uint8_t* eds, uint32_t k, uint32_t row0, uint32_t row1, const DeviceTables& t,
                              hipStream_t s, const uint8_t* ods = nullptr);
hipError_t launch_extend_cols(uint8_t* eds, uint32_t k, uint32_t nsq, const DeviceTables& t, hipStream_t s);

// NMT + DAH over resident EDSs. work: scratch of nmt_workspace_size(k, nsq) bytes; its
// carve-up is nmt_kernels.hip's own. A batch (nsq > 1) hashes leaves and level 1 in one
// kernel and has no leaf area; one square keeps leaf records (the two-step commit below).
size_t nmt_workspace_size(uint32_t k, uint32_t nsq);
hipError_t launch_commit(const uint8_t* eds, uint32_t k, uint32_t nsq, uint8_t* row_roots,
                         uint8_t* col_roots, uint8_t* dah, int32_t* status, void* work,
                         bool order_check, hipStream_t s);
// One square's commit (nsq == 1) in two steps: the leaves of EDS rows [row0, row1)
// (init_bad: reset the push-order flags first; it must precede every leaf launch of the
// commit in stream order), then, after every leaf, the tree levels, roots and DAH.
hipError_t launch_commit_leaves(const uint8_t* eds, uint32_t k, uint32_t nsq, void* work, bool order_check,
                                uint32_t row0, uint32_t row1, bool init_bad, hipStream_t s);
// host_out (nsq == 1, optional): page-locked host memory that receives out_bytes (a multiple of
// 16) starting at row_roots from the DAH launch itself; row_roots, col_roots, dah and status
// must then be the parts of one ext::ResultBlock(k, 1) (extend_plan.hpp).
hipError_t launch_commit_trees(uint32_t k, uint32_t nsq, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                               int32_t* status, void* work, hipStream_t s, uint8_t* host_out = nullptr,
                               uint32_t out_bytes = 0);
// One erasured axis root (cells contiguous) or plain NMT root over leaves.
hipError_t launch_axis_root(const uint8_t* cells, uint32_t k, uint32_t axis, uint8_t* root,
                            void* work, hipStream_t s);
size_t axis_root_workspace_size(uint32_t k);
hipError_t launch_nmt_root(const uint8_t* leaves, uint32_t n, uint32_t leaf_len, uint8_t* root,
                           void* work, hipStream_t s);
size_t nmt_root_workspace_size(uint32_t n);
// RFC-6962 root over n items of item_len bytes (DataAvailabilityHeader.Hash).
hipError_t launch_merkle_root(const uint8_t* items, uint32_t n, uint32_t item_len, uint8_t* out,
                              void* work, hipStream_t s);
size_t merkle_workspace_size(uint32_t n);
// merkle.HashFromByteSlices over n slices of any length (data + off[i] .. off[i + 1]),
// all device pointers; work: slices_workspace_size(n) bytes.
hipError_t launch_hash_slices(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out, void* work,
                              hipStream_t s);
size_t slices_workspace_size(uint32_t n);

// Row-sharded mode (one column slab of one square per rank).
size_t slab_workspace_size(uint32_t k, uint32_t w);
// The slab commit in two steps: leaves of slab rows [row0, row1) (the rows < k half first,
// init_bad resetting the push-order flag), then, after every leaf, the trees and status.
hipError_t launch_slab_leaves(const uint8_t* slab, uint32_t k, uint32_t c0, uint32_t w, uint32_t row0, uint32_t row1,
                              void* work, bool order_check, bool init_bad, hipStream_t s);
hipError_t launch_slab_trees(uint32_t k, uint32_t w, uint32_t* col_rec, uint32_t* row_sub, int32_t* status,
                             void* work, hipStream_t s);
// A rank's two device steps (api_shard.cpp): the row pass into the all-to-all send layout
// [nranks][k/nranks][w][512], and the column pass + slab commit over [2k][w][512].
hipError_t shard_rows_enqueue(const DeviceTables& t, const uint8_t* ods_rows, uint32_t k, uint32_t nranks,
                              uint8_t* send, hipStream_t s);
hipError_t shard_cols_enqueue(const DeviceTables& t, uint8_t* slab, uint32_t k, uint32_t nranks, uint32_t rank,
                              uint32_t* col_rec, uint32_t* row_sub, int32_t* status, void* work, bool order_check,
                              hipStream_t s);
size_t shard_finish_workspace_size(uint32_t k, uint32_t nranks);
// gathered: [nranks][2k + w + 1] records, rank order (row subtrees, column roots, status).
hipError_t launch_shard_finish(const uint32_t* gathered, uint32_t k, uint32_t nranks, uint8_t* row_roots,
                               uint8_t* col_roots, uint8_t* dah, int32_t* status, void* work, bool order_check,
                               hipStream_t s);

// Same-run probes (probe_kernels.hip): SHA-256 chained in registers (out: blocks*256 words,
// clk: 2 counters per wave), and a streaming copy of `bytes` (a multiple of 16).
hipError_t launch_probe_sha(uint32_t* out, unsigned long long* clk, uint32_t blocks, int n, hipStream_t s);
// mode 0: copy `bytes` from src to dst (one lane per 16-byte element; blocks unused); 1: read
// src only; 2 / 3: write dst only, 16 / 4 bytes per lane (grid-strided over `blocks` workgroups)
hipError_t launch_probe_copy(const void* src, void* dst, uint64_t bytes, uint32_t blocks, int mode, bool nt,
                             hipStream_t s);
// GF(2^8) encode transform alone (rs_axis.hip), k = 32/64/128: ntiles tiles reading the same
// k x 256 B of src; dst (k x 256 B) written only when store != 0.
hipError_t launch_probe_rs_transform(uint32_t k, const uint32_t* src, uint32_t* dst, uint32_t ntiles, uint32_t store,
                                     hipStream_t s);
// GF(2^16) register kernel alone (rs_gf16x.hip), k = 256/512: ntiles 64-byte-block tiles, all
// loads from the 512 bytes at src, nothing stored.
hipError_t launch_probe_rs_transform_gf16(uint32_t k, const uint8_t* src, uint8_t* dst, uint32_t ntiles,
                                          hipStream_t s);

// Repair helpers (repair_kernels.hip, nmt_trees.hip).
hipError_t launch_gather_axes(const uint8_t* eds, const uint8_t* mask, uint32_t W, const int32_t* idx, int is_col,
                              uint32_t naxes, uint8_t* dense, uint8_t* dmask, hipStream_t s);
hipError_t launch_scatter_axes(uint8_t* eds, uint8_t* mask, uint32_t W, const int32_t* idx, int is_col,
                               uint32_t naxes, const uint8_t* dense, hipStream_t s);
hipError_t launch_cmp(const uint8_t* x, uint64_t xstride, const uint8_t* y, uint64_t ystride, uint64_t bytes,
                      uint32_t naxes, int32_t* flags, hipStream_t s, const int32_t* idx = nullptr);
size_t axes_roots_workspace_size(uint32_t k, uint32_t naxes);
// A single-wave kernel that idles `us` microseconds on s (schedule fuzzing only).
hipError_t launch_delay(uint32_t us, hipStream_t s);
hipError_t launch_axes_roots(const uint8_t* cells, uint32_t k, const int32_t* axis_idx, uint32_t naxes,
                             uint32_t* roots, void* work, hipStream_t s);

// Exported trees (proofs): all NMT levels of gathered axes (level-major, 96-byte records,
// axes_trees_nodes(k, naxes) records) and all RFC-6962 levels over n = 2^m 90-byte items
// (2n - 1 nodes of 8 big-endian words; work: merkle_workspace_size(n) bytes).
size_t axes_trees_nodes(uint32_t k, uint32_t naxes);
hipError_t launch_axes_trees(const uint8_t* cells, uint32_t k, const int32_t* axis_idx, uint32_t naxes,
                             uint32_t* nodes, hipStream_t s);
hipError_t launch_rfc_tree(const uint8_t* items90, uint32_t n, uint32_t* levels, void* work, hipStream_t s);

hipError_t launch_gather_nodes(const uint32_t* nodes, const int32_t* rec, uint32_t n, uint8_t* out, hipStream_t s);
// Blob share commitment (inclusion.cpp): trees of the gathered rows, subtree roots at
// (rows[i], depths[i], positions[i]) of the rows' ODS halves, RFC-6962 root -> d_out[32].
hipError_t launch_commitment(const uint8_t* d_cells, uint32_t k, uint32_t r0, uint32_t nrows, const uint32_t* rows,
                             const uint32_t* depths, const uint32_t* positions, uint32_t npaths, int32_t* d_idx,
                             uint32_t* d_nodes, uint8_t* d_items, void* d_merkle_work, uint8_t* d_out,
                             hipStream_t s);

// Blob share commitments from blob bytes (blob_commit.hip; plan and layout: blob_plan.hpp).
// d_work: blob_commit_workspace_size bytes whose head already holds the plan's tables (the
// records, then, 256-aligned, the slot table); d_out: 32 bytes per blob. d_shares (optional,
// plan.slots * 512 bytes): the A/B partner of the leaf stage, shares expanded into it first.
namespace blob {
struct Plan;
}
size_t blob_commit_workspace_size(uint64_t slots, uint64_t roots, uint32_t nblobs);
hipError_t launch_blob_commit(const uint8_t* d_data, const blob::Plan& plan, void* d_work, uint8_t* d_out,
                              hipStream_t s, uint32_t* d_shares = nullptr);

// The k x k ODS written into quadrant Q0 of d_eds from a layout (square_build.hip): d_segs
// the segments, d_share_seg the segment index of each of the k * k shares, d_compact the
// compact shares (16-byte aligned), d_txs the tx bytes the BLOB segments point into.
hipError_t launch_square_build(const uint8_t* d_txs, const cel_square_segment* d_segs, const uint32_t* d_share_seg,
                               const uint8_t* d_compact, uint8_t* d_eds, uint32_t k, hipStream_t s);
// The same for every block of a chunk in one launch (block_batch_plan.hpp): the blocks' plans
// concatenated, d_share_seg entries chunk-wide segment indices, d_seg_block the block of each
// segment, d_recs a bb::BlockRec per block; total_shares * 32 lanes, below 2^32.
namespace bb {
struct BlockRec;
}
hipError_t launch_square_build_batch(const uint8_t* d_txs, const cel_square_segment* d_segs, const uint32_t* d_share_seg,
                                     const uint32_t* d_seg_block, const bb::BlockRec* d_recs, const uint8_t* d_compact,
                                     uint8_t* d_eds, uint32_t total_shares, hipStream_t s);

// Erasure decode of `naxes` axes of 2n shards each, gathered into a dense
// [naxes][2n][len] buffer with a [naxes][2n] present mask. In place.
// GF(2^16) erasure decode over n = 512, 1024 or 2048 points (rs_decode_gf16.hip).
bool rs_decode_gf16_supported(uint32_t n);
// GF(2^16) encode of 1024 or 2048 data shards in bit planes (codec API).
hipError_t launch_rs_encode_gf16p(const RsGeom& g, const DeviceTables& t, hipStream_t s);
hipError_t launch_rs_decode_gf16(uint8_t* shards, const uint8_t* present, uint32_t naxes, uint32_t n, uint32_t len,
                                 const DeviceTables& t, hipStream_t s);
hipError_t launch_rs_decode(uint8_t* shards, const uint8_t* present, uint32_t naxes, uint32_t n,
                            uint32_t len, const DeviceTables& t, hipStream_t s);
// GF(2^8) register-resident decode (rs_decode_axis.hip): n = 32..256 points, len % 64 == 0.
bool rs_decode_axis_supported(uint32_t n, uint32_t len);
hipError_t launch_rs_decode_axis(uint8_t* shards, const uint8_t* present, uint32_t naxes, uint32_t n, uint32_t len,
                                 const uint32_t* mul8, hipStream_t s);
// The repair's solve of naxes axes (rows if is_col == 0, columns if 1, indices idx; with
// is_col < 0 every entry carries its direction in bit 30) of a W x W square of 512-byte
// cells in place: erased cells decoded straight into the square, the axes marked present
// in mask (W = 32 .. 256, the register decoder's range).
hipError_t launch_rs_decode_in_square(uint8_t* eds, uint8_t* mask, uint32_t W, const int32_t* idx, int is_col,
                                      uint32_t naxes, const uint32_t* mul8, hipStream_t s);
// The batch repair's passes over nsq squares back to back at eds ([nsq][W][W][512], masks
// [nsq][W*W]), W = 64, 128, 256: nent entries, each an axis of one square with its direction
// (repair_plan.hpp pack_entry). The decode as launch_rs_decode_in_square per entry; the
// encoding check as launch_rs_check_axes per entry, into flags[square][direction][axis].
hipError_t launch_rs_decode_in_squares(uint8_t* eds, uint8_t* masks, uint32_t W, uint32_t nsq, const int32_t* entries,
                                       uint32_t nent, const uint32_t* mul8, hipStream_t s);
hipError_t launch_rs_check_axes_batch(const uint8_t* eds, uint32_t k, uint32_t nsq, const int32_t* entries,
                                      uint32_t nent, int32_t* flags, hipStream_t s);

}  // namespace cel

// Page-locked staging that an enqueued upload may still be reading. An asynchronous entry
// returns while the copy out of `buf` may still be queued, so the buffer is refilled only after
// `ev` (recorded behind that copy, `pending` since) has passed: stage_acquire and stage_uploaded
// (api_common.hpp) are that rule, and but for the ctx's teardown nothing else touches the four
// fields. A caller may build its table before it asks for the buffer, as commit_enqueue does:
// nothing in between touches the buffer, so the wait may come after the planning.
namespace cel {
struct StagedUpload {
  void* buf = nullptr;
  size_t size = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
};
}  // namespace cel

// The opaque context of the C ABI.
struct cel_ctx {
  static constexpr int kPipe = cel::ext::kPipeStreams;  // internal streams of the chunked batch pipeline
  int device = 0;
  // The streams, in the order they are created: with four hardware queues per process a
  // stream's queue depends on how many were created before it, so the set stays as measured
  // (dl[2] and dl[3] carry no work: DESIGN.md section 5).
  hipStream_t stream = nullptr;
  hipStream_t sub[kPipe] = {nullptr, nullptr, nullptr, nullptr};
  // EDS downloads (dl[0], beside the hashing) and the k = 512 upload chunks (dl[1])
  hipStream_t dl[kPipe] = {nullptr, nullptr, nullptr, nullptr};
  // Events, each named for what it signals. A call records an event before it enqueues a wait
  // for it, and calls on a ctx hold its lock, so an event serves every path that means the
  // same thing by it.
  hipEvent_t ev_start = nullptr;  // the caller's stream at the start of a call: the internal streams begin here
  // CEL_FLAG_CALLER_STREAM batches: the previous one's extension-done event (recorded
  // once ext_pending); the next such batch starts after it (api.cpp)
  hipEvent_t ev_ext = nullptr;
  bool ext_pending = false;
  // the batch pipelines, by chunk number (ext::HostPlan, ext::PipePlan): chunk c's extension
  // is done (its EDS may go back), chunk c is committed (the call's stream may go on)
  hipEvent_t ev_extended[cel::ext::kHostChunks] = {};
  hipEvent_t ev_committed[cel::ext::kHostChunks] = {};
  static_assert(cel::ext::kPipeChunks <= cel::ext::kHostChunks, "ev_committed is indexed by either pipeline's chunk");
  // the one-square path: upload chunk c has arrived, the rows of chunk c are extended (chunk 0
  // where the square goes up whole), the column pass is done (the block path: the extension)
  hipEvent_t ev_up[cel::ext::kUp] = {};
  hipEvent_t ev_rows[cel::ext::kUp] = {};
  hipEvent_t ev_cols = nullptr;
  hipEvent_t ev_dl = nullptr;  // the download stream is done with the call's EDS
  // The repair's two streams (api_repair.cpp, RepairBufs). Its own events: the repair and the
  // extension never overlap on a ctx, since the ctx lock is held to a call's final sync, so
  // keeping them apart from the extension's events changes no ordering.
  hipEvent_t ev_repair_main = nullptr, ev_repair_side[2] = {}, ev_repair_done = nullptr;
  std::mutex mu;
  cel::DeviceTables tables;
  std::string last_error;
  // Grow-only device scratch (reused across calls on this ctx).
  static constexpr int kScratch = 7;
  void* scratch[kScratch] = {};
  size_t scratch_size[kScratch] = {};
  // Grow-only page-locked host staging (the repair's axis lists).
  void* hstage = nullptr;
  size_t hstage_size = 0;
  // The two staged uploads of a ctx. plan_up: the plans of the blob commitment calls
  // (api_commit.cpp), the proof tables of the NMT verifiers (api_verify.cpp), the request table
  // of the prover (api_prove.cpp) and the namespaces of a namespace plan (api_namespace.cpp),
  // through plan_stage / plan_uploaded. square_up: the square build's plan (api_block.cpp). Its
  // device copy, in scratch slot S_SQ, is a second matter: k_square_build reads it until
  // ev_sq_done, and the next call's stream waits for that event before its upload overwrites
  // the plan (enqueue_square); sq_built: a build has been enqueued.
  cel::StagedUpload plan_up, square_up;
  hipEvent_t ev_sq_done = nullptr;
  bool sq_built = false;
  // cel_dev_tree_index_build_batch: the squares' statuses as one device array (the index keeps
  // each in its slice's tail, an index size apart), so that they go back in one copy. The copy
  // reads it until ev_ix_status; the next build's stream waits for that event before its DAH
  // kernel writes the array again, and a build that has to grow it waits on the host.
  int32_t* ix_status = nullptr;
  size_t ix_status_n = 0;
  hipEvent_t ev_ix_status = nullptr;
  bool ix_status_pending = false;
  // The last cel_block_extend_batch on this ctx: each block's message ("" where it is CEL_OK),
  // for cel_block_batch_error.
  std::vector<std::string> block_errors;
  // Schedule fuzzing of the repair's two streams (cel_debug_schedule_fuzz; tests only):
  // before each enqueue point, an idle kernel of 0..fuzz_max_us microseconds.
  uint64_t fuzz_state = 0;
  uint32_t fuzz_max_us = 0;
  // The last blob plan made on this ctx (api_blobs.cpp): the workspace that holds it, what it
  // was made for, and its records as the plan call downloaded them. The emit call builds the
  // commitments' plan from them without waiting for the device.
  struct BlobPlan {
    const void* d_work = nullptr;
    uint32_t k = 0, n_ranges = 0;
    uint64_t total = 0, total_bytes = 0;
    std::vector<cel_blob_rec> recs;
  } blob_plan;
  // The last tx plan made on this ctx (api_txs.cpp): the workspace that holds it, what it was
  // made for and its counts. Its records stay on the device.
  struct TxPlan {
    const void* d_work = nullptr;
    uint32_t k = 0, n_ranges = 0;
    uint64_t total = 0, n_units = 0, total_bytes = 0;
  } tx_plan;
  // cel_extend_sharded's plan (buffers, streams, RCCL communicators), kept while the device
  // list, k and flags stay the same (api_multi.cpp)
  cel_shard_plan* shard_cache = nullptr;
  // cel_extend_batch_multi's host worker thread for this ctx (api_multi.cpp), made on first use
  void* worker = nullptr;
};

namespace cel {
void destroy_ctx_worker(cel_ctx* c);  // api_multi.cpp: joins the ctx's worker, if any
}
