// C ABI of the block path from txs (include/celestia_eds.h):
//   cel_block_extend      <- app/process_proposal.go:107 (ValidateBlobTx's commitments), :122
//       square.Construct, app/prepare_proposal.go:50 square.Build, app/extend_block.go:16
//       square.Construct + da.ExtendShares + NewDataAvailabilityHeader, as one call
//   cel_dev_square_build  <- the square written on the device from a layout, for callers that
//       keep the block resident
//   cel_block_extend_batch / cel_dev_square_build_batch  <- the same for a range of heights:
//       the blocks grouped by width and cut into chunks (block_batch_plan.hpp), one
//       k_square_build_batch launch per chunk, one extension and commit per width class
// The host lays the square out (square.cpp, cel::sq::square_layout: no blob byte is touched),
// the blob bytes cross PCIe once, k_square_build (square_build.hip) writes every ODS share
// into quadrant Q0 of the EDS, the extension runs in place, and the blob share commitments
// are hashed from the same device copy of the tx bytes (blob_commit.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "api_common.hpp"
#include "blob_plan.hpp"
#include "block_batch_plan.hpp"
#include "cel_internal.hpp"
#include "square_blobs.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

// A caller's layout: ascending segments that cover [0, k * k) exactly once, compact reads
// inside the compact shares, blob segments as long as their blob.
cel_status check_layout(cel_ctx* ctx, const cel_square_segment* segs, uint32_t nseg, uint32_t ncompact, uint32_t k,
                        bool* has_blob) {
  uint64_t at = 0;
  *has_blob = false;
  for (uint32_t i = 0; i < nseg; i++) {
    const cel_square_segment& s = segs[i];
    const std::string where = "segment " + std::to_string(i);
    if (s.start != at || s.count == 0) return fail(ctx, CEL_EINVAL, where + " does not continue the square");
    if (s.kind == CEL_SEG_COMPACT) {
      if (s.off > ncompact || s.count > ncompact - s.off) return fail(ctx, CEL_EINVAL, where + " reads past the compact shares");
    } else if (s.kind == CEL_SEG_BLOB) {
      if (s.len == 0 || blob::sparse_shares_needed(s.len) != s.count)
        return fail(ctx, CEL_EINVAL, where + " does not hold its blob's shares");
      *has_blob = true;
    } else if (s.kind != CEL_SEG_PAD) {
      return fail(ctx, CEL_EINVAL, where + " has an unknown kind");
    }
    at += s.count;
  }
  if (at != (uint64_t)k * k)
    return fail(ctx, CEL_EINVAL, "the segments cover " + std::to_string(at) + " shares, the square has " +
                                     std::to_string((uint64_t)k * k));
  return CEL_OK;
}

// Uploads the plan of a checked layout (the segments with their BLOB offsets lowered by sub,
// the share -> segment table, the compact shares) into scratch slot S_SQ through the
// ctx's staged upload square_up, and enqueues k_square_build on s. d_txs + (off - sub) is a blob's
// first byte. ctx->mu held, device current.
cel_status enqueue_square(cel_ctx* ctx, const uint8_t* d_txs, uint64_t sub, const cel_square_segment* segs,
                          uint32_t nseg, const uint8_t* compact, uint32_t ncompact, uint32_t k, uint8_t* d_eds,
                          hipStream_t s) {
  hipError_t e;
  const size_t seg_b = align256((size_t)nseg * sizeof(cel_square_segment));
  const size_t tab_b = align256((size_t)k * k * 4);
  const size_t bytes = seg_b + tab_b + (size_t)ncompact * kShare;
  if (!ctx->ev_sq_done && (e = hipEventCreateWithFlags(&ctx->ev_sq_done, hipEventDisableTiming)) != hipSuccess)
    return hip_fail(ctx, e, "event");
  cel_status status = CEL_OK;
  uint8_t* st = static_cast<uint8_t*>(stage_acquire(ctx, ctx->square_up, bytes, &status));
  if (!st) return status;
  cel_square_segment* hs = reinterpret_cast<cel_square_segment*>(st);
  uint32_t* tab = reinterpret_cast<uint32_t*>(st + seg_b);
  for (uint32_t i = 0; i < nseg; i++) {
    hs[i] = segs[i];
    if (hs[i].kind == CEL_SEG_BLOB) hs[i].off -= sub;
    std::fill(tab + hs[i].start, tab + hs[i].start + hs[i].count, i);
  }
  if (ncompact) std::memcpy(st + seg_b + tab_b, compact, (size_t)ncompact * kShare);
  e = hipSuccess;
  uint8_t* d_plan = static_cast<uint8_t*>(scratch(ctx, S_SQ, bytes, &e));
  if (!d_plan) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  // the previous build (perhaps on another stream) reads the device plan until ev_sq_done
  if (ctx->sq_built && (e = hipStreamWaitEvent(s, ctx->ev_sq_done, 0)) != hipSuccess) return hip_fail(ctx, e, "event");
  if ((e = hipMemcpyAsync(d_plan, st, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((status = stage_uploaded(ctx, ctx->square_up, s)) != CEL_OK) return status;
  ctx->sq_built = true;
  e = launch_square_build(d_txs, reinterpret_cast<const cel_square_segment*>(d_plan),
                          reinterpret_cast<const uint32_t*>(d_plan + seg_b), d_plan + seg_b + tab_b, d_eds, k, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "square build");
  if ((e = hipEventRecord(ctx->ev_sq_done, s)) != hipSuccess) return hip_fail(ctx, e, "event");
  return CEL_OK;
}

// One block of a chunk as the batch build reads it: a checked layout, and what its BLOB offsets
// are lowered by in the uploaded copy.
struct BatchBlock {
  const cel_square_segment* segs;
  uint32_t nseg;
  const uint8_t* compact;
  uint32_t ncompact;
};

// A chunk's uploaded plan: segments | share -> segment table | segment -> block table | block
// records | compact shares, each on a 256-byte boundary (16 suffices for the compact shares).
struct ChunkPlanBytes {
  size_t seg, tab, blk, rec, compact, total;
  ChunkPlanBytes(uint32_t nseg, uint32_t shares, uint32_t nblocks, uint32_t ncompact) {
    Carver c(nullptr);
    seg = c.off, c.take<uint8_t>((size_t)nseg * sizeof(cel_square_segment));
    tab = c.off, c.take<uint8_t>((size_t)shares * 4);
    blk = c.off, c.take<uint8_t>((size_t)nseg * 4);
    rec = c.off, c.take<uint8_t>((size_t)nblocks * sizeof(bb::BlockRec));
    compact = c.off, c.take<uint8_t>((size_t)ncompact * kShare);
    total = c.size();
  }
};

// Writes the plan of n blocks (recs[b] holding block b's bases) into st.
void fill_chunk_plan(uint8_t* st, const ChunkPlanBytes& pb, const BatchBlock* blocks, const bb::BlockRec* recs,
                     uint32_t n) {
  cel_square_segment* hs = reinterpret_cast<cel_square_segment*>(st + pb.seg);
  uint32_t* tab = reinterpret_cast<uint32_t*>(st + pb.tab);
  uint32_t* blk = reinterpret_cast<uint32_t*>(st + pb.blk);
  for (uint32_t b = 0; b < n; b++) {
    const BatchBlock& B = blocks[b];
    const bb::BlockRec& r = recs[b];
    for (uint32_t i = 0; i < B.nseg; i++) {
      const cel_square_segment& g = B.segs[i];
      hs[r.seg_base + i] = g;
      blk[r.seg_base + i] = b;
      std::fill(tab + r.first_share + g.start, tab + r.first_share + g.start + g.count, r.seg_base + i);
    }
    if (B.ncompact) std::memcpy(st + pb.compact + (size_t)r.compact_base * kShare, B.compact, (size_t)B.ncompact * kShare);
  }
  std::memcpy(st + pb.rec, recs, (size_t)n * sizeof(bb::BlockRec));
}

// Uploads a filled chunk plan from page-locked st into d_plan and enqueues k_square_build_batch
// on s. The caller keeps the staged upload's and the device plan's rules (enqueue_square).
cel_status enqueue_chunk_build(cel_ctx* ctx, const uint8_t* d_txs, const uint8_t* st, uint8_t* d_plan,
                               const ChunkPlanBytes& pb, uint32_t shares, uint8_t* d_eds, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemcpyAsync(d_plan, st, pb.total, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  e = launch_square_build_batch(d_txs, reinterpret_cast<const cel_square_segment*>(d_plan + pb.seg),
                                reinterpret_cast<const uint32_t*>(d_plan + pb.tab),
                                reinterpret_cast<const uint32_t*>(d_plan + pb.blk),
                                reinterpret_cast<const bb::BlockRec*>(d_plan + pb.rec), d_plan + pb.compact, d_eds,
                                shares, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "square build");
  return CEL_OK;
}

// What the host entry keeps of a chunk besides the planner's figures.
struct ChunkIo {
  ChunkPlanBytes pb{0, 0, 0, 0};
  size_t plan_at = 0;            // its plan in the staged upload and in S_SQ
  uint64_t up_b = 0;             // blob bytes uploaded
  const uint8_t* direct = nullptr;  // page-locked txs: the one span that goes up in place
  size_t gather_at = 0;          // else: where its gathered bytes lie in host staging
  std::vector<size_t> run_off;   // each class run's ResultBlock in the result region
  size_t out_b = 0, res_b = 0;   // the commitments' offset; the region's bytes
  size_t res_at = 0;             // the region in host staging
  size_t nmt_b = 0;
  uint32_t nb = 0;               // commitments
  uint64_t commit_shares = 0;
};

}  // namespace

extern "C" {

cel_status cel_dev_square_build(cel_ctx* ctx, const void* d_txs, const cel_square_segment* segments,
                                uint32_t n_segments, const uint8_t* compact, uint32_t n_compact_shares, uint32_t k,
                                void* d_eds, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!segments || !n_segments || !d_eds || (n_compact_shares && !compact)) return fail(ctx, CEL_EINVAL, "nil argument");
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if ((uintptr_t)d_eds & 15u) return fail(ctx, CEL_EINVAL, "the EDS buffer must be 16-byte aligned");
  bool has_blob;
  if ((st = check_layout(ctx, segments, n_segments, n_compact_shares, k, &has_blob)) != CEL_OK) return st;
  if (has_blob && !d_txs) return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  return enqueue_square(ctx, static_cast<const uint8_t*>(d_txs), 0, segments, n_segments, compact, n_compact_shares, k,
                        static_cast<uint8_t*>(d_eds), pick_stream(ctx, stream));
}

cel_status cel_block_extend(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                            uint32_t max_square_size, uint32_t subtree_root_threshold, uint32_t greedy,
                            uint32_t* k_out, uint8_t* included, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                            uint8_t* eds_out, uint64_t eds_cap, uint8_t* commitments, uint32_t* commit_tx_index,
                            uint32_t commit_cap, uint32_t* n_commit, uint32_t flags) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!k_out || !row_roots || !col_roots || !dah || (ntx && (!txs || !tx_lens)) ||
      (commit_cap && (!commitments || !commit_tx_index || !n_commit)))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (!max_square_size || !is_pow2(max_square_size)) return fail(ctx, CEL_EINVAL, "max square size must be a power of 2");
  if (subtree_root_threshold == 0) return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  if (max_square_size > 512)
    return fail(ctx, CEL_ETOOBIG, "square width " + std::to_string(max_square_size) + " exceeds the device path (512)");

  // the square's layout and every blob of every BlobTx: host work, no blob byte touched
  sq::Layout L;
  std::vector<sq::BlobRef> all;
  cel_status st =
      sq::square_layout(txs, tx_lens, ntx, max_square_size, subtree_root_threshold, greedy, included, L, &all);
  if (st) return fail(ctx, st, cel_square_last_error());
  const uint32_t k = L.k;
  *k_out = k;
  if (n_commit) *n_commit = (uint32_t)all.size();
  const size_t eds_b = (size_t)4 * k * k * kShare;
  const ext::ResultBlock rb(k, 1);
  if (eds_out && eds_cap < eds_b)
    return fail(ctx, CEL_EINVAL,
                "EDS output holds " + std::to_string(eds_cap) + " bytes, the square needs " + std::to_string(eds_b));
  const uint32_t nb = commit_cap ? (uint32_t)all.size() : 0;
  std::vector<CommitItem> items(nb);
  uint64_t commit_shares = 0;
  if (nb) {
    if (nb > commit_cap)
      return fail(ctx, CEL_EINVAL,
                  "output holds " + std::to_string(commit_cap) + " blobs, the txs carry " + std::to_string(nb));
    for (uint32_t i = 0; i < nb; i++) {
      if ((st = commit_check_blob(ctx, i, all[i].len, all[i].share_version)) != CEL_OK) return st;
      items[i] = CommitItem{all[i].ns, nullptr, all[i].len};
      commit_tx_index[i] = all[i].tx_index;
      commit_shares += blob::sparse_shares_needed(all[i].len);
    }
  }

  // the one range of txs that holds every blob byte the device reads: the kept blobs'
  // (the square) and, with commitments, every blob's. Normal txs in front of it stay on the
  // host (their content travels inside the compact shares); with greedy = 0 it lies inside
  // the blob txs' contiguous tail.
  uint64_t lo = UINT64_MAX, hi = 0;
  for (const cel_square_segment& s : L.segs)
    if (s.kind == CEL_SEG_BLOB) lo = std::min<uint64_t>(lo, s.off), hi = std::max<uint64_t>(hi, s.off + s.len);
  for (uint32_t i = 0; i < nb; i++) lo = std::min(lo, all[i].off), hi = std::max(hi, all[i].off + all[i].len);
  const uint64_t up_b = hi > lo ? hi - lo : 0;
  std::vector<uint64_t> offs(nb);
  for (uint32_t i = 0; i < nb; i++) offs[i] = all[i].off - lo;

  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream, d = ctx->dl[0];
  hipError_t e = hipSuccess;
  // the commitments follow the result block on a 256-byte boundary
  const size_t out_b = align256(rb.bytes()), res_b = out_b + (size_t)nb * 32;
  const size_t nmt_b = align256(nmt_workspace_size(k, 1));
  const bool direct = up_b && page_locked(txs);
  // + 8: the last dword a lane may touch starts inside the data; keep it inside the buffer
  uint8_t* d_in = static_cast<uint8_t*>(scratch(ctx, S_IN, up_b + 8, &e));
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  uint8_t* d_work =
      static_cast<uint8_t*>(scratch(ctx, S_WORK, nmt_b + (nb ? commit_workspace_bound(commit_shares, nb) : 0), &e));
  uint8_t* d_out = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, res_b, &e));
  if (!d_in || !d_eds || !d_work || !d_out) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  uint8_t* h_out = static_cast<uint8_t*>(host_stage(ctx, res_b + (direct ? 0 : up_b)));
  if (!h_out) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  int32_t* d_st = reinterpret_cast<int32_t*>(d_out + rb.status());

  if (up_b) {
    const uint8_t* src = txs + lo;
    if (!direct) {
      std::memcpy(h_out + res_b, src, up_b);
      src = h_out + res_b;
    }
    if ((e = hipMemcpyAsync(d_in, src, up_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  }
  if ((st = enqueue_square(ctx, d_in, lo == UINT64_MAX ? 0 : lo, L.segs.data(), (uint32_t)L.segs.size(),
                           L.compact.data(), (uint32_t)(L.compact.size() / kShare), k, d_eds, s)) != CEL_OK)
    return st;
  if ((e = launch_extend(nullptr, d_eds, k, 1, ctx->tables, s)) != hipSuccess) return hip_fail(ctx, e, "extend square");
  if (eds_out && (e = stream_after(d, ctx->ev_cols, s)) != hipSuccess) return hip_fail(ctx, e, "event");
  if ((e = launch_commit(d_eds, k, 1, d_out + rb.row_roots(), d_out + rb.col_roots(), d_out + rb.dah(), d_st, d_work,
                         (flags & CEL_FLAG_ORDER_CHECK) != 0, s)) != hipSuccess)
    return hip_fail(ctx, e, "commit square");
  if (nb && (st = commit_enqueue(ctx, d_in, 0, offs.data(), items.data(), nb, subtree_root_threshold, d_out + out_b,
                                 d_work + nmt_b, s)) != CEL_OK)
    return st;
  // roots, data root, status and the commitments in one copy into page-locked staging
  if ((e = hipMemcpyAsync(h_out, d_out, res_b, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
  if (eds_out) {
    // after every launch is enqueued: a copy into pageable memory blocks the calling thread
    e = copy_back(eds_out, d_eds, ext::copy_back_rects(k, 0, 2 * k, (flags & CEL_FLAG_PARITY_ONLY) != 0), d);
    if (e == hipSuccess) e = stream_after(s, ctx->ev_dl, d);
    if (e != hipSuccess) return hip_fail(ctx, e, "D2H");
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  if (nb) std::memcpy(commitments, h_out + out_b, (size_t)nb * 32);
  return order_status(ctx, rb.unpack(h_out, row_roots, col_roots, dah, nullptr));
}

cel_status cel_dev_square_build_batch(cel_ctx* ctx, const void* d_txs, const uint64_t* tx_base, uint32_t n_blocks,
                                      const cel_square_segment* segments, const uint32_t* n_segments,
                                      const uint8_t* compact, const uint32_t* n_compact_shares, const uint32_t* k,
                                      void* d_eds, const uint64_t* eds_off, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_blocks || !tx_base || !segments || !n_segments || !n_compact_shares || !k || !d_eds || !eds_off)
    return fail(ctx, CEL_EINVAL, "nil argument");
  if ((uintptr_t)d_eds & 15u) return fail(ctx, CEL_EINVAL, "the EDS buffer must be 16-byte aligned");
  std::vector<BatchBlock> blocks(n_blocks);
  std::vector<bb::BlockRec> recs(n_blocks);
  uint64_t shares = 0, nseg = 0, ncompact = 0;
  bool any_blob = false;
  for (uint32_t b = 0; b < n_blocks; b++) {
    const std::string where = "block " + std::to_string(b) + ": ";
    cel_status st = validate_square(ctx, k[b], kShare);
    if (st == CEL_OK && !n_segments[b]) st = fail(ctx, CEL_EINVAL, "nil argument");
    if (st == CEL_OK && n_compact_shares[b] && !compact) st = fail(ctx, CEL_EINVAL, "nil argument");
    if (st == CEL_OK && (eds_off[b] & 15u)) st = fail(ctx, CEL_EINVAL, "the EDS offset must be a multiple of 16");
    bool has_blob = false;
    if (st == CEL_OK) st = check_layout(ctx, segments + nseg, n_segments[b], n_compact_shares[b], k[b], &has_blob);
    if (st != CEL_OK) return fail(ctx, st, where + ctx->last_error);
    any_blob |= has_blob;
    blocks[b] = BatchBlock{segments + nseg, n_segments[b], compact ? compact + ncompact * kShare : nullptr,
                           n_compact_shares[b]};
    recs[b] = bb::BlockRec{eds_off[b], tx_base[b], (uint32_t)shares, (uint32_t)nseg, (uint32_t)ncompact,
                           bb::log2u(k[b])};
    shares += (uint64_t)k[b] * k[b];
    nseg += n_segments[b];
    ncompact += n_compact_shares[b];
    if (shares >= (1u << 27) || nseg > UINT32_MAX || ncompact > UINT32_MAX)
      return fail(ctx, CEL_ETOOBIG, "the blocks hold 2^27 shares or more");
  }
  if (any_blob && !d_txs) return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  hipStream_t s = pick_stream(ctx, stream);
  const ChunkPlanBytes pb((uint32_t)nseg, (uint32_t)shares, n_blocks, (uint32_t)ncompact);
  hipError_t e;
  if (!ctx->ev_sq_done && (e = hipEventCreateWithFlags(&ctx->ev_sq_done, hipEventDisableTiming)) != hipSuccess)
    return hip_fail(ctx, e, "event");
  cel_status status = CEL_OK;
  uint8_t* st = static_cast<uint8_t*>(stage_acquire(ctx, ctx->square_up, pb.total, &status));
  if (!st) return status;
  fill_chunk_plan(st, pb, blocks.data(), recs.data(), n_blocks);
  e = hipSuccess;
  uint8_t* d_plan = static_cast<uint8_t*>(scratch(ctx, S_SQ, pb.total, &e));
  if (!d_plan) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  // the previous build (perhaps on another stream) reads the device plan until ev_sq_done
  if (ctx->sq_built && (e = hipStreamWaitEvent(s, ctx->ev_sq_done, 0)) != hipSuccess) return hip_fail(ctx, e, "event");
  ctx->sq_built = true;
  status = enqueue_chunk_build(ctx, static_cast<const uint8_t*>(d_txs), st, d_plan, pb, (uint32_t)shares,
                               static_cast<uint8_t*>(d_eds), s);
  // the copy out of st may be enqueued even where the launch failed
  const cel_status up = stage_uploaded(ctx, ctx->square_up, s);
  if (status != CEL_OK) return status;
  if (up != CEL_OK) return up;
  if ((e = hipEventRecord(ctx->ev_sq_done, s)) != hipSuccess) return hip_fail(ctx, e, "event");
  return CEL_OK;
}

cel_status cel_block_extend_batch(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens, const uint32_t* block_ntx,
                                  uint32_t n_blocks, uint32_t max_square_size, uint32_t subtree_root_threshold,
                                  uint32_t greedy, uint32_t host_threads, uint64_t max_eds_bytes, uint32_t* k_out,
                                  int32_t* status_out, uint8_t* included, uint8_t* row_roots, uint8_t* col_roots,
                                  uint32_t* root_off, uint64_t roots_cap, uint8_t* dah, uint8_t* commitments,
                                  uint32_t* commit_block, uint32_t* commit_tx_index, uint32_t commit_cap,
                                  uint32_t* n_commit, float* phase_ms, uint32_t flags) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const uint32_t n = n_blocks;
  if (!n || !block_ntx || !k_out || !status_out || !row_roots || !col_roots || !root_off || !dah ||
      (commit_cap && (!commitments || !commit_block || !commit_tx_index || !n_commit)))
    return fail(ctx, CEL_EINVAL, "nil argument");
  std::vector<uint64_t> tx0(n + 1, 0);  // each block's first tx
  for (uint32_t i = 0; i < n; i++) tx0[i + 1] = tx0[i] + block_ntx[i];
  if (tx0[n] && (!txs || !tx_lens)) return fail(ctx, CEL_EINVAL, "nil argument");
  if (!max_square_size || !is_pow2(max_square_size)) return fail(ctx, CEL_EINVAL, "max square size must be a power of 2");
  if (subtree_root_threshold == 0) return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  if (max_square_size > 512)
    return fail(ctx, CEL_ETOOBIG, "square width " + std::to_string(max_square_size) + " exceeds the device path (512)");
  std::vector<uint64_t> boff(n + 1, 0);  // each block's first byte
  for (uint32_t i = 0; i < n; i++) {
    uint64_t b = 0;
    for (uint64_t t = tx0[i]; t < tx0[i + 1]; t++) b += tx_lens[t];
    boff[i + 1] = boff[i] + b;
  }

  // every block's layout and every blob of its BlobTxs: host work, no blob byte touched. The
  // layout's message is per thread, so a worker copies it before it takes the next block.
  const auto t_layout = std::chrono::steady_clock::now();
  std::vector<sq::Layout> L(n);
  std::vector<std::vector<sq::BlobRef>> all(n);
  std::vector<int32_t> bst(n, CEL_OK);
  std::vector<std::string> msg(n);
  std::vector<uint8_t> inc(tx0[n] + 1, 0);
  {
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
      for (uint32_t i; (i = next.fetch_add(1)) < n;) {
        bst[i] = sq::square_layout(txs ? txs + boff[i] : nullptr, tx_lens ? tx_lens + tx0[i] : nullptr, block_ntx[i],
                                   max_square_size, subtree_root_threshold, greedy, inc.data() + tx0[i], L[i], &all[i]);
        if (bst[i] != CEL_OK) msg[i] = cel_square_last_error();
      }
    };
    const uint32_t nthreads = std::min(std::max(host_threads, 1u), n);
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nthreads; t++) pool.emplace_back(work);
    work();
    for (std::thread& t : pool) t.join();
  }
  const float layout_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_layout).count();

  // a block whose commitments cannot be computed fails as a whole, as in the single call
  uint64_t total_blobs = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (bst[i] != CEL_OK) continue;
    for (uint32_t j = 0; commit_cap && j < all[i].size() && bst[i] == CEL_OK; j++)
      if ((bst[i] = commit_check_blob(ctx, j, all[i][j].len, all[i][j].share_version)) != CEL_OK) msg[i] = ctx->last_error;
    if (bst[i] == CEL_OK) total_blobs += all[i].size();
  }
  if (total_blobs > UINT32_MAX) return fail(ctx, CEL_ETOOBIG, "too many blobs");
  if (n_commit) *n_commit = (uint32_t)total_blobs;
  if (commit_cap && total_blobs > commit_cap)
    return fail(ctx, CEL_EINVAL,
                "output holds " + std::to_string(commit_cap) + " blobs, the txs carry " + std::to_string(total_blobs));
  uint64_t total_roots = 0;
  for (uint32_t i = 0; i < n; i++)
    if (bst[i] == CEL_OK) total_roots += 2 * L[i].k;
  if (total_roots > roots_cap)
    return fail(ctx, CEL_EINVAL,
                "roots output holds " + std::to_string(roots_cap) + " nodes, the blocks need " + std::to_string(total_roots));

  // the plan, and what of the outputs the host knows already
  std::vector<bb::BlockIn> in(n);
  for (uint32_t i = 0; i < n; i++)
    in[i] = bb::BlockIn{L[i].k, bst[i], (uint32_t)L[i].segs.size(), (uint32_t)(L[i].compact.size() / kShare)};
  bb::Plan plan = bb::plan_blocks(in.data(), n, max_eds_bytes);
  std::vector<uint32_t> blob0(n + 1, 0);  // each block's first commitment in the flat output
  const bool want_commit = commit_cap != 0;
  for (uint32_t i = 0, at = 0; i < n; i++) {
    const bool ok = bst[i] == CEL_OK;
    k_out[i] = ok ? L[i].k : 0;
    status_out[i] = bst[i];
    root_off[i] = at;
    at += ok ? 2 * L[i].k : 0;
    root_off[i + 1] = at;
    std::memset(dah + (size_t)i * 32, 0, 32);
    if (!ok) std::fill(inc.begin() + tx0[i], inc.begin() + tx0[i + 1], 0);
    blob0[i + 1] = blob0[i] + (ok && want_commit ? (uint32_t)all[i].size() : 0);
    for (uint32_t j = blob0[i]; j < blob0[i + 1]; j++) {
      commit_block[j] = i;
      commit_tx_index[j] = all[i][j - blob0[i]].tx_index;
    }
  }
  if (included && tx0[n]) std::memcpy(included, inc.data(), tx0[n]);
  ctx->block_errors = msg;
  // the call's result: the first failed block in block order (a device status may still join)
  auto first_failure = [&]() -> cel_status {
    for (uint32_t i = 0; i < n; i++)
      if (bst[i] != CEL_OK) return fail(ctx, (cel_status)bst[i], "block " + std::to_string(i) + ": " + ctx->block_errors[i]);
    return CEL_OK;
  };
  if (phase_ms) phase_ms[0] = layout_ms, phase_ms[1] = 0.f;
  if (plan.chunks.empty()) return first_failure();

  // Per chunk: the one range of each block's txs that holds every blob byte the device reads
  // (as in cel_block_extend), where those ranges go in the chunk's device copy, the result
  // region and the workspaces. Page-locked txs go up in place as one span from the first
  // range's start to the last one's end when that is at most twice the bytes needed (the
  // blocks of a chunk are class-ordered, so their ranges may lie anywhere among the txs);
  // otherwise the ranges are gathered into page-locked staging.
  const bool locked = boff[n] && page_locked(txs);
  const uint32_t nchunks = (uint32_t)plan.chunks.size();
  std::vector<ChunkIo> io(nchunks);
  std::vector<uint64_t> lo(n, 0), hi(n, 0), dev_at(n, 0);  // per caller block: its range, and its place on the device
  size_t plan_total = 0, host_total = 0, in_max = 0, eds_max = 0, work_max = 0, res_max = 0;
  for (uint32_t c = 0; c < nchunks; c++) {
    const bb::Chunk& ch = plan.chunks[c];
    ChunkIo& o = io[c];
    uint64_t need = 0, span_lo = UINT64_MAX, span_hi = 0;
    for (uint32_t q = ch.first; q < ch.first + ch.count; q++) {
      const uint32_t i = plan.order[q];
      uint64_t l = UINT64_MAX, h = 0;
      for (const cel_square_segment& s : L[i].segs)
        if (s.kind == CEL_SEG_BLOB) l = std::min<uint64_t>(l, s.off), h = std::max<uint64_t>(h, s.off + s.len);
      if (want_commit)
        for (const sq::BlobRef& b : all[i]) l = std::min(l, b.off), h = std::max(h, b.off + b.len);
      if (h > l) {
        lo[i] = l, hi[i] = h;
        need += h - l;
        span_lo = std::min(span_lo, boff[i] + l), span_hi = std::max(span_hi, boff[i] + h);
      }
      o.nb += want_commit ? (uint32_t)all[i].size() : 0;
      if (want_commit)
        for (const sq::BlobRef& b : all[i]) o.commit_shares += blob::sparse_shares_needed(b.len);
    }
    const bool direct = locked && need && span_hi - span_lo <= 2 * need;
    o.up_b = direct ? span_hi - span_lo : need;
    if (direct) o.direct = txs + span_lo;
    uint64_t at = 0;
    for (uint32_t q = ch.first; q < ch.first + ch.count; q++) {
      const uint32_t i = plan.order[q];
      dev_at[i] = direct ? boff[i] + lo[i] - span_lo : at;
      at += hi[i] - lo[i];
      // a BLOB offset counts from the block's first tx byte: that byte's place in the device copy
      plan.recs[q].txs_base = dev_at[i] - lo[i];
    }
    o.pb = ChunkPlanBytes(ch.nseg, ch.shares, ch.count, ch.ncompact);
    o.plan_at = plan_total;
    plan_total += o.pb.total;
    size_t res = 0;
    for (uint32_t r = ch.run0; r < ch.run0 + ch.nruns; r++) {
      o.run_off.push_back(res);
      res += align256(ext::ResultBlock(plan.runs[r].k, plan.runs[r].count).bytes());
      o.nmt_b = std::max(o.nmt_b, align256(nmt_workspace_size(plan.runs[r].k, plan.runs[r].count)));
    }
    o.out_b = res;
    o.res_b = align256(res + (size_t)o.nb * 32);
    o.res_at = host_total;
    host_total += o.res_b;
    if (!direct) o.gather_at = host_total, host_total += align256(o.up_b);
    in_max = std::max<size_t>(in_max, o.up_b);
    eds_max = std::max<size_t>(eds_max, ch.eds_bytes);
    work_max = std::max(work_max, o.nmt_b + (o.nb ? commit_workspace_bound(o.commit_shares, o.nb) : 0));
    res_max = std::max(res_max, o.res_b);
  }

  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  // The chunks run one after another on s, so one buffer of each kind, sized for the largest
  // chunk, serves them all in stream order; the plans of all chunks lie side by side (host and
  // device), and every chunk's results and gathered bytes have a place of their own in host
  // staging, because the host reads and writes them without waiting for the stream.
  // + 8: the last dword a lane may touch starts inside the data; keep it inside the buffer
  uint8_t* d_in = static_cast<uint8_t*>(scratch(ctx, S_IN, in_max + 8, &e));
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_max, &e));
  uint8_t* d_work = static_cast<uint8_t*>(scratch(ctx, S_WORK, work_max, &e));
  uint8_t* d_out = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, res_max, &e));
  uint8_t* d_plan = static_cast<uint8_t*>(scratch(ctx, S_SQ, plan_total, &e));
  if (!d_in || !d_eds || !d_work || !d_out || !d_plan) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  uint8_t* h = static_cast<uint8_t*>(host_stage(ctx, host_total));
  if (!h) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  if (!ctx->ev_sq_done && (e = hipEventCreateWithFlags(&ctx->ev_sq_done, hipEventDisableTiming)) != hipSuccess)
    return hip_fail(ctx, e, "event");
  cel_status st = CEL_OK;
  uint8_t* hp = static_cast<uint8_t*>(stage_acquire(ctx, ctx->square_up, plan_total, &st));
  if (!hp) return st;
  std::vector<BatchBlock> blocks;
  for (uint32_t c = 0; c < nchunks; c++) {
    const bb::Chunk& ch = plan.chunks[c];
    blocks.clear();
    for (uint32_t q = ch.first; q < ch.first + ch.count; q++) {
      const sq::Layout& l = L[plan.order[q]];
      blocks.push_back(BatchBlock{l.segs.data(), (uint32_t)l.segs.size(), l.compact.data(), (uint32_t)(l.compact.size() / kShare)});
    }
    fill_chunk_plan(hp + io[c].plan_at, io[c].pb, blocks.data(), plan.recs.data() + ch.first, ch.count);
  }

  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (phase_ms && ((e = hipEventCreate(&t0)) != hipSuccess || (e = hipEventCreate(&t1)) != hipSuccess)) {
    if (t0) (void)hipEventDestroy(t0);
    return hip_fail(ctx, e, "event");
  }
  // from here on every way out passes `done`, which frees the timing events
  auto done = [&](cel_status r) {
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    return r;
  };
  // the previous build (perhaps on another stream) reads the device plans until ev_sq_done
  if (ctx->sq_built && (e = hipStreamWaitEvent(s, ctx->ev_sq_done, 0)) != hipSuccess) return done(hip_fail(ctx, e, "event"));
  ctx->sq_built = true;
  if (t0 && (e = hipEventRecord(t0, s)) != hipSuccess) return done(hip_fail(ctx, e, "event"));
  const bool order_check = (flags & CEL_FLAG_ORDER_CHECK) != 0;
  std::vector<CommitItem> items;
  std::vector<uint64_t> offs;
  bool staged = false;  // a copy out of hp has been enqueued
  auto enqueue_chunk = [&](uint32_t c) -> cel_status {
    const bb::Chunk& ch = plan.chunks[c];
    const ChunkIo& o = io[c];
    if (o.up_b) {
      const uint8_t* src = o.direct;
      if (!src) {
        uint8_t* dst = h + o.gather_at;
        for (uint32_t q = ch.first; q < ch.first + ch.count; q++) {
          const uint32_t i = plan.order[q];
          if (hi[i] > lo[i]) std::memcpy(dst + dev_at[i], txs + boff[i] + lo[i], hi[i] - lo[i]);
        }
        src = dst;
      }
      if ((e = hipMemcpyAsync(d_in, src, o.up_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
    }
    staged = true;
    cel_status r = enqueue_chunk_build(ctx, d_in, hp + o.plan_at, d_plan + o.plan_at, o.pb, ch.shares, d_eds, s);
    if (r != CEL_OK) return r;
    for (uint32_t ri = 0; ri < ch.nruns; ri++) {
      const bb::ClassRun& run = plan.runs[ch.run0 + ri];
      uint8_t* eds = d_eds + plan.recs[run.first].eds_off;  // the run's EDSs lie back to back from here
      const ext::ResultBlock rb(run.k, run.count);
      uint8_t* out = d_out + o.run_off[ri];
      if ((e = launch_extend(nullptr, eds, run.k, run.count, ctx->tables, s)) != hipSuccess)
        return hip_fail(ctx, e, "extend square");
      if ((e = launch_commit(eds, run.k, run.count, out + rb.row_roots(), out + rb.col_roots(), out + rb.dah(),
                             reinterpret_cast<int32_t*>(out + rb.status()), d_work, order_check, s)) != hipSuccess)
        return hip_fail(ctx, e, "commit square");
    }
    if (o.nb) {
      items.clear();
      offs.clear();
      for (uint32_t q = ch.first; q < ch.first + ch.count; q++) {
        const uint32_t i = plan.order[q];
        for (const sq::BlobRef& b : all[i]) {
          items.push_back(CommitItem{b.ns, nullptr, b.len});
          offs.push_back(dev_at[i] + (b.off - lo[i]));
        }
      }
      if ((r = commit_enqueue(ctx, d_in, 0, offs.data(), items.data(), o.nb, subtree_root_threshold, d_out + o.out_b,
                              d_work + o.nmt_b, s)) != CEL_OK)
        return r;
    }
    // roots, data roots, statuses and the commitments of the chunk in one copy
    if ((e = hipMemcpyAsync(h + o.res_at, d_out, o.res_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_fail(ctx, e, "D2H");
    return CEL_OK;
  };
  for (uint32_t c = 0; c < nchunks && st == CEL_OK; c++) st = enqueue_chunk(c);
  if (staged) {
    const cel_status up = stage_uploaded(ctx, ctx->square_up, s);
    if (st == CEL_OK) st = up;
    if ((e = hipEventRecord(ctx->ev_sq_done, s)) != hipSuccess && st == CEL_OK) st = hip_fail(ctx, e, "event");
  }
  if (st == CEL_OK && t1 && (e = hipEventRecord(t1, s)) != hipSuccess) st = hip_fail(ctx, e, "event");
  // also where an enqueue failed: the host staging of what was enqueued must not be reused under it
  e = hipStreamSynchronize(s);
  if (st != CEL_OK) return done(st);
  if (e != hipSuccess) return done(hip_fail(ctx, e, "sync"));
  if (t1 && hipEventElapsedTime(&phase_ms[1], t0, t1) != hipSuccess) phase_ms[1] = 0.f;

  for (uint32_t c = 0; c < nchunks; c++) {
    const bb::Chunk& ch = plan.chunks[c];
    const ChunkIo& o = io[c];
    const uint8_t* res = h + o.res_at;
    for (uint32_t ri = 0; ri < ch.nruns; ri++) {
      const bb::ClassRun& run = plan.runs[ch.run0 + ri];
      const ext::ResultBlock rb(run.k, run.count);
      const uint8_t* b = res + o.run_off[ri];
      const size_t sq_roots = (size_t)2 * run.k * kNode;
      for (uint32_t j = 0; j < run.count; j++) {
        const uint32_t i = plan.order[run.first + j];
        std::memcpy(row_roots + (size_t)root_off[i] * kNode, b + rb.row_roots() + j * sq_roots, sq_roots);
        std::memcpy(col_roots + (size_t)root_off[i] * kNode, b + rb.col_roots() + j * sq_roots, sq_roots);
        std::memcpy(dah + (size_t)i * 32, b + rb.dah() + (size_t)j * 32, 32);
        int32_t dst;
        std::memcpy(&dst, b + rb.status() + (size_t)j * 4, 4);
        if (dst != CEL_OK) {
          status_out[i] = bst[i] = dst;
          ctx->block_errors[i] = dst == CEL_EORDER ? kOrderMessage : "device status";
        }
      }
    }
    const uint8_t* com = res + o.out_b;
    for (uint32_t q = ch.first; o.nb && q < ch.first + ch.count; q++) {
      const uint32_t i = plan.order[q];
      const size_t nbytes = (size_t)all[i].size() * 32;
      if (nbytes) std::memcpy(commitments + (size_t)blob0[i] * 32, com, nbytes);
      com += nbytes;
    }
  }
  return done(first_failure());
}

const char* cel_block_batch_error(cel_ctx* ctx, uint32_t block) {
  if (!ctx) return "";
  std::lock_guard<std::mutex> lock(ctx->mu);
  return block < ctx->block_errors.size() ? ctx->block_errors[block].c_str() : "";
}

}  // extern "C"
