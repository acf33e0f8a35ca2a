// C ABI of the block path from txs (include/celestia_eds.h):
//   cel_block_extend      <- app/process_proposal.go:107 (ValidateBlobTx's commitments), :122
//       square.Construct, app/prepare_proposal.go:50 square.Build, app/extend_block.go:16
//       square.Construct + da.ExtendShares + NewDataAvailabilityHeader, as one call
//   cel_dev_square_build  <- the square written on the device from a layout, for callers that
//       keep the block resident
// The host lays the square out (square.cpp, cel::sq::square_layout: no blob byte is touched),
// the blob bytes cross PCIe once, k_square_build (square_build.hip) writes every ODS share
// into quadrant Q0 of the EDS, the extension runs in place, and the blob share commitments
// are hashed from the same device copy of the tx bytes (blob_commit.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "blob_plan.hpp"
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

}  // extern "C"
