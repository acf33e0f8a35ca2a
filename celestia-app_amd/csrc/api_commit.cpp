// C ABI of the blob share commitments computed from blob bytes (include/celestia_eds.h):
//   cel_create_commitments / cel_dev_create_commitments  <- go-square v1.1.0
//       inclusion.CreateCommitments, as blobtypes.ValidateBlobTx recomputes them for every
//       blob of a BlobTx (x/blob/types/blob_tx.go:96-105) before the square exists
//   cel_blob_tx_commitments  <- the same for every blob of every BlobTx of a block, one
//       device batch (the loop of app/process_proposal.go:101-110)
//   cel_blob_subtree_sizes   <- inclusion.MerkleMountainRangeSizes(SparseSharesNeeded(len),
//       SubTreeWidth(...)), host only
// The host plans the leaf slots (blob_plan.hpp); every hash runs in blob_commit.hip. Only
// blob bytes and the plan tables are uploaded: shares are never materialised.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "blob_plan.hpp"
#include "square_blobs.hpp"
#include "cel_internal.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

constexpr uint64_t kChunkBytes = 64ull << 20;  // blob bytes per device batch of the host entries

using Item = CommitItem;

}  // namespace

namespace cel {
namespace abi {

// Workspace for any plan of nblobs blobs with total_shares shares: a blob's alignment gap
// is below its width, and SubTreeWidth(n) - 1 <= n, so the slots stay below twice the
// shares (+ one tile of rounding); there is at most one root per share.
size_t commit_workspace_bound(uint64_t total_shares, uint32_t nblobs) {
  return blob_commit_workspace_size(2 * total_shares + blob::kTile, total_shares, nblobs);
}

cel_status commit_check_blob(cel_ctx* ctx, uint32_t i, uint64_t len, uint32_t share_version) {
  if (len == 0) return fail(ctx, CEL_EINVAL, "blob " + std::to_string(i) + " has no data");
  if (share_version != 0) return fail(ctx, CEL_EINVAL, "unsupported share version " + std::to_string(share_version));
  if (blob::sparse_shares_needed(len) > blob::kMaxShares)
    return fail(ctx, CEL_ETOOBIG, "blob " + std::to_string(i) + " exceeds the device path (2^20 shares)");
  return CEL_OK;
}

// Plans items [0, nb) whose bytes lie in d_data back to back from base_off on (offs ==
// nullptr) or at byte offsets offs[i], uploads the tables into d_work's head and enqueues the
// kernels on s. ctx->mu held, device current.
cel_status commit_enqueue(cel_ctx* ctx, const uint8_t* d_data, uint64_t base_off, const uint64_t* offs,
                          const CommitItem* items, uint32_t nb, uint32_t threshold, uint8_t* d_out, void* d_work,
                          hipStream_t s) {
  blob::Plan plan;
  plan.recs.reserve(nb);
  uint64_t off = base_off;
  for (uint32_t i = 0; i < nb; i++) {
    blob::plan_add(plan, items[i].ns, offs ? offs[i] : off, items[i].len, threshold);
    off += items[i].len;
    if (plan.slots + blob::kTile > blob::kMaxSlots)
      return fail(ctx, CEL_ETOOBIG, "too many shares for one device batch");
  }
  const uint64_t slots = (plan.slots + blob::kTile - 1) / blob::kTile * blob::kTile;
  // the head of blob_work's layout (blob_commit.hip): the records, then the slot table
  const size_t rec_bytes = align256((size_t)nb * sizeof(blob::Rec));
  const size_t bytes = rec_bytes + slots * 4;
  cel_status status = CEL_OK;
  uint8_t* st = static_cast<uint8_t*>(plan_stage(ctx, bytes, &status));
  if (!st) return status;
  std::memset(st, 0, rec_bytes);
  std::memcpy(st, plan.recs.data(), (size_t)nb * sizeof(blob::Rec));
  blob::plan_finish(plan, reinterpret_cast<uint32_t*>(st + rec_bytes));
  hipError_t e;
  if ((e = hipMemcpyAsync(d_work, st, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((status = plan_uploaded(ctx, s)) != CEL_OK) return status;
  // Measurement aid (tools/commit_bench.py --leaf-ab): CEL_COMMIT_LEAF=expanded runs the leaf
  // stage's A/B partner, which first writes every share into ctx scratch (512 B per slot).
  uint32_t* d_shares = nullptr;
  const char* leaf = std::getenv("CEL_COMMIT_LEAF");
  if (leaf && std::strcmp(leaf, "expanded") == 0) {
    e = hipSuccess;
    d_shares = static_cast<uint32_t*>(scratch(ctx, S_EDS, slots * kShare, &e));
    if (!d_shares) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  }
  Range r("blob_commit");
  if ((e = launch_blob_commit(d_data, plan, d_work, d_out, s, d_shares)) != hipSuccess)
    return hip_fail(ctx, e, "blob commit");
  return CEL_OK;
}

// Is p page-locked host memory (cel_host_alloc, hipHostMalloc / hipHostRegister)?
bool page_locked(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky "invalid value" of a pageable pointer
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

}  // namespace abi
}  // namespace cel

namespace {

// Commitments of host blobs, in chunks of whole blobs of about kChunkBytes. contiguous: the
// items' bytes lie back to back from items[0].data on (one copy per chunk, straight from
// the caller's memory if that is page-locked); otherwise each blob is packed into the
// page-locked staging buffer. ctx->mu held.
cel_status run_host(cel_ctx* ctx, const std::vector<Item>& items, bool contiguous, uint32_t threshold,
                    uint8_t* commitments) {
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const bool direct = contiguous && page_locked(items[0].data);
  const uint32_t n = (uint32_t)items.size();
  for (uint32_t b0 = 0; b0 < n;) {
    uint32_t b1 = b0;
    uint64_t bytes = 0, shares = 0;
    do {
      bytes += items[b1].len;
      shares += blob::sparse_shares_needed(items[b1].len);
      b1++;
    } while (b1 < n && bytes + items[b1].len <= kChunkBytes);
    const uint32_t nb = b1 - b0;
    hipError_t e = hipSuccess;
    // + 8: the last dword a lane may touch starts inside the data; keep it inside the buffer
    uint8_t* d_in = static_cast<uint8_t*>(scratch(ctx, S_IN, bytes + 8, &e));
    void* d_work = scratch(ctx, S_WORK, commit_workspace_bound(shares, nb), &e);
    uint8_t* d_out = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)nb * 32, &e));
    if (!d_in || !d_work || !d_out) return fail(ctx, CEL_ENOMEM, "device allocation failed");
    const size_t out_at = direct ? 0 : align256(bytes);
    uint8_t* hs = static_cast<uint8_t*>(host_stage(ctx, out_at + (size_t)nb * 32));
    if (!hs) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
    const uint8_t* src = items[b0].data;
    if (!direct) {
      if (contiguous) {
        std::memcpy(hs, src, bytes);
      } else {
        uint64_t at = 0;
        for (uint32_t i = b0; i < b1; i++) {
          std::memcpy(hs + at, items[i].data, items[i].len);
          at += items[i].len;
        }
      }
      src = hs;
    }
    if ((e = hipMemcpyAsync(d_in, src, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
    cel_status st = commit_enqueue(ctx, d_in, 0, nullptr, items.data() + b0, nb, threshold, d_out, d_work, s);
    if (st) return st;
    if ((e = hipMemcpyAsync(hs + out_at, d_out, (size_t)nb * 32, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_fail(ctx, e, "D2H");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
    std::memcpy(commitments + (size_t)b0 * 32, hs + out_at, (size_t)nb * 32);
    b0 = b1;
  }
  return CEL_OK;
}

// Argument checks shared by the host and the device-resident entry; fills items.
cel_status collect(cel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t nblobs,
                   const uint8_t* namespaces, const uint8_t* share_versions, uint32_t threshold, const void* out,
                   std::vector<Item>& items) {
  if (!data || !offsets || !namespaces || !out) return fail(ctx, CEL_EINVAL, "nil argument");
  if (nblobs == 0) return fail(ctx, CEL_EINVAL, "no blobs");
  if (threshold == 0) return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  items.resize(nblobs);
  for (uint32_t i = 0; i < nblobs; i++) {
    if (offsets[i + 1] < offsets[i]) return fail(ctx, CEL_EINVAL, "blob offsets must be non-decreasing");
    const uint64_t len = offsets[i + 1] - offsets[i];
    cel_status st = commit_check_blob(ctx, i, len, share_versions ? share_versions[i] : 0);
    if (st) return st;
    items[i] = Item{namespaces + (size_t)i * kNs, data + offsets[i], len};
  }
  return CEL_OK;
}

}  // namespace

extern "C" {

cel_status cel_create_commitments(cel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t nblobs,
                                  const uint8_t* namespaces, const uint8_t* share_versions,
                                  uint32_t subtree_root_threshold, uint8_t* commitments) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  std::vector<Item> items;
  cel_status st = collect(ctx, data, offsets, nblobs, namespaces, share_versions, subtree_root_threshold, commitments,
                          items);
  if (st) return st;
  return run_host(ctx, items, true, subtree_root_threshold, commitments);
}

size_t cel_dev_commitments_workspace_size(uint64_t total_shares, uint32_t nblobs) {
  return commit_workspace_bound(total_shares, nblobs);
}

cel_status cel_dev_create_commitments(cel_ctx* ctx, const void* d_data, const uint64_t* offsets, uint32_t nblobs,
                                      const uint8_t* namespaces, const uint8_t* share_versions,
                                      uint32_t subtree_root_threshold, void* d_commitments, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  std::vector<Item> items;
  cel_status st = collect(ctx, static_cast<const uint8_t*>(d_data), offsets, nblobs, namespaces, share_versions,
                          subtree_root_threshold, d_commitments, items);
  if (st) return st;
  DeviceGuard g(ctx->device);
  return commit_enqueue(ctx, static_cast<const uint8_t*>(d_data), offsets[0], nullptr, items.data(), nblobs,
                        subtree_root_threshold, static_cast<uint8_t*>(d_commitments), d_work, pick_stream(ctx, stream));
}

cel_status cel_blob_tx_commitments(cel_ctx* ctx, const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                                   uint32_t subtree_root_threshold, uint8_t* commitments, uint32_t* tx_index,
                                   uint32_t cap, uint32_t* n_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_out || (ntx && (!txs || !tx_lens)) || (cap && (!commitments || !tx_index)))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (subtree_root_threshold == 0) return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  std::vector<blob::View> views, all;
  std::vector<uint32_t> from;
  size_t off = 0;
  for (uint32_t t = 0; t < ntx; t++) {
    if (blob::blob_tx_views(txs + off, tx_lens[t], views))
      for (const blob::View& v : views) {
        all.push_back(v);
        from.push_back(t);
      }
    off += tx_lens[t];
  }
  *n_out = (uint32_t)all.size();
  if (cap == 0 || all.empty()) return CEL_OK;
  if (all.size() > cap)
    return fail(ctx, CEL_EINVAL,
                "output holds " + std::to_string(cap) + " blobs, the txs carry " + std::to_string(all.size()));
  std::vector<Item> items(all.size());
  for (size_t i = 0; i < all.size(); i++) {
    cel_status st = commit_check_blob(ctx, (uint32_t)i, all[i].len, all[i].share_version);
    if (st) return st;
    items[i] = Item{all[i].ns, all[i].data, all[i].len};
    tx_index[i] = from[i];
  }
  return run_host(ctx, items, false, subtree_root_threshold, commitments);
}

cel_status cel_blob_subtree_sizes(uint64_t blob_len, uint32_t subtree_root_threshold, uint32_t* shares, uint32_t* width,
                                  uint32_t* sizes, uint32_t cap, uint32_t* n_out) {
  if (blob_len == 0 || subtree_root_threshold == 0 || !n_out || (cap && !sizes)) return CEL_EINVAL;
  const uint64_t n = blob::sparse_shares_needed(blob_len);
  if (n > blob::kMaxShares) return CEL_ETOOBIG;
  const uint32_t w = blob::subtree_width((uint32_t)n, subtree_root_threshold);
  std::vector<uint32_t> mmr;
  blob::mountain_range((uint32_t)n, w, mmr);
  if (shares) *shares = (uint32_t)n;
  if (width) *width = w;
  *n_out = (uint32_t)mmr.size();
  for (uint32_t i = 0; i < cap && i < mmr.size(); i++) sizes[i] = mmr[i];
  return CEL_OK;
}

}  // extern "C"
