// C ABI of the blobs of a resident square (include/celestia_eds.h):
//   cel_dev_blobs_plan / cel_dev_blobs_emit  <- go-square v1.1.0 parseSparseShares over runs of
//       ODS shares, then inclusion.CreateCommitment of every blob found: what celestia-node's
//       blob service (GetAll, Get, Included) builds from the shares of a namespace
//   cel_blobs_by_range                        the same for a square in host memory
//   cel_namespace_ods_ranges                  a namespace plan's inclusion entries as ODS ranges
// The number of blobs and their sizes depend on the data, so the device classifies, counts and
// places them (blob_parse.hip) and the plan call waits for the counts. The emit call gathers
// the bytes into the layout the commitments take (api_commit.cpp, blob_commit.hip): the share
// bytes never leave the device.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "blob_parse.hpp"
#include "cel_internal.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

struct Counts {
  uint64_t blobs = 0, bytes = 0;
};

// The plan of n_ranges checked ranges (total shares in all) into d_work; its records into
// ctx->blob_plan, its statuses into range_status (nullable). Synchronous on s. ctx->mu held,
// device current.
cel_status plan_locked(cel_ctx* ctx, const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                       const uint32_t* ends, uint64_t total, uint32_t* range_status, Counts* out, void* d_work,
                       hipStream_t s) {
  ctx->blob_plan = cel_ctx::BlobPlan{};
  const bparse::Work w = bparse::carve(d_work, total, n_ranges);
  cel_status st = CEL_OK;
  const size_t up_b = (2 * (size_t)n_ranges + 1) * 4;
  uint8_t* stage = static_cast<uint8_t*>(plan_stage(ctx, align256(up_b) + sizeof(bparse::Head), &st));
  if (!stage) return st;
  uint32_t* roff = reinterpret_cast<uint32_t*>(stage);
  bparse::range_offsets(n_ranges, starts, ends, roff);
  std::memcpy(roff + n_ranges + 1, starts, (size_t)n_ranges * 4);
  hipError_t e;
  // no plan_uploaded behind this copy: the call waits for s below, before anyone refills the buffer
  if ((e = hipMemcpyAsync(w.roff, stage, up_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((e = launch_blob_parse_plan(d_eds, k, n_ranges, w, s)) != hipSuccess) return hip_fail(ctx, e, "blob plan");
  bparse::Head* head = reinterpret_cast<bparse::Head*>(stage + align256(up_b));
  if ((e = hipMemcpyAsync(head, w.head, sizeof(bparse::Head), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  const bparse::Head h = *head;
  if (h.n_blobs > total || h.total != total || h.total_shares > total)
    return fail(ctx, CEL_EDEVICE, "blob plan: more blobs than shares");
  const size_t rec_b = (size_t)h.n_blobs * sizeof(cel_blob_rec), st_b = (size_t)n_ranges * 4;
  stage = static_cast<uint8_t*>(plan_stage(ctx, align256(rec_b) + st_b, &st));
  if (!stage) return st;
  if (rec_b && (e = hipMemcpyAsync(stage, w.recs, rec_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipMemcpyAsync(stage + align256(rec_b), w.range_status, st_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  if (range_status) std::memcpy(range_status, stage + align256(rec_b), st_b);
  cel_ctx::BlobPlan& p = ctx->blob_plan;
  const cel_blob_rec* recs = reinterpret_cast<const cel_blob_rec*>(stage);
  p.recs.assign(recs, recs + h.n_blobs);
  p.d_work = d_work;
  p.k = k;
  p.n_ranges = n_ranges;
  p.total = total;
  p.total_bytes = h.total_bytes;
  out->blobs = h.n_blobs;
  out->bytes = h.total_bytes;
  return CEL_OK;
}

// The bytes and, with d_commitments, the commitments of the first n_blobs blobs of the ctx's
// plan, enqueued on s. ctx->mu held, device current.
cel_status emit_locked(cel_ctx* ctx, const uint8_t* d_eds, uint64_t n_blobs, uint8_t* d_data, uint8_t* d_commitments,
                       uint32_t threshold, void* d_commit_work, hipStream_t s) {
  const cel_ctx::BlobPlan& p = ctx->blob_plan;
  const uint32_t nb = (uint32_t)(n_blobs < p.recs.size() ? n_blobs : p.recs.size());
  if (!nb) return CEL_OK;
  const bparse::Work w = bparse::carve(const_cast<void*>(p.d_work), p.total, p.n_ranges);
  const uint64_t bytes = nb < p.recs.size() ? p.recs[nb].data_off : p.total_bytes;
  hipError_t e;
  if ((e = launch_blob_parse_gather(d_eds, p.k, w, nb, bytes, d_data, s)) != hipSuccess)
    return hip_fail(ctx, e, "blob gather");
  if (!d_commitments) return CEL_OK;
  std::vector<CommitItem> items(nb);
  std::vector<uint64_t> offs(nb);
  for (uint32_t i = 0; i < nb; i++) {
    items[i] = CommitItem{p.recs[i].ns, nullptr, p.recs[i].len};
    offs[i] = p.recs[i].data_off;
  }
  return commit_enqueue(ctx, d_data, 0, offs.data(), items.data(), nb, threshold, d_commitments, d_commit_work, s);
}

}  // namespace

extern "C" {

size_t cel_dev_blobs_workspace_size(uint64_t total_shares, uint32_t n_ranges) {
  if (total_shares >= bparse::kMaxTotal) return 0;
  return bparse::carve(nullptr, total_shares, n_ranges).bytes;
}

cel_status cel_dev_blobs_plan(cel_ctx* ctx, const void* d_eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                              const uint32_t* ends, uint64_t cap, cel_blob_rec* recs, uint32_t* range_status,
                              uint64_t* n_blobs, uint64_t* total_bytes, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_blobs || !total_bytes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_blobs = *total_bytes = 0;
  if (cap && !recs) return fail(ctx, CEL_EINVAL, "nil argument");
  uint64_t total = 0;
  const std::string err = bparse::ranges_error(k, n_ranges, starts, ends, &total);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n_ranges == 0) {
    ctx->blob_plan = cel_ctx::BlobPlan{};
    return CEL_OK;
  }
  if (!d_eds || !d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds and d_work must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  Counts c;
  const cel_status st = plan_locked(ctx, static_cast<const uint8_t*>(d_eds), k, n_ranges, starts, ends, total,
                                    range_status, &c, d_work, pick_stream(ctx, stream));
  if (st) return st;
  *n_blobs = c.blobs;
  *total_bytes = c.bytes;
  if (cap == 0 && !recs) return CEL_OK;
  if (cap < c.blobs)
    return fail(ctx, CEL_EINVAL, "cap " + std::to_string(cap) + " is below the " + std::to_string(c.blobs) +
                                     " blobs of the plan");
  if (c.blobs) std::memcpy(recs, ctx->blob_plan.recs.data(), (size_t)c.blobs * sizeof(cel_blob_rec));
  return CEL_OK;
}

cel_status cel_dev_blobs_emit(cel_ctx* ctx, const void* d_eds, uint32_t k, uint64_t n_blobs, void* d_data,
                              void* d_commitments, uint32_t subtree_root_threshold, void* d_work, void* d_commit_work,
                              void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!is_pow2(k) || k > bparse::kMaxWidth)
    return fail(ctx, CEL_EINVAL, "square width " + std::to_string(k) + " is not a power of two up to 512");
  if (n_blobs == 0) return CEL_OK;
  if (!d_eds || !d_data || !d_work || (d_commitments && !d_commit_work)) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_data) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds, d_data and d_work must be 16-byte aligned");
  if (d_commitments && subtree_root_threshold == 0)
    return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  const cel_ctx::BlobPlan& p = ctx->blob_plan;
  if (p.d_work != d_work || p.k != k)
    return fail(ctx, CEL_EINVAL, "d_work does not hold the last blob plan of this context for width " + std::to_string(k));
  DeviceGuard g(ctx->device);
  return emit_locked(ctx, static_cast<const uint8_t*>(d_eds), n_blobs, static_cast<uint8_t*>(d_data),
                     static_cast<uint8_t*>(d_commitments), subtree_root_threshold, d_commit_work,
                     pick_stream(ctx, stream));
}

cel_status cel_blobs_by_range(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                              const uint32_t* ends, uint64_t cap, uint64_t data_cap, cel_blob_rec* recs,
                              uint32_t* range_status, uint8_t* data_out, uint8_t* commitments_out,
                              uint32_t subtree_root_threshold, uint64_t* n_blobs, uint64_t* total_bytes) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_blobs || !total_bytes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_blobs = *total_bytes = 0;
  const bool count_only = cap == 0 && data_cap == 0 && !recs && !data_out && !commitments_out;
  if (!count_only && ((cap && !recs) || (data_cap && !data_out))) return fail(ctx, CEL_EINVAL, "nil argument");
  if (commitments_out && subtree_root_threshold == 0)
    return fail(ctx, CEL_EINVAL, "subtree root threshold must be positive");
  uint64_t total = 0;
  const std::string err = bparse::ranges_error(k, n_ranges, starts, ends, &total);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n_ranges == 0) return CEL_OK;
  if (!eds) return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  // the upper half of the square holds Q0: rows 0 .. k - 1 at their pitch of 2k shares
  const size_t half_b = (size_t)2 * k * k * kShare;
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, half_b, &e));
  void* d_work = scratch(ctx, S_MASK, bparse::carve(nullptr, total, n_ranges).bytes, &e);
  if (!d_eds || !d_work) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, half_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  // the plan lies in the ctx's own scratch: no later emit call may find it
  struct Forget {
    cel_ctx* ctx;
    ~Forget() { ctx->blob_plan = cel_ctx::BlobPlan{}; }
  } forget{ctx};
  Counts c;
  cel_status st = plan_locked(ctx, d_eds, k, n_ranges, starts, ends, total, range_status, &c, d_work, s);
  if (st) return st;
  *n_blobs = c.blobs;
  *total_bytes = c.bytes;
  if (count_only) return CEL_OK;
  if (cap < c.blobs || data_cap < c.bytes)
    return fail(ctx, CEL_EINVAL, "caps (" + std::to_string(cap) + ", " + std::to_string(data_cap) +
                                     ") are below the plan's " + std::to_string(c.blobs) + " blobs, " +
                                     std::to_string(c.bytes) + " bytes");
  if (!c.blobs) return CEL_OK;
  std::memcpy(recs, ctx->blob_plan.recs.data(), (size_t)c.blobs * sizeof(cel_blob_rec));
  uint64_t shares = 0;
  for (const cel_blob_rec& r : ctx->blob_plan.recs) shares += r.shares;
  const uint32_t nb = (uint32_t)c.blobs;
  uint8_t* d_data = static_cast<uint8_t*>(scratch(ctx, S_IN, c.bytes, &e));
  void* d_cwork = commitments_out ? scratch(ctx, S_WORK, commit_workspace_bound(shares, nb), &e) : nullptr;
  uint8_t* d_out = commitments_out ? static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)nb * 32, &e)) : nullptr;
  if (!d_data || (commitments_out && (!d_cwork || !d_out))) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  if ((st = emit_locked(ctx, d_eds, nb, d_data, d_out, subtree_root_threshold, d_cwork, s)) != CEL_OK) return st;
  if ((e = hipMemcpyAsync(data_out, d_data, c.bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if (commitments_out &&
      (e = hipMemcpyAsync(commitments_out, d_out, (size_t)nb * 32, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

cel_status cel_namespace_ods_ranges(uint32_t k, uint32_t n_namespaces, uint64_t n_entries, const uint32_t* ns_idx,
                                    const uint32_t* rows, const int32_t* starts, const int32_t* ends,
                                    const uint8_t* kinds, uint32_t* range_start, uint32_t* range_end) {
  if (!is_pow2(k) || k > bparse::kMaxWidth) return CEL_EINVAL;
  if (n_namespaces && (!range_start || !range_end)) return CEL_EINVAL;
  if (n_entries && (!ns_idx || !rows || !starts || !ends || !kinds)) return CEL_EINVAL;
  std::vector<uint8_t> seen(n_namespaces, 0);
  for (uint32_t i = 0; i < n_namespaces; i++) range_start[i] = range_end[i] = 0;
  for (uint64_t e = 0; e < n_entries; e++) {
    if (ns_idx[e] >= n_namespaces) return CEL_EINVAL;
    if (kinds[e] != CEL_NS_INCLUSION) continue;
    if (rows[e] >= k || starts[e] < 0 || ends[e] <= starts[e] || (uint32_t)ends[e] > k) return CEL_EINVAL;
    const uint32_t i = ns_idx[e];
    const uint32_t a = rows[e] * k + (uint32_t)starts[e], b = rows[e] * k + (uint32_t)ends[e];
    if (!seen[i]) {
      seen[i] = 1;
      range_start[i] = a;
    } else if (a != range_end[i]) {
      return CEL_EINVAL;  // a gap, or entries out of order: not one run of ODS shares
    }
    range_end[i] = b;
  }
  return CEL_OK;
}

}  // extern "C"
