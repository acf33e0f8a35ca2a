// C ABI of the txs of a resident square (include/celestia_eds.h):
//   cel_dev_txs_plan / cel_dev_txs_emit  <- go-square v1.1.0 parseCompactShares over runs of ODS
//       shares: the units of the tx and PayForBlob namespaces, what shares.ParseTxs and
//       square.Deconstruct read
//   cel_txs_by_range                      the same for a square in host memory
// The number of units and their sizes depend on the data, so the device walks, counts and places
// them (tx_parse.hip) and the plan call waits for the counts. The emit call writes the records,
// gathers the bytes and hashes them: the share bytes never leave the device.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "api_common.hpp"
#include "cel_internal.hpp"
#include "tx_parse.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

// The plan of n_ranges checked ranges (total shares in all) into d_work; its counts into
// ctx->tx_plan, its statuses and flags into range_status and range_flags (nullable).
// Synchronous on s. ctx->mu held, device current.
cel_status plan_locked(cel_ctx* ctx, const uint8_t* d_eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                       const uint32_t* ends, uint64_t total, uint32_t* range_status, uint32_t* range_flags, void* d_work,
                       hipStream_t s) {
  ctx->tx_plan = cel_ctx::TxPlan{};
  const txparse::Work w = txparse::carve(d_work, total, n_ranges);
  cel_status st = CEL_OK;
  const size_t up_b = (2 * (size_t)n_ranges + 1) * 4, st_b = (size_t)n_ranges * 4;
  const size_t head_at = bparse::align256(up_b), st_at = head_at + bparse::align256(sizeof(txparse::Head));
  const size_t fl_at = st_at + bparse::align256(st_b);
  uint8_t* stage = static_cast<uint8_t*>(plan_stage(ctx, fl_at + st_b, &st));
  if (!stage) return st;
  uint32_t* roff = reinterpret_cast<uint32_t*>(stage);
  bparse::range_offsets(n_ranges, starts, ends, roff);
  std::memcpy(roff + n_ranges + 1, starts, st_b);
  hipError_t e;
  // no plan_uploaded behind this copy: the call waits for s below, before anyone refills the buffer
  if ((e = hipMemcpyAsync(w.roff, stage, up_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((e = launch_tx_parse_plan(d_eds, k, n_ranges, w, s)) != hipSuccess) return hip_fail(ctx, e, "tx plan");
  if ((e = hipMemcpyAsync(stage + head_at, w.head, sizeof(txparse::Head), hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipMemcpyAsync(stage + st_at, w.range_status, st_b, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipMemcpyAsync(stage + fl_at, w.range_flags, st_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  txparse::Head h;
  std::memcpy(&h, stage + head_at, sizeof h);
  // a unit is two bytes or more of a share's 512
  if (h.total != total || h.n_units > total * 256) return fail(ctx, CEL_EDEVICE, "tx plan: more units than the shares hold");
  if (range_status) std::memcpy(range_status, stage + st_at, st_b);
  if (range_flags) std::memcpy(range_flags, stage + fl_at, st_b);
  cel_ctx::TxPlan& p = ctx->tx_plan;
  p.d_work = d_work;
  p.k = k;
  p.n_ranges = n_ranges;
  p.total = total;
  p.n_units = h.n_units;
  p.total_bytes = h.total_bytes;
  return CEL_OK;
}

// The records, bytes and, with d_hashes, hashes of the first n_units units of the ctx's plan,
// enqueued on s. ctx->mu held, device current.
cel_status emit_locked(cel_ctx* ctx, const uint8_t* d_eds, uint64_t n_units, cel_tx_rec* d_recs, uint8_t* d_data,
                       uint8_t* d_hashes, hipStream_t s) {
  const cel_ctx::TxPlan& p = ctx->tx_plan;
  const uint64_t n = n_units < p.n_units ? n_units : p.n_units;
  if (!n) return CEL_OK;
  const txparse::Work w = txparse::carve(const_cast<void*>(p.d_work), p.total, p.n_ranges);
  const hipError_t e = launch_tx_parse_emit(d_eds, p.k, w, p.n_ranges, n, p.total_bytes, d_recs, d_data, d_hashes, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "tx emit");
  return CEL_OK;
}

}  // namespace

extern "C" {

size_t cel_dev_txs_workspace_size(uint64_t total_shares, uint32_t n_ranges) {
  if (total_shares >= bparse::kMaxTotal) return 0;
  return txparse::carve(nullptr, total_shares, n_ranges).bytes;
}

cel_status cel_dev_txs_plan(cel_ctx* ctx, const void* d_eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                            const uint32_t* ends, uint32_t* range_status, uint32_t* range_flags, uint64_t* n_units,
                            uint64_t* total_bytes, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_units || !total_bytes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_units = *total_bytes = 0;
  uint64_t total = 0;
  const std::string err = bparse::ranges_error(k, n_ranges, starts, ends, &total);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n_ranges == 0) {
    ctx->tx_plan = cel_ctx::TxPlan{};
    return CEL_OK;
  }
  if (!d_eds || !d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds and d_work must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  const cel_status st = plan_locked(ctx, static_cast<const uint8_t*>(d_eds), k, n_ranges, starts, ends, total,
                                    range_status, range_flags, d_work, pick_stream(ctx, stream));
  if (st) return st;
  *n_units = ctx->tx_plan.n_units;
  *total_bytes = ctx->tx_plan.total_bytes;
  return CEL_OK;
}

cel_status cel_dev_txs_emit(cel_ctx* ctx, const void* d_eds, uint32_t k, uint64_t n_units, void* d_recs, void* d_data,
                            void* d_hashes, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!is_pow2(k) || k > bparse::kMaxWidth)
    return fail(ctx, CEL_EINVAL, "square width " + std::to_string(k) + " is not a power of two up to 512");
  if (n_units == 0) return CEL_OK;
  if (!d_eds || !d_recs || !d_data || !d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_recs) | reinterpret_cast<uintptr_t>(d_data) |
       reinterpret_cast<uintptr_t>(d_hashes) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds, d_recs, d_data, d_hashes and d_work must be 16-byte aligned");
  const cel_ctx::TxPlan& p = ctx->tx_plan;
  if (p.d_work != d_work || p.k != k)
    return fail(ctx, CEL_EINVAL, "d_work does not hold the last tx plan of this context for width " + std::to_string(k));
  DeviceGuard g(ctx->device);
  return emit_locked(ctx, static_cast<const uint8_t*>(d_eds), n_units, static_cast<cel_tx_rec*>(d_recs),
                     static_cast<uint8_t*>(d_data), static_cast<uint8_t*>(d_hashes), pick_stream(ctx, stream));
}

cel_status cel_txs_by_range(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n_ranges, const uint32_t* starts,
                            const uint32_t* ends, uint64_t cap, uint64_t data_cap, cel_tx_rec* recs,
                            uint32_t* range_status, uint32_t* range_flags, uint8_t* data_out, uint8_t* hashes_out,
                            uint64_t* n_units, uint64_t* total_bytes) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_units || !total_bytes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_units = *total_bytes = 0;
  const bool count_only = cap == 0 && data_cap == 0 && !recs && !data_out && !hashes_out;
  if (!count_only && ((cap && !recs) || (data_cap && !data_out))) return fail(ctx, CEL_EINVAL, "nil argument");
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
  void* d_work = scratch(ctx, S_MASK, txparse::carve(nullptr, total, n_ranges).bytes, &e);
  if (!d_eds || !d_work) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, half_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  // the plan lies in the ctx's own scratch: no later emit call may find it
  struct Forget {
    cel_ctx* ctx;
    ~Forget() { ctx->tx_plan = cel_ctx::TxPlan{}; }
  } forget{ctx};
  cel_status st = plan_locked(ctx, d_eds, k, n_ranges, starts, ends, total, range_status, range_flags, d_work, s);
  if (st) return st;
  const uint64_t units = ctx->tx_plan.n_units, bytes = ctx->tx_plan.total_bytes;
  *n_units = units;
  *total_bytes = bytes;
  if (count_only) return CEL_OK;
  if (cap < units || data_cap < bytes)
    return fail(ctx, CEL_EINVAL, "caps (" + std::to_string(cap) + ", " + std::to_string(data_cap) +
                                     ") are below the plan's " + std::to_string(units) + " units, " +
                                     std::to_string(bytes) + " bytes");
  if (!units) return CEL_OK;
  const size_t rec_b = (size_t)units * sizeof(cel_tx_rec), hash_b = (size_t)units * 32;
  cel_tx_rec* d_recs = static_cast<cel_tx_rec*>(scratch(ctx, S_WORK, rec_b, &e));
  uint8_t* d_data = static_cast<uint8_t*>(scratch(ctx, S_IN, bytes, &e));
  uint8_t* d_hashes = hashes_out ? static_cast<uint8_t*>(scratch(ctx, S_ROOTS, hash_b, &e)) : nullptr;
  if (!d_recs || !d_data || (hashes_out && !d_hashes)) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  if ((st = emit_locked(ctx, d_eds, units, d_recs, d_data, d_hashes, s)) != CEL_OK) return st;
  if ((e = hipMemcpyAsync(recs, d_recs, rec_b, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipMemcpyAsync(data_out, d_data, bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (hashes_out && (e = hipMemcpyAsync(hashes_out, d_hashes, hash_b, hipMemcpyDeviceToHost, s)) != hipSuccess))
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

}  // extern "C"
