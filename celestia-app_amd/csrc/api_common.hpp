// Shared helpers of the C-ABI host layer (every api_*.cpp): error reporting with the
// reference's messages, grow-only device scratch and page-locked staging per ctx, the staged
// uploads' rule, the EDS copy-back, device selection, argument checks of a square, and the
// entry points one api file lends another (blob commitments, the repair with the ctx lock held).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "cel_internal.hpp"

namespace cel {
namespace abi {

enum ScratchSlot { S_IN = 0, S_EDS = 1, S_WORK = 2, S_ROOTS = 3, S_AUX = 4, S_MASK = 5, S_SQ = 6 };

inline cel_status fail(cel_ctx* ctx, cel_status st, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return st;
}

inline cel_status hip_fail(cel_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, CEL_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

inline void* scratch(cel_ctx* ctx, int slot, size_t bytes, hipError_t* err) {
  if (bytes == 0) bytes = 256;
  if (ctx->scratch_size[slot] >= bytes) return ctx->scratch[slot];
  if (ctx->scratch[slot]) (void)hipFree(ctx->scratch[slot]);
  ctx->scratch[slot] = nullptr;
  ctx->scratch_size[slot] = 0;
  void* p = nullptr;
  *err = hipMalloc(&p, bytes);
  if (*err != hipSuccess) return nullptr;
  ctx->scratch[slot] = p;
  ctx->scratch_size[slot] = bytes;
  return p;
}

// Grow-only page-locked host staging of a ctx (calls on a ctx hold its lock, so one buffer
// serves them all): device results come back in one asynchronous copy into it, then a host
// memcpy to the caller's (often pageable) buffers. nullptr if the allocation fails.
inline void* host_stage(cel_ctx* ctx, size_t bytes) {
  if (ctx->hstage_size >= bytes) return ctx->hstage;
  if (ctx->hstage) (void)hipHostFree(ctx->hstage);
  ctx->hstage = nullptr;
  ctx->hstage_size = 0;
  // coherent: kernels may store results into it directly (the one-square DAH launch)
  if (hipHostMalloc(&ctx->hstage, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
  ctx->hstage_size = bytes;
  return ctx->hstage;
}

// A staged upload's buffer with room for `bytes`, once its last upload has left it (the
// StagedUpload rule of cel_internal.hpp). nullptr with the status in *st. A caller that uploads
// from the buffer calls stage_uploaded behind the copy, unless it waits for the stream itself
// before it returns (the namespace plan).
inline void* stage_acquire(cel_ctx* ctx, StagedUpload& u, size_t bytes, cel_status* st) {
  if (bytes == 0) bytes = 256;  // never nullptr on success
  hipError_t e;
  if (!u.ev && (e = hipEventCreateWithFlags(&u.ev, hipEventDisableTiming)) != hipSuccess) {
    *st = hip_fail(ctx, e, "event");
    return nullptr;
  }
  if (u.pending) {
    if ((e = hipEventSynchronize(u.ev)) != hipSuccess) {
      *st = hip_fail(ctx, e, "plan upload");
      return nullptr;
    }
    u.pending = false;
  }
  if (u.size < bytes) {
    if (u.buf) (void)hipHostFree(u.buf);
    u.buf = nullptr;
    u.size = 0;
    if (hipHostMalloc(&u.buf, bytes, hipHostMallocDefault) != hipSuccess) {
      u.buf = nullptr;
      *st = fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
      return nullptr;
    }
    u.size = bytes;
  }
  return u.buf;
}

// After the copy out of the buffer has been enqueued on s: the next stage_acquire waits for it.
inline cel_status stage_uploaded(cel_ctx* ctx, StagedUpload& u, hipStream_t s) {
  const hipError_t e = hipEventRecord(u.ev, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "event");
  u.pending = true;
  return CEL_OK;
}

// The ctx's plan buffer under that rule.
inline void* plan_stage(cel_ctx* ctx, size_t bytes, cel_status* st) { return stage_acquire(ctx, ctx->plan_up, bytes, st); }
inline cel_status plan_uploaded(cel_ctx* ctx, hipStream_t s) { return stage_uploaded(ctx, ctx->plan_up, s); }

// A square's push-order status as the call's result, with the reference's message.
constexpr const char* kOrderMessage = "invalid push order: leaf namespaces must be non-decreasing";
inline cel_status order_status(cel_ctx* ctx, int32_t st) {
  return st == CEL_EORDER ? fail(ctx, CEL_EORDER, kOrderMessage) : (cel_status)st;
}

// The rectangles of an EDS copy-back (ext::copy_back_rects) enqueued on s, in order. One that is
// contiguous on both sides goes as hipMemcpyAsync, a strided one as hipMemcpy2DAsync: the DMA
// engines treat the two calls differently, and the paths were measured with these. always_2d:
// every rectangle as a 2-D copy (the shard plan's slabs, also the one rank's whole square).
inline hipError_t copy_back(uint8_t* host, const uint8_t* dev, const ext::Rects& rs, hipStream_t s,
                            bool always_2d = false) {
  hipError_t e = hipSuccess;
  for (uint32_t i = 0; i < rs.n && e == hipSuccess; i++) {
    const ext::Rect& r = rs.r[i];
    e = r.contiguous() && !always_2d
            ? hipMemcpyAsync(host + r.dst_off, dev + r.src_off, r.width * r.rows, hipMemcpyDeviceToHost, s)
            : hipMemcpy2DAsync(host + r.dst_off, r.dst_pitch, dev + r.src_off, r.src_pitch, r.width, r.rows,
                               hipMemcpyDeviceToHost, s);
  }
  return e;
}

// `to` goes on only behind what `from` holds now: ev recorded on from, waited for on to.
inline hipError_t stream_after(hipStream_t to, hipEvent_t ev, hipStream_t from) {
  const hipError_t e = hipEventRecord(ev, from);
  return e == hipSuccess ? hipStreamWaitEvent(to, ev, 0) : e;
}

inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }

// da.SquareSize: RoundUpPowerOfTwo(ceil(sqrt(len))) (data_availability_header.go:205-215)
inline uint32_t square_size(uint32_t n) {
  const uint32_t s = (uint32_t)std::ceil(std::sqrt((double)n));
  uint32_t r = 1;
  while (r < s) r <<= 1;
  return r;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

inline hipStream_t pick_stream(cel_ctx* ctx, void* stream) {
  return stream ? static_cast<hipStream_t>(stream) : ctx->stream;
}


// Blob share commitments (api_commit.cpp), shared with the block entry point (api_block.cpp).
struct CommitItem {
  const uint8_t* ns;    // 29 bytes
  const uint8_t* data;  // host bytes (unused where the bytes are on the device already)
  uint64_t len;
};
// Is p page-locked host memory (cel_host_alloc, hipHostMalloc / hipHostRegister)?
bool page_locked(const void* p);
// "blob i has no data" / "unsupported share version v" / above 2^20 shares.
cel_status commit_check_blob(cel_ctx* ctx, uint32_t i, uint64_t len, uint32_t share_version);
// Workspace for any plan of nblobs blobs with total_shares shares.
size_t commit_workspace_bound(uint64_t total_shares, uint32_t nblobs);
// Plans nb blobs whose bytes lie in d_data back to back from base_off on (offs == nullptr) or
// at byte offsets offs[i]; uploads the plan into d_work's head (through plan_stage, under
// its rule) and enqueues the kernels on s: 32 bytes per blob into d_out.
cel_status commit_enqueue(cel_ctx* ctx, const uint8_t* d_data, uint64_t base_off, const uint64_t* offs,
                          const CommitItem* items, uint32_t nb, uint32_t threshold, uint8_t* d_out, void* d_work,
                          hipStream_t s);

// cel_dev_repair's body, for a caller that holds ctx->mu (api_repair.cpp).
cel_status dev_repair_locked(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k, const uint8_t* row_roots,
                             const uint8_t* col_roots, int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                             uint8_t* byz_present);

// The batch tree index of n <= prove::kMaxSquares squares (api_prove.cpp), for a caller that holds
// ctx->mu with the device current and the arguments checked; status (host, n, nullable) is copied
// back on s. Shared with the namespace rows over many squares (api_namespace.cpp).
cel_status index_batch_enqueue(cel_ctx* ctx, const uint8_t* d_eds, uint32_t n, uint32_t k, void* d_index,
                               uint8_t* d_row_roots, uint8_t* d_col_roots, uint8_t* d_dah, int32_t* status,
                               bool order_check, hipStream_t s);

inline cel_status validate_square(cel_ctx* ctx, uint32_t k, uint32_t share_size) {
  if (share_size != kShare)
    return fail(ctx, CEL_ECHUNK, "share size must be appconsts.ShareSize (512) on the device path");
  if (!is_pow2(k)) return fail(ctx, CEL_ENOTPOW2, "square width is not a power of 2: got " + std::to_string(k));
  if (k > 512) return fail(ctx, CEL_ETOOBIG, "square width " + std::to_string(k) + " exceeds the device path (512)");
  return CEL_OK;
}

}  // namespace abi
}  // namespace cel
