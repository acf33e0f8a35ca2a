// Shared helpers of the C-ABI host layer (every api_*.cpp): error reporting with the
// reference's messages, grow-only device scratch and page-locked staging per ctx, the plan
// buffer's upload rule, device selection, argument checks of a square, and the entry points
// one api file lends another (blob commitments, the repair with the ctx lock held).
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

// The ctx's page-locked plan buffer with room for `bytes`, once its last upload has left it
// (the ev_plan rule of cel_internal.hpp). nullptr with the status in *st. A caller that
// uploads from the buffer calls plan_uploaded behind the copy, unless it waits for the stream
// itself before it returns (the namespace plan).
inline void* plan_stage(cel_ctx* ctx, size_t bytes, cel_status* st) {
  if (bytes == 0) bytes = 256;  // never nullptr on success
  hipError_t e;
  if (!ctx->ev_plan && (e = hipEventCreateWithFlags(&ctx->ev_plan, hipEventDisableTiming)) != hipSuccess) {
    *st = hip_fail(ctx, e, "event");
    return nullptr;
  }
  if (ctx->plan_pending) {
    if ((e = hipEventSynchronize(ctx->ev_plan)) != hipSuccess) {
      *st = hip_fail(ctx, e, "plan upload");
      return nullptr;
    }
    ctx->plan_pending = false;
  }
  if (ctx->plan_stage_size < bytes) {
    if (ctx->plan_stage) (void)hipHostFree(ctx->plan_stage);
    ctx->plan_stage = nullptr;
    ctx->plan_stage_size = 0;
    if (hipHostMalloc(&ctx->plan_stage, bytes, hipHostMallocDefault) != hipSuccess) {
      ctx->plan_stage = nullptr;
      *st = fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
      return nullptr;
    }
    ctx->plan_stage_size = bytes;
  }
  return ctx->plan_stage;
}

// After the copy out of the plan buffer has been enqueued on s: the next plan_stage waits for it.
inline cel_status plan_uploaded(cel_ctx* ctx, hipStream_t s) {
  const hipError_t e = hipEventRecord(ctx->ev_plan, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "event");
  ctx->plan_pending = true;
  return CEL_OK;
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
// at byte offsets offs[i]; uploads the plan into d_work's head (through ctx->plan_stage, under
// its ev_plan rule) and enqueues the kernels on s: 32 bytes per blob into d_out.
cel_status commit_enqueue(cel_ctx* ctx, const uint8_t* d_data, uint64_t base_off, const uint64_t* offs,
                          const CommitItem* items, uint32_t nb, uint32_t threshold, uint8_t* d_out, void* d_work,
                          hipStream_t s);

// cel_dev_repair's body, for a caller that holds ctx->mu (api_repair.cpp).
cel_status dev_repair_locked(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k, const uint8_t* row_roots,
                             const uint8_t* col_roots, int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                             uint8_t* byz_present);

inline cel_status validate_square(cel_ctx* ctx, uint32_t k, uint32_t share_size) {
  if (share_size != kShare)
    return fail(ctx, CEL_ECHUNK, "share size must be appconsts.ShareSize (512) on the device path");
  if (!is_pow2(k)) return fail(ctx, CEL_ENOTPOW2, "square width is not a power of 2: got " + std::to_string(k));
  if (k > 512) return fail(ctx, CEL_ETOOBIG, "square width " + std::to_string(k) + " exceeds the device path (512)");
  return CEL_OK;
}

}  // namespace abi
}  // namespace cel
