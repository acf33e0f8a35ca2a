// C ABI of the batched NMT prover (include/celestia_eds.h):
//   cel_dev_tree_index_build  every node of the 4k NMTs of a resident square, kept on the device
//   cel_prove_offsets         nmt ProveRange's node counts as prefix sums (host only)
//   cel_dev_prove_batch       <- nmt v0.22.0 NamespacedMerkleTree.ProveRange [dep] for every
//       request of a batch: the range proofs of ShareProofs (pkg/proof/proof.go:147-202) and
//       of sampled cells, in the layout cel_dev_nmt_verify_batch and cel_dev_place_samples read
//   cel_prove_samples / cel_prove_ranges  the same for a square in host memory
//   cel_dev_tree_index_build_batch / cel_dev_prove_squares / cel_prove_samples_squares  the index
//       of n resident squares of one width in one launch per step, and proofs whose requests
//       each name their square (nmt_prove.hpp: the batch index)
// The host checks the requests and uploads one fixed-size record per proof; the nodes are
// selected and packed in nmt_prove.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "cel_internal.hpp"
#include "nmt_prove.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

bool index_width(uint32_t k) { return is_pow2(k) && k <= kMaxGf16Width; }

// "" if [start, end) is a range of 2k leaves, else what is wrong with it.
std::string range_error(uint32_t i, uint32_t W, int32_t start, int32_t end) {
  if (start >= 0 && end > start && (uint32_t)end <= W) return "";
  return "proof " + std::to_string(i) + ": range [" + std::to_string(start) + ", " + std::to_string(end) +
         ") is not a range of " + std::to_string(W) + " leaves";
}

thread_local std::string offsets_error;

// The prefix sums of cel_prove_offsets; the message of a bad range into *err.
cel_status offsets(uint32_t k, uint32_t n, const int32_t* starts, const int32_t* ends, uint64_t* leaf_off,
                   uint64_t* node_off, std::string* err) {
  const prove::IndexLayout x = prove::index_layout(k);
  leaf_off[0] = node_off[0] = 0;
  for (uint32_t i = 0; i < n; i++) {
    *err = range_error(i, x.W, starts[i], ends[i]);
    if (!err->empty()) return CEL_EINVAL;
    leaf_off[i + 1] = leaf_off[i] + (uint64_t)(ends[i] - starts[i]);
    node_off[i + 1] = node_off[i] + prove::node_count(x.L, (uint32_t)starts[i], (uint32_t)ends[i] - 1);
  }
  return CEL_OK;
}

// The request table of a batch through the ctx's page-locked plan buffer (under its staged-upload
// rule, as verify_enqueue does) into d_work, then the kernel. ctx->mu held, device current.
// squares != nullptr: a batch index of n_squares squares, request i on square squares[i]; the
// table is then one of prove::SquareRequest.
cel_status prove_enqueue(cel_ctx* ctx, const uint8_t* d_eds, const void* d_index, uint32_t k, uint32_t n,
                         const uint8_t* axes, const uint32_t* index, const int32_t* starts, const int32_t* ends,
                         uint8_t* d_leaves, uint8_t* d_nodes, void* d_work, hipStream_t s,
                         const uint32_t* squares = nullptr, uint32_t n_squares = 1) {
  const prove::IndexLayout x = prove::index_layout(k);
  const size_t bytes = (size_t)n * (squares ? sizeof(prove::SquareRequest) : sizeof(prove::Request));
  cel_status st = CEL_OK;
  void* stage = plan_stage(ctx, bytes, &st);
  if (!stage) return st;
  prove::Request* req = static_cast<prove::Request*>(stage);
  prove::SquareRequest* sreq = static_cast<prove::SquareRequest*>(stage);
  // one pass: each request checked and written with the running sums of cel_prove_offsets;
  // nothing is enqueued before the last one has passed
  uint64_t node0 = 0, leaf0 = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (squares && squares[i] >= n_squares)
      return fail(ctx, CEL_EINVAL, "proof " + std::to_string(i) + ": square " + std::to_string(squares[i]) + " of " +
                                       std::to_string(n_squares));
    if (axes[i] > 1) return fail(ctx, CEL_EINVAL, "proof " + std::to_string(i) + ": axis " + std::to_string(axes[i]));
    if (index[i] >= x.W)
      return fail(ctx, CEL_EINVAL, "proof " + std::to_string(i) + ": tree " + std::to_string(index[i]) + " of " +
                                       std::to_string(x.W));
    if (starts[i] < 0 || ends[i] <= starts[i] || (uint32_t)ends[i] > x.W)
      return fail(ctx, CEL_EINVAL, range_error(i, x.W, starts[i], ends[i]));
    const prove::Request r{axes[i], index[i], starts[i], ends[i], node0, leaf0};
    if (squares) sreq[i] = prove::SquareRequest{r, squares[i], 0};
    else req[i] = r;
    leaf0 += (uint64_t)(ends[i] - starts[i]);
    node0 += prove::node_count(x.L, (uint32_t)starts[i], (uint32_t)ends[i] - 1);
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(d_work, stage, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((st = plan_uploaded(ctx, s)) != CEL_OK) return st;
  e = squares ? launch_prove_squares(d_eds, d_index, k, static_cast<const prove::SquareRequest*>(d_work), n, d_leaves,
                                     d_nodes, s)
              : launch_prove(d_eds, d_index, k, static_cast<const prove::Request*>(d_work), n, d_leaves, d_nodes, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "nmt prove");
  return CEL_OK;
}

// cel_prove_ranges with ctx->mu held and the arguments checked: upload, index, proofs, download.
cel_status prove_host(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n, const uint8_t* axes,
                      const uint32_t* index, const int32_t* starts, const int32_t* ends, uint8_t* leaves_out,
                      uint8_t* nodes_out, uint64_t* node_off_out) {
  std::vector<uint64_t> leaf_off((size_t)n + 1), node_off((size_t)n + 1);
  std::string err;
  if (offsets(k, n, starts, ends, leaf_off.data(), node_off.data(), &err) != CEL_OK) return fail(ctx, CEL_EINVAL, err);
  if (node_off_out) std::memcpy(node_off_out, node_off.data(), ((size_t)n + 1) * 8);
  const size_t eds_b = (size_t)4 * k * k * kShare, leaf_b = leaves_out ? (size_t)leaf_off[n] * kShare : 0,
               node_b = (size_t)node_off[n] * kNode;
  DeviceGuard g(ctx->device);
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  void* d_index = scratch(ctx, S_WORK, prove::index_layout(k).bytes, &e);
  uint8_t* d_leaves = static_cast<uint8_t*>(scratch(ctx, S_IN, leaf_b, &e));
  uint8_t* d_nodes = static_cast<uint8_t*>(scratch(ctx, S_AUX, node_b, &e));
  uint8_t* d_roots = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)4 * k * kNode, &e));
  void* d_req = scratch(ctx, S_MASK, (size_t)n * sizeof(prove::Request), &e);
  if (!d_eds || !d_index || !d_leaves || !d_nodes || !d_roots || !d_req)
    return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, eds_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((e = launch_tree_index(d_eds, k, d_index, d_roots, d_roots + (size_t)2 * k * kNode, nullptr, nullptr, false,
                             s)) != hipSuccess)
    return hip_fail(ctx, e, "tree index");
  const cel_status st = prove_enqueue(ctx, d_eds, d_index, k, n, axes, index, starts, ends,
                                      leaves_out ? d_leaves : nullptr, d_nodes, d_req, s);
  if (st) return st;
  if (leaf_b && (e = hipMemcpyAsync(leaves_out, d_leaves, leaf_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if (node_b && (e = hipMemcpyAsync(nodes_out, d_nodes, node_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

// "" if the batch calls take n_squares squares of width k, else what is wrong.
std::string squares_error(uint32_t k, uint32_t n_squares) {
  if (!is_pow2(k) || k > 512) return "square width " + std::to_string(k) + " is not a power of two up to 512";
  if (n_squares > prove::kMaxSquares)
    return std::to_string(n_squares) + " squares are more than one call takes (" + std::to_string(prove::kMaxSquares) +
           ")";
  return "";
}

}  // namespace

// The batch index of n squares and, with `status`, its copy back on s through the ctx's status
// array (cel_internal.hpp: ix_status). ctx->mu held, device current, arguments checked.
cel_status cel::abi::index_batch_enqueue(cel_ctx* ctx, const uint8_t* d_eds, uint32_t n, uint32_t k, void* d_index,
                               uint8_t* d_row_roots, uint8_t* d_col_roots, uint8_t* d_dah, int32_t* status,
                               bool order_check, hipStream_t s) {
  hipError_t e;
  int32_t* d_status = nullptr;
  if (status) {
    if (!ctx->ev_ix_status &&
        (e = hipEventCreateWithFlags(&ctx->ev_ix_status, hipEventDisableTiming)) != hipSuccess)
      return hip_fail(ctx, e, "event");
    if (ctx->ix_status_n < n) {
      if (ctx->ix_status_pending && (e = hipEventSynchronize(ctx->ev_ix_status)) != hipSuccess)
        return hip_fail(ctx, e, "index status");
      ctx->ix_status_pending = false;
      if (ctx->ix_status) (void)hipFree(ctx->ix_status);
      ctx->ix_status = nullptr;
      ctx->ix_status_n = 0;
      const size_t cap = ((size_t)n + 63) & ~(size_t)63;
      if (hipMalloc(reinterpret_cast<void**>(&ctx->ix_status), cap * 4) != hipSuccess) {
        ctx->ix_status = nullptr;
        return fail(ctx, CEL_ENOMEM, "device allocation failed");
      }
      ctx->ix_status_n = cap;
    } else if (ctx->ix_status_pending && (e = hipStreamWaitEvent(s, ctx->ev_ix_status, 0)) != hipSuccess) {
      return hip_fail(ctx, e, "index status");
    }
    d_status = ctx->ix_status;
  }
  if ((e = launch_tree_index_batch(d_eds, k, n, d_index, d_row_roots, d_col_roots, d_dah, d_status, order_check, s)) !=
      hipSuccess)
    return hip_fail(ctx, e, "tree index batch");
  if (status) {
    if ((e = hipMemcpyAsync(status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_fail(ctx, e, "D2H");
    if ((e = hipEventRecord(ctx->ev_ix_status, s)) != hipSuccess) return hip_fail(ctx, e, "event");
    ctx->ix_status_pending = true;
  }
  return CEL_OK;
}

extern "C" {

size_t cel_dev_tree_index_batch_size(uint32_t k, uint32_t n) {
  // n times the single size for every width the single size is given for; the build below takes
  // the widths cel_dev_tree_index_build takes (up to 512), as the single pair does
  if (!index_width(k) || n == 0 || n > prove::kMaxSquares) return 0;
  const uint64_t one = prove::index_bytes(2 * k);
  if (one > SIZE_MAX / n) return 0;
  return (size_t)(one * n);
}

cel_status cel_dev_tree_index_build_batch(cel_ctx* ctx, const void* d_eds, uint32_t n, uint32_t k, void* d_index,
                                          void* d_row_roots, void* d_col_roots, void* d_dah, int32_t* status,
                                          uint32_t flags, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const std::string err = squares_error(k, n);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) return CEL_OK;
  if (!d_eds || !d_index || !d_row_roots || !d_col_roots) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_index)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds and d_index must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_row_roots) | reinterpret_cast<uintptr_t>(d_col_roots)) & 1)
    return fail(ctx, CEL_EINVAL, "d_row_roots and d_col_roots must be 2-byte aligned");
  DeviceGuard g(ctx->device);
  return index_batch_enqueue(ctx, static_cast<const uint8_t*>(d_eds), n, k, d_index, static_cast<uint8_t*>(d_row_roots),
                             static_cast<uint8_t*>(d_col_roots), static_cast<uint8_t*>(d_dah), status,
                             (flags & CEL_FLAG_ORDER_CHECK) != 0, pick_stream(ctx, stream));
}

size_t cel_dev_prove_squares_workspace_size(uint32_t n) {
  return align256((size_t)(n ? n : 1) * sizeof(prove::SquareRequest));
}

cel_status cel_dev_prove_squares(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k, uint32_t n_squares,
                                 uint32_t n, const uint32_t* squares, const uint8_t* axes, const uint32_t* index,
                                 const int32_t* starts, const int32_t* ends, void* d_leaves, void* d_nodes,
                                 void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const std::string err = squares_error(k, n_squares);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) return CEL_OK;
  if (!d_index || !squares || !axes || !index || !starts || !ends || !d_nodes || !d_work || (d_leaves && !d_eds))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (d_leaves && ((reinterpret_cast<uintptr_t>(d_leaves) | reinterpret_cast<uintptr_t>(d_eds)) & 15))
    return fail(ctx, CEL_EINVAL, "d_leaves and d_eds must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_index) & 15) || (reinterpret_cast<uintptr_t>(d_work) & 15))
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_nodes) & 1) return fail(ctx, CEL_EINVAL, "d_nodes must be 2-byte aligned");
  DeviceGuard g(ctx->device);
  // n > 0 with n_squares = 0: request 0's square is out of range
  return prove_enqueue(ctx, static_cast<const uint8_t*>(d_eds), d_index, k, n, axes, index, starts, ends,
                       static_cast<uint8_t*>(d_leaves), static_cast<uint8_t*>(d_nodes), d_work,
                       pick_stream(ctx, stream), squares, n_squares);
}

cel_status cel_prove_samples_squares(cel_ctx* ctx, const uint8_t* eds, uint32_t n_squares, uint32_t k, uint32_t n,
                                     const uint32_t* squares, const uint32_t* rows, const uint32_t* cols,
                                     const uint8_t* axes, uint8_t* shares_out, uint8_t* nodes_out,
                                     uint64_t* node_off_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const std::string err = squares_error(k, n_squares);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (!node_off_out) return fail(ctx, CEL_EINVAL, "nil argument");
  if (n == 0) {
    node_off_out[0] = 0;
    return CEL_OK;
  }
  if (!eds || !squares || !rows || !cols || !axes || !shares_out || !nodes_out)
    return fail(ctx, CEL_EINVAL, "nil argument");
  const prove::IndexLayout x = prove::index_layout(k);
  const uint32_t W = x.W;
  std::vector<uint32_t> index(n);
  std::vector<int32_t> starts(n), ends(n);
  for (uint32_t i = 0; i < n; i++) {
    if (squares[i] >= n_squares)
      return fail(ctx, CEL_EINVAL, "sample " + std::to_string(i) + ": square " + std::to_string(squares[i]) + " of " +
                                       std::to_string(n_squares));
    if (rows[i] >= W || cols[i] >= W)
      return fail(ctx, CEL_EINVAL, "sample " + std::to_string(i) + ": cell (" + std::to_string(rows[i]) + ", " +
                                       std::to_string(cols[i]) + ") outside the square of width " + std::to_string(W));
    if (axes[i] > 1) return fail(ctx, CEL_EINVAL, "sample " + std::to_string(i) + ": axis " + std::to_string(axes[i]));
    index[i] = axes[i] ? cols[i] : rows[i];
    starts[i] = (int32_t)(axes[i] ? rows[i] : cols[i]);
    ends[i] = starts[i] + 1;
  }
  for (uint32_t i = 0; i <= n; i++) node_off_out[i] = (uint64_t)i * x.L;  // a single leaf of 2^L: L nodes
  const size_t eds_b = (size_t)n_squares * W * W * kShare, leaf_b = (size_t)n * kShare,
               node_b = (size_t)node_off_out[n] * kNode;
  DeviceGuard g(ctx->device);
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  void* d_index = scratch(ctx, S_WORK, (size_t)n_squares * prove::index_bytes(W), &e);
  uint8_t* d_leaves = static_cast<uint8_t*>(scratch(ctx, S_IN, leaf_b, &e));
  uint8_t* d_nodes = static_cast<uint8_t*>(scratch(ctx, S_AUX, node_b, &e));
  uint8_t* d_roots = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)n_squares * 2 * W * kNode, &e));
  void* d_req = scratch(ctx, S_MASK, (size_t)n * sizeof(prove::SquareRequest), &e);
  if (!d_eds || !d_index || !d_leaves || !d_nodes || !d_roots || !d_req)
    return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, eds_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  cel_status st = index_batch_enqueue(ctx, d_eds, n_squares, k, d_index, d_roots, d_roots + (size_t)n_squares * W * kNode,
                                      nullptr, nullptr, false, s);
  if (st) return st;
  st = prove_enqueue(ctx, d_eds, d_index, k, n, axes, index.data(), starts.data(), ends.data(), d_leaves, d_nodes, d_req,
                     s, squares, n_squares);
  if (st) return st;
  if ((e = hipMemcpyAsync(shares_out, d_leaves, leaf_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if (node_b && (e = hipMemcpyAsync(nodes_out, d_nodes, node_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

size_t cel_dev_tree_index_size(uint32_t k) { return index_width(k) ? (size_t)prove::index_layout(k).bytes : 0; }

cel_status cel_dev_tree_index_build(cel_ctx* ctx, const void* d_eds, uint32_t k, void* d_index, void* d_row_roots,
                                    void* d_col_roots, void* d_dah, int32_t* status, uint32_t flags, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!d_eds || !d_index || !d_row_roots || !d_col_roots) return fail(ctx, CEL_EINVAL, "nil argument");
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_index)) & 15)
    return fail(ctx, CEL_EINVAL, "d_eds and d_index must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  hipStream_t s = pick_stream(ctx, stream);
  uint8_t* base = static_cast<uint8_t*>(d_index);
  int32_t* d_status = reinterpret_cast<int32_t*>(base + prove::index_layout(k).status_off);
  hipError_t e = launch_tree_index(static_cast<const uint8_t*>(d_eds), k, d_index, static_cast<uint8_t*>(d_row_roots),
                                   static_cast<uint8_t*>(d_col_roots), static_cast<uint8_t*>(d_dah),
                                   status ? d_status : nullptr, (flags & CEL_FLAG_ORDER_CHECK) != 0, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "tree index");
  if (status && (e = hipMemcpyAsync(status, d_status, 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  return CEL_OK;
}

cel_status cel_prove_offsets(uint32_t k, uint32_t n, const int32_t* starts, const int32_t* ends, uint64_t* leaf_off,
                             uint64_t* node_off) {
  offsets_error.clear();
  if (!index_width(k) || !leaf_off || !node_off || (n && (!starts || !ends))) {
    offsets_error = "nil argument or a width that is not a power of two up to " + std::to_string(kMaxGf16Width);
    return CEL_EINVAL;
  }
  return offsets(k, n, starts, ends, leaf_off, node_off, &offsets_error);
}

const char* cel_prove_last_error(void) { return offsets_error.c_str(); }

size_t cel_dev_prove_workspace_size(uint32_t n) { return align256((size_t)(n ? n : 1) * sizeof(prove::Request)); }

cel_status cel_dev_prove_batch(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k, uint32_t n,
                               const uint8_t* axes, const uint32_t* index, const int32_t* starts, const int32_t* ends,
                               void* d_leaves, void* d_nodes, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if (n == 0) return CEL_OK;
  if (!d_index || !axes || !index || !starts || !ends || !d_nodes || !d_work || (d_leaves && !d_eds))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (d_leaves && ((reinterpret_cast<uintptr_t>(d_leaves) | reinterpret_cast<uintptr_t>(d_eds)) & 15))
    return fail(ctx, CEL_EINVAL, "d_leaves and d_eds must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_index) & 15) || (reinterpret_cast<uintptr_t>(d_work) & 15))
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_nodes) & 1) return fail(ctx, CEL_EINVAL, "d_nodes must be 2-byte aligned");
  DeviceGuard g(ctx->device);
  return prove_enqueue(ctx, static_cast<const uint8_t*>(d_eds), d_index, k, n, axes, index, starts, ends,
                       static_cast<uint8_t*>(d_leaves), static_cast<uint8_t*>(d_nodes), d_work,
                       pick_stream(ctx, stream));
}

cel_status cel_prove_ranges(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n, const uint8_t* axes,
                            const uint32_t* index, const int32_t* starts, const int32_t* ends, uint8_t* leaves_out,
                            uint8_t* nodes_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if (n == 0) return CEL_OK;
  if (!eds || !axes || !index || !starts || !ends || !nodes_out) return fail(ctx, CEL_EINVAL, "nil argument");
  return prove_host(ctx, eds, k, n, axes, index, starts, ends, leaves_out, nodes_out, nullptr);
}

cel_status cel_prove_samples(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n, const uint32_t* rows,
                             const uint32_t* cols, const uint8_t* axes, uint8_t* shares_out, uint8_t* nodes_out,
                             uint64_t* node_off_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if (!node_off_out) return fail(ctx, CEL_EINVAL, "nil argument");
  node_off_out[0] = 0;
  if (n == 0) return CEL_OK;
  if (!eds || !rows || !cols || !axes || !shares_out || !nodes_out) return fail(ctx, CEL_EINVAL, "nil argument");
  // sample i as proof i: leaf cols[i] of row rows[i], or leaf rows[i] of column cols[i]
  const uint32_t W = 2 * k;
  std::vector<uint32_t> index(n);
  std::vector<int32_t> starts(n), ends(n);
  for (uint32_t i = 0; i < n; i++) {
    if (rows[i] >= W || cols[i] >= W)
      return fail(ctx, CEL_EINVAL, "sample " + std::to_string(i) + ": cell (" + std::to_string(rows[i]) + ", " +
                                       std::to_string(cols[i]) + ") outside the square of width " + std::to_string(W));
    if (axes[i] > 1) return fail(ctx, CEL_EINVAL, "sample " + std::to_string(i) + ": axis " + std::to_string(axes[i]));
    index[i] = axes[i] ? cols[i] : rows[i];
    starts[i] = (int32_t)(axes[i] ? rows[i] : cols[i]);
    ends[i] = starts[i] + 1;
  }
  return prove_host(ctx, eds, k, n, axes, index.data(), starts.data(), ends.data(), shares_out, nodes_out,
                    node_off_out);
}

}  // extern "C"
