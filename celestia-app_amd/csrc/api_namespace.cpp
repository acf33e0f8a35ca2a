// C ABI of the namespace queries (include/celestia_eds.h):
//   cel_dev_namespace_plan / cel_dev_namespace_prove  <- nmt v0.22.0 ProveNamespace [dep] for every
//       (namespace, row) of a batch over one resident square: what celestia-node's
//       GetSharesByNamespace asks of every row whose root range holds the namespace
//   cel_namespace_rows                                 the same for a square in host memory
//   cel_dev_namespace_plan_squares / cel_dev_namespace_prove_squares / cel_namespace_rows_squares
//       the same over a batch index: a query is a (square, namespace) pair, one plan for all
// The plan's sizes depend on the data, so the device finds, counts and places the entries
// (nmt_namespace.hip) and the plan call waits for the counts. The verifier of these proofs
// (cel_nmt_verify_namespace_batch) is in api_verify.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "cel_internal.hpp"
#include "nmt_namespace.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

bool plan_width(uint32_t k) { return is_pow2(k) && k <= 512; }

// "" if the n namespaces can be planned over a square of width k, else what is wrong.
std::string plan_error(uint32_t k, uint32_t n, const uint8_t* namespaces) {
  if (!plan_width(k)) return "square width " + std::to_string(k) + " is not a power of two up to 512";
  if ((uint64_t)n * 2 * k > 0xFFFFFFFFull) return "n * 2k does not fit 32 bits";
  for (uint32_t i = 0; i < n; i++) {
    bool parity = true;
    for (uint32_t j = 0; j < kNs; j++) parity = parity && namespaces[(size_t)i * kNs + j] == 0xFF;
    if (parity) return "namespace " + std::to_string(i) + " is the parity namespace, which holds no data";
  }
  return "";
}

// The same for n (square, namespace) queries over a batch index of n_squares squares: the
// query's square comes first, so that a request to a square that is not there is named as such.
std::string squares_plan_error(uint32_t k, uint32_t n_squares, uint32_t n, const uint32_t* squares,
                               const uint8_t* namespaces) {
  if (!plan_width(k)) return "square width " + std::to_string(k) + " is not a power of two up to 512";
  if (n_squares > prove::kMaxSquares)
    return std::to_string(n_squares) + " squares are more than one call takes (" + std::to_string(prove::kMaxSquares) +
           ")";
  for (uint32_t i = 0; i < n; i++)
    if (squares[i] >= n_squares)
      return "query " + std::to_string(i) + ": square " + std::to_string(squares[i]) + " of " +
             std::to_string(n_squares);
  return plan_error(k, n, namespaces);
}

struct PlanOut {
  uint64_t cap;
  uint32_t *ns_idx, *rows;
  int32_t *starts, *ends;
  uint8_t* kinds;
  uint64_t *leaf_off, *node_off;
  bool none() const { return !ns_idx && !rows && !starts && !ends && !kinds && !leaf_off && !node_off; }
  bool all() const { return ns_idx && rows && starts && ends && kinds && leaf_off && node_off; }
};

// The plan of n checked namespaces into d_work and, where there is room, into `out`; the totals
// into *tot. Synchronous on s. ctx->mu held, device current.
// squares != nullptr: a plan over a batch index, query i on square squares[i] (checked).
cel_status plan_locked(cel_ctx* ctx, const void* d_index, uint32_t k, uint32_t n, const uint8_t* namespaces,
                       const PlanOut& out, nsq::Sums* tot, void* d_work, hipStream_t s,
                       const uint32_t* squares = nullptr) {
  const nsq::Work w = nsq::carve(d_work, k, n);
  cel_status st = CEL_OK;
  const size_t ns_b = (size_t)n * 32;
  uint8_t* stage = static_cast<uint8_t*>(plan_stage(ctx, ns_b + sizeof(nsq::Head), &st));
  if (!stage) return st;
  for (uint32_t i = 0; i < n; i++)
    nsq::query_row(stage + (size_t)i * 32, namespaces + (size_t)i * kNs, squares ? squares[i] : 0);
  hipError_t e;
  // no plan_uploaded behind this copy: the call waits for s below, before anyone refills the buffer
  if ((e = hipMemcpyAsync(w.ns, stage, ns_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  // Measurement aid (tools/namespace_bench.py): CEL_NS_PLAN_STAGES = a mask of the stages to run
  // (1 find, 2 prefix sum and compaction) over what the others left in the workspace.
  int stages = 3;
  if (const char* env = std::getenv("CEL_NS_PLAN_STAGES")) stages = std::atoi(env) & 3;
  e = squares ? launch_ns_plan_squares(d_index, k, n, w, s) : launch_ns_plan(d_index, k, n, w, stages, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "namespace plan");
  nsq::Head* head = reinterpret_cast<nsq::Head*>(stage + ns_b);
  if ((e = hipMemcpyAsync(head, w.head, sizeof(nsq::Head), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  *tot = head->totals;
  if (tot->entries > w.npairs) return fail(ctx, CEL_EDEVICE, "namespace plan: more entries than pairs");
  if (out.cap == 0 && out.none()) return CEL_OK;
  if (out.cap < tot->entries)
    return fail(ctx, CEL_EINVAL, "cap " + std::to_string(out.cap) + " is below the " + std::to_string(tot->entries) +
                                     " entries of the plan");
  const size_t req_b = (size_t)tot->entries * sizeof(nsq::Request);
  nsq::Request* req = static_cast<nsq::Request*>(plan_stage(ctx, req_b, &st));
  if (!req) return st;
  if (req_b) {
    if ((e = hipMemcpyAsync(req, w.req, req_b, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  }
  for (uint64_t i = 0; i < tot->entries; i++) {
    const nsq::Request& q = req[i];
    out.ns_idx[i] = q.ns_idx;
    out.rows[i] = q.row;
    out.starts[i] = q.start;
    out.ends[i] = q.end;
    out.kinds[i] = (uint8_t)q.kind;
    out.leaf_off[i] = q.leaf0;
    out.node_off[i] = q.node0;
  }
  out.leaf_off[tot->entries] = tot->leaves;
  out.node_off[tot->entries] = tot->nodes;
  return CEL_OK;
}

}  // namespace

extern "C" {

size_t cel_dev_namespace_workspace_size(uint32_t k, uint32_t n) {
  if (!plan_width(k) || (uint64_t)n * 2 * k > 0xFFFFFFFFull) return 0;
  return nsq::carve(nullptr, k, n).bytes;
}

cel_status cel_dev_namespace_plan(cel_ctx* ctx, const void* d_index, uint32_t k, uint32_t n, const uint8_t* namespaces,
                                  uint64_t cap, uint32_t* ns_idx, uint32_t* rows, int32_t* starts, int32_t* ends,
                                  uint8_t* kinds, uint64_t* leaf_off, uint64_t* node_off, uint64_t* n_entries,
                                  void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_entries) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_entries = 0;
  const PlanOut out{cap, ns_idx, rows, starts, ends, kinds, leaf_off, node_off};
  if (!out.none() && !out.all()) return fail(ctx, CEL_EINVAL, "nil argument");
  if (cap && !out.all()) return fail(ctx, CEL_EINVAL, "nil argument");
  if (n && !namespaces) return fail(ctx, CEL_EINVAL, "nil argument");
  const std::string err = plan_error(k, n, namespaces);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) {
    if (out.all()) leaf_off[0] = node_off[0] = 0;
    return CEL_OK;
  }
  if (!d_index || !d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_index) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  nsq::Sums tot{};
  const cel_status st = plan_locked(ctx, d_index, k, n, namespaces, out, &tot, d_work, pick_stream(ctx, stream));
  if (st == CEL_OK || st == CEL_EINVAL) *n_entries = tot.entries;
  return st;
}

cel_status cel_dev_namespace_prove(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k, uint64_t n_entries,
                                   void* d_leaves, void* d_nodes, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!plan_width(k)) return fail(ctx, CEL_EINVAL, "square width " + std::to_string(k) + " is not a power of two up to 512");
  if (n_entries > 0xFFFFFFFFull) return fail(ctx, CEL_EINVAL, "more entries than any plan holds");
  if (n_entries == 0) return CEL_OK;
  if (!d_index || !d_nodes || !d_work || (d_leaves && !d_eds)) return fail(ctx, CEL_EINVAL, "nil argument");
  if (d_leaves && ((reinterpret_cast<uintptr_t>(d_leaves) | reinterpret_cast<uintptr_t>(d_eds)) & 15))
    return fail(ctx, CEL_EINVAL, "d_leaves and d_eds must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_index) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_nodes) & 1) return fail(ctx, CEL_EINVAL, "d_nodes must be 2-byte aligned");
  DeviceGuard g(ctx->device);
  const hipError_t e = launch_ns_emit(static_cast<const uint8_t*>(d_eds), d_index, k, d_work, (uint32_t)n_entries,
                                      static_cast<uint8_t*>(d_leaves), static_cast<uint8_t*>(d_nodes),
                                      pick_stream(ctx, stream));
  return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "namespace prove");
}

cel_status cel_namespace_rows(cel_ctx* ctx, const uint8_t* eds, uint32_t k, uint32_t n, const uint8_t* namespaces,
                              uint64_t cap, uint64_t leaf_cap, uint64_t node_cap, uint32_t* ns_idx, uint32_t* rows,
                              int32_t* starts, int32_t* ends, uint8_t* kinds, uint64_t* leaf_off, uint64_t* node_off,
                              uint8_t* leaves_out, uint8_t* nodes_out, uint64_t* n_entries, uint64_t* total_leaves,
                              uint64_t* total_nodes) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_entries || !total_leaves || !total_nodes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_entries = *total_leaves = *total_nodes = 0;
  const PlanOut out{cap, ns_idx, rows, starts, ends, kinds, leaf_off, node_off};
  const bool count_only = cap == 0 && out.none() && !leaves_out && !nodes_out;
  if (!count_only && (!out.all() || (leaf_cap && !leaves_out) || (node_cap && !nodes_out)))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (n && !namespaces) return fail(ctx, CEL_EINVAL, "nil argument");
  const std::string err = plan_error(k, n, namespaces);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) {
    if (out.all()) leaf_off[0] = node_off[0] = 0;
    return CEL_OK;
  }
  if (!eds) return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  const prove::IndexLayout x = prove::index_layout(k);
  const size_t eds_b = (size_t)4 * k * k * kShare;
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  uint8_t* d_index = static_cast<uint8_t*>(scratch(ctx, S_WORK, x.bytes, &e));
  uint8_t* d_roots = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)4 * k * kNode, &e));
  void* d_work = scratch(ctx, S_MASK, nsq::carve(nullptr, k, n).bytes, &e);
  if (!d_eds || !d_index || !d_roots || !d_work) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, eds_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  int32_t* d_status = reinterpret_cast<int32_t*>(d_index + x.status_off);
  if ((e = launch_tree_index(d_eds, k, d_index, d_roots, d_roots + (size_t)2 * k * kNode, nullptr, d_status, true, s)) !=
      hipSuccess)
    return hip_fail(ctx, e, "tree index");
  int32_t* h_status = static_cast<int32_t*>(host_stage(ctx, 256));
  if (!h_status) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  if ((e = hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  if (*h_status != CEL_OK)
    return fail(ctx, CEL_EORDER, "invalid push order: a namespace is smaller than the previous one");
  nsq::Sums tot{};
  // the entry arrays are written only when the shares and nodes fit as well: count first
  const PlanOut count{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  cel_status st = plan_locked(ctx, d_index, k, n, namespaces, count, &tot, d_work, s);
  if (st) return st;
  *n_entries = tot.entries;
  *total_leaves = tot.leaves;
  *total_nodes = tot.nodes;
  if (count_only) return CEL_OK;
  if (cap < tot.entries || leaf_cap < tot.leaves || node_cap < tot.nodes)
    return fail(ctx, CEL_EINVAL, "caps (" + std::to_string(cap) + ", " + std::to_string(leaf_cap) + ", " +
                                     std::to_string(node_cap) + ") are below the plan's " + std::to_string(tot.entries) +
                                     " entries, " + std::to_string(tot.leaves) + " shares, " +
                                     std::to_string(tot.nodes) + " nodes");
  if ((st = plan_locked(ctx, d_index, k, n, namespaces, out, &tot, d_work, s)) != CEL_OK) return st;
  const size_t leaf_b = (size_t)tot.leaves * kShare, node_b = (size_t)tot.nodes * kNode;
  uint8_t* d_leaves = static_cast<uint8_t*>(scratch(ctx, S_IN, leaf_b, &e));
  uint8_t* d_nodes = static_cast<uint8_t*>(scratch(ctx, S_AUX, node_b, &e));
  if (!d_leaves || !d_nodes) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  if ((e = launch_ns_emit(d_eds, d_index, k, d_work, (uint32_t)tot.entries, d_leaves, d_nodes, s)) != hipSuccess)
    return hip_fail(ctx, e, "namespace prove");
  if (leaf_b && (e = hipMemcpyAsync(leaves_out, d_leaves, leaf_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if (node_b && (e = hipMemcpyAsync(nodes_out, d_nodes, node_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

// ------------------------------------------------------------- over a batch index

size_t cel_dev_namespace_squares_workspace_size(uint32_t k, uint32_t n) { return cel_dev_namespace_workspace_size(k, n); }

cel_status cel_dev_namespace_plan_squares(cel_ctx* ctx, const void* d_index, uint32_t k, uint32_t n_squares, uint32_t n,
                                          const uint32_t* squares, const uint8_t* namespaces, uint64_t cap,
                                          uint32_t* query_idx, uint32_t* rows, int32_t* starts, int32_t* ends,
                                          uint8_t* kinds, uint64_t* leaf_off, uint64_t* node_off, uint64_t* n_entries,
                                          void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_entries) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_entries = 0;
  const PlanOut out{cap, query_idx, rows, starts, ends, kinds, leaf_off, node_off};
  if (!out.none() && !out.all()) return fail(ctx, CEL_EINVAL, "nil argument");
  if (cap && !out.all()) return fail(ctx, CEL_EINVAL, "nil argument");
  if (n && (!namespaces || !squares)) return fail(ctx, CEL_EINVAL, "nil argument");
  const std::string err = squares_plan_error(k, n_squares, n, squares, namespaces);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) {
    if (out.all()) leaf_off[0] = node_off[0] = 0;
    return CEL_OK;
  }
  if (!d_index || !d_work) return fail(ctx, CEL_EINVAL, "nil argument");
  if ((reinterpret_cast<uintptr_t>(d_index) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  nsq::Sums tot{};
  const cel_status st =
      plan_locked(ctx, d_index, k, n, namespaces, out, &tot, d_work, pick_stream(ctx, stream), squares);
  if (st == CEL_OK || st == CEL_EINVAL) *n_entries = tot.entries;
  return st;
}

cel_status cel_dev_namespace_prove_squares(cel_ctx* ctx, const void* d_eds, const void* d_index, uint32_t k,
                                           uint32_t n_squares, uint64_t n_entries, void* d_leaves, void* d_nodes,
                                           void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const std::string err = squares_plan_error(k, n_squares, 0, nullptr, nullptr);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n_entries > 0xFFFFFFFFull) return fail(ctx, CEL_EINVAL, "more entries than any plan holds");
  if (n_entries == 0 || n_squares == 0) return CEL_OK;
  if (!d_index || !d_nodes || !d_work || (d_leaves && !d_eds)) return fail(ctx, CEL_EINVAL, "nil argument");
  if (d_leaves && ((reinterpret_cast<uintptr_t>(d_leaves) | reinterpret_cast<uintptr_t>(d_eds)) & 15))
    return fail(ctx, CEL_EINVAL, "d_leaves and d_eds must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_index) | reinterpret_cast<uintptr_t>(d_work)) & 15)
    return fail(ctx, CEL_EINVAL, "d_index and d_work must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_nodes) & 1) return fail(ctx, CEL_EINVAL, "d_nodes must be 2-byte aligned");
  DeviceGuard g(ctx->device);
  const hipError_t e = launch_ns_emit_squares(static_cast<const uint8_t*>(d_eds), d_index, k, n_squares, d_work,
                                              (uint32_t)n_entries, static_cast<uint8_t*>(d_leaves),
                                              static_cast<uint8_t*>(d_nodes), pick_stream(ctx, stream));
  return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "namespace prove");
}

cel_status cel_namespace_rows_squares(cel_ctx* ctx, const uint8_t* eds, uint32_t n_squares, uint32_t k, uint32_t n,
                                      const uint32_t* squares, const uint8_t* namespaces, uint64_t cap,
                                      uint64_t leaf_cap, uint64_t node_cap, uint32_t* query_idx, uint32_t* rows,
                                      int32_t* starts, int32_t* ends, uint8_t* kinds, uint64_t* leaf_off,
                                      uint64_t* node_off, uint8_t* leaves_out, uint8_t* nodes_out, uint64_t* n_entries,
                                      uint64_t* total_leaves, uint64_t* total_nodes) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!n_entries || !total_leaves || !total_nodes) return fail(ctx, CEL_EINVAL, "nil argument");
  *n_entries = *total_leaves = *total_nodes = 0;
  const PlanOut out{cap, query_idx, rows, starts, ends, kinds, leaf_off, node_off};
  const bool count_only = cap == 0 && out.none() && !leaves_out && !nodes_out;
  if (!count_only && (!out.all() || (leaf_cap && !leaves_out) || (node_cap && !nodes_out)))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (n && (!namespaces || !squares)) return fail(ctx, CEL_EINVAL, "nil argument");
  const std::string err = squares_plan_error(k, n_squares, n, squares, namespaces);
  if (!err.empty()) return fail(ctx, CEL_EINVAL, err);
  if (n == 0) {
    if (out.all()) leaf_off[0] = node_off[0] = 0;
    return CEL_OK;
  }
  if (!eds) return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  const uint32_t W = 2 * k;
  const size_t eds_b = (size_t)n_squares * W * W * kShare;
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  uint8_t* d_index = static_cast<uint8_t*>(scratch(ctx, S_WORK, (size_t)n_squares * prove::index_bytes(W), &e));
  uint8_t* d_roots = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, (size_t)n_squares * 2 * W * kNode, &e));
  void* d_work = scratch(ctx, S_MASK, nsq::carve(nullptr, k, n).bytes, &e);
  if (!d_eds || !d_index || !d_roots || !d_work) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemcpyAsync(d_eds, eds, eds_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  std::vector<int32_t> status(n_squares, 0);
  cel_status st = index_batch_enqueue(ctx, d_eds, n_squares, k, d_index, d_roots,
                                      d_roots + (size_t)n_squares * W * kNode, nullptr, status.data(), true, s);
  if (st) return st;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  for (uint32_t i = 0; i < n_squares; i++)
    if (status[i] != CEL_OK)
      return fail(ctx, CEL_EORDER, "square " + std::to_string(i) +
                                       ": invalid push order: a namespace is smaller than the previous one");
  nsq::Sums tot{};
  // the entry arrays are written only when the shares and nodes fit as well: count first
  const PlanOut count{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if ((st = plan_locked(ctx, d_index, k, n, namespaces, count, &tot, d_work, s, squares)) != CEL_OK) return st;
  *n_entries = tot.entries;
  *total_leaves = tot.leaves;
  *total_nodes = tot.nodes;
  if (count_only) return CEL_OK;
  if (cap < tot.entries || leaf_cap < tot.leaves || node_cap < tot.nodes)
    return fail(ctx, CEL_EINVAL, "caps (" + std::to_string(cap) + ", " + std::to_string(leaf_cap) + ", " +
                                     std::to_string(node_cap) + ") are below the plan's " + std::to_string(tot.entries) +
                                     " entries, " + std::to_string(tot.leaves) + " shares, " +
                                     std::to_string(tot.nodes) + " nodes");
  if ((st = plan_locked(ctx, d_index, k, n, namespaces, out, &tot, d_work, s, squares)) != CEL_OK) return st;
  const size_t leaf_b = (size_t)tot.leaves * kShare, node_b = (size_t)tot.nodes * kNode;
  uint8_t* d_leaves = static_cast<uint8_t*>(scratch(ctx, S_IN, leaf_b, &e));
  uint8_t* d_nodes = static_cast<uint8_t*>(scratch(ctx, S_AUX, node_b, &e));
  if (!d_leaves || !d_nodes) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  if ((e = launch_ns_emit_squares(d_eds, d_index, k, n_squares, d_work, (uint32_t)tot.entries, d_leaves, d_nodes, s)) !=
      hipSuccess)
    return hip_fail(ctx, e, "namespace prove");
  if (leaf_b && (e = hipMemcpyAsync(leaves_out, d_leaves, leaf_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if (node_b && (e = hipMemcpyAsync(nodes_out, d_nodes, node_b, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

}  // extern "C"
