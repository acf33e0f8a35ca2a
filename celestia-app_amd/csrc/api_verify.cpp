// C ABI of the batched NMT proof verifiers and of the repair from proven samples
// (include/celestia_eds.h):
//   cel_nmt_verify_batch / cel_dev_nmt_verify_batch  <- nmt Proof.VerifyInclusion (nmt v0.22.0
//       proof.go [dep]) for every proof of a batch: the NMT range proofs of ShareProofs
//       (pkg/proof/share_proof.go:60-82) and of sampled cells
//   cel_dev_place_samples  <- cells with single-leaf proofs against the DAH's row or column
//       roots, checked and then written into a resident EDS
//   cel_repair_samples     <- the same into an empty square, then cel_dev_repair
//   cel_nmt_verify_namespace_batch / cel_dev_nmt_verify_namespace_batch  <- nmt
//       Proof.VerifyNamespace [dep]: the same host side with the proofs' kinds in the table
// The host flattens the proofs into a table (nmt_verify.hpp) and picks the sample that
// fills each cell; every hash runs in nmt_verify.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "cel_internal.hpp"
#include "nmt_verify.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

constexpr uint64_t kMaxRecords = 1ull << 31;  // leaves, nodes: record indices fit 32 bits with room

// A batch of proofs under one of the two rules: kinds == nullptr is VerifyInclusion, else
// VerifyNamespace with kinds[i] the kind of proof i (CEL_NS_INCLUSION / CEL_NS_ABSENCE).
struct Batch {
  uint32_t n;
  const int32_t *starts, *ends;
  const uint8_t* kinds;
  const uint8_t* namespaces;
  const uint64_t *leaf_off, *node_off;
  uint32_t nroots;
  const uint32_t* root_idx;
  bool by_namespace() const { return kinds != nullptr; }
  uint64_t total_leaves() const { return leaf_off[n] - leaf_off[0]; }
  uint64_t total_nodes() const { return node_off[n] - node_off[0]; }
};

// The call errors of a batch (n > 0, pointers checked by the caller).
cel_status check_batch(cel_ctx* ctx, const Batch& b) {
  for (uint32_t i = 0; i < b.n; i++) {
    if (b.leaf_off[i + 1] < b.leaf_off[i]) return fail(ctx, CEL_EINVAL, "leaf offsets must be non-decreasing");
    if (b.node_off[i + 1] < b.node_off[i]) return fail(ctx, CEL_EINVAL, "node offsets must be non-decreasing");
    if (b.root_idx[i] >= b.nroots)
      return fail(ctx, CEL_EINVAL, "proof " + std::to_string(i) + ": root index " + std::to_string(b.root_idx[i]) +
                                       " of " + std::to_string(b.nroots) + " roots");
  }
  // the namespace rule keeps one more leaf record per proof (verify_ns_carve), the node
  // records one root per proof under both rules
  const uint64_t own_records = b.by_namespace() ? b.n : 0;
  if (b.total_leaves() + own_records >= kMaxRecords || b.total_nodes() + b.n >= kMaxRecords)
    return fail(ctx, CEL_ETOOBIG, "too many leaves or nodes for one device batch");
  return CEL_OK;
}

// Fills the table of batch b in the ctx's page-locked plan buffer (api_common.hpp: plan_stage),
// uploads it into d_work's head and enqueues the kernels of b's rule on s. d_leaves / d_nodes:
// the first leaf / node of the batch. ctx->mu held, device current.
cel_status verify_enqueue(cel_ctx* ctx, const Batch& b, const uint8_t* d_leaves, const uint8_t* d_nodes,
                          const uint8_t* d_roots, uint8_t* d_ok, void* d_work, hipStream_t s) {
  const uint64_t tl = b.total_leaves(), tn = b.total_nodes();
  // the table is the same under both rules; the namespace rule's workspace has more behind it
  VerifyNsWork ns_dev{};
  if (b.by_namespace()) ns_dev = verify_ns_carve(d_work, tl, tn, b.n);
  const VerifyWork dev = b.by_namespace() ? ns_dev.v : verify_carve(d_work, tl, tn, b.n);
  cel_status st = CEL_OK;
  void* stage = plan_stage(ctx, dev.head_bytes, &st);
  if (!stage) return st;
  const VerifyWork host = b.by_namespace() ? verify_ns_carve(stage, tl, tn, b.n).v : verify_carve(stage, tl, tn, b.n);
  for (uint32_t i = 0; i < b.n; i++) {
    VerifyProof& p = host.proofs[i];
    p.start = b.starts[i];
    p.end = b.ends[i];
    const uint64_t nl = b.leaf_off[i + 1] - b.leaf_off[i], nn = b.node_off[i + 1] - b.node_off[i];
    p.nleaves = (uint32_t)nl;
    p.nnodes = (uint32_t)nn;
    p.leaf0 = b.leaf_off[i] - b.leaf_off[0];
    p.node0 = b.node_off[i] - b.node_off[0];
    p.root = b.root_idx[i];
    p.pad = b.by_namespace() ? b.kinds[i] : 0;
    uint8_t* ns = reinterpret_cast<uint8_t*>(host.ns) + (size_t)i * 32;
    std::memcpy(ns, b.namespaces + (size_t)i * kNs, kNs);
    ns[29] = ns[30] = ns[31] = 0;
    for (uint64_t j = 0; j < nl; j++) host.leaf_proof[p.leaf0 + j] = i;
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(d_work, stage, dev.head_bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  if ((st = plan_uploaded(ctx, s)) != CEL_OK) return st;
  // Measurement aid (tools/verify_bench.py, tools/namespace_bench.py): CEL_VERIFY_STAGES = a
  // mask of the stages to run (1 repack, 2 leaves, 4 fold), so that one stage can be timed
  // over the records the others left in the workspace.
  int stages = kVerifyAll;
  if (const char* env = std::getenv("CEL_VERIFY_STAGES")) stages = std::atoi(env) & kVerifyAll;
  if (b.by_namespace()) {
    Range r("nmt_verify_namespace");
    if ((e = launch_verify_ns(ns_dev, d_leaves, tl, d_nodes, tn, d_roots, b.n, d_ok, stages, s)) != hipSuccess)
      return hip_fail(ctx, e, "nmt verify namespace");
  } else {
    Range r("nmt_verify");
    if ((e = launch_verify(dev, d_leaves, tl, d_nodes, tn, d_roots, b.n, d_ok, stages, s)) != hipSuccess)
      return hip_fail(ctx, e, "nmt verify");
  }
  return CEL_OK;
}

// One host array of a call on its way to the device: page-locked memory is copied in place,
// pageable memory through the ctx's page-locked staging at `at` (the caller sized it).
cel_status upload(cel_ctx* ctx, void* dst, const void* src, size_t bytes, uint8_t* stage, size_t* at, hipStream_t s) {
  if (!bytes) return CEL_OK;
  if (!page_locked(src)) {
    std::memcpy(stage + *at, src, bytes);
    src = stage + *at;
    *at += align256(bytes);
  }
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "H2D");
}

// A batch of host proofs: uploads, kernels, verdicts back into ok_out. Synchronous. The
// leaves stay in scratch S_IN (*d_leaves_out) and S_ROOTS has `extra` more bytes behind the
// verdicts (*d_extra_out) for the caller's next step. ctx->mu held, device current.
cel_status verify_host(cel_ctx* ctx, const Batch& b, const uint8_t* leaves, const uint8_t* nodes, const uint8_t* roots,
                       uint8_t* ok_out, size_t extra, uint8_t** d_leaves_out, uint8_t** d_extra_out) {
  cel_status st = check_batch(ctx, b);
  if (st) return st;
  hipStream_t s = ctx->stream;
  const uint64_t tl = b.total_leaves(), tn = b.total_nodes();
  const size_t leaf_b = (size_t)tl * kShare, node_b = (size_t)tn * kNode, root_b = (size_t)b.nroots * kNode;
  const size_t ok_a = align256(b.n);
  hipError_t e = hipSuccess;
  uint8_t* d_leaves = static_cast<uint8_t*>(scratch(ctx, S_IN, leaf_b, &e));
  uint8_t* d_nodes = static_cast<uint8_t*>(scratch(ctx, S_AUX, align256(node_b) + root_b, &e));
  const size_t work_b = b.by_namespace() ? verify_ns_carve(nullptr, tl, tn, b.n).bytes
                                         : verify_carve(nullptr, tl, tn, b.n).bytes;
  void* d_work = scratch(ctx, S_WORK, work_b, &e);
  uint8_t* d_ok = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, ok_a + extra, &e));
  if (!d_leaves || !d_nodes || !d_work || !d_ok) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  uint8_t* d_roots = d_nodes + align256(node_b);
  uint8_t* hs = static_cast<uint8_t*>(host_stage(ctx, ok_a + align256(leaf_b) + align256(node_b) + align256(root_b)));
  if (!hs) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  size_t at = ok_a;
  if ((st = upload(ctx, d_leaves, leaves + b.leaf_off[0] * kShare, leaf_b, hs, &at, s)) != CEL_OK) return st;
  if ((st = upload(ctx, d_nodes, nodes + b.node_off[0] * kNode, node_b, hs, &at, s)) != CEL_OK) return st;
  if ((st = upload(ctx, d_roots, roots, root_b, hs, &at, s)) != CEL_OK) return st;
  if ((st = verify_enqueue(ctx, b, d_leaves, d_nodes, d_roots, d_ok, d_work, s)) != CEL_OK) return st;
  if ((e = hipMemcpyAsync(hs, d_ok, b.n, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  std::memcpy(ok_out, hs, b.n);
  if (d_leaves_out) *d_leaves_out = d_leaves;
  if (d_extra_out) *d_extra_out = d_ok + ok_a;
  return CEL_OK;
}

// cel_dev_place_samples with ctx->mu held and the arguments checked.
cel_status place_samples_locked(cel_ctx* ctx, uint8_t* d_eds, uint8_t* present, uint32_t k, const uint8_t* row_roots,
                                const uint8_t* col_roots, uint32_t n, const uint32_t* rows, const uint32_t* cols,
                                const uint8_t* axes, const uint8_t* shares, const uint8_t* nodes,
                                const uint64_t* node_off, uint8_t* ok_out) {
  const uint32_t W = 2 * k;
  // sample i as proof i: one leaf (share i) at leaf cols[i] of row root rows[i], or at leaf
  // rows[i] of column root W + cols[i]; the wrapper's namespace rule (nmt_wrapper.go:100-107)
  std::vector<int32_t> starts(n), ends(n);
  std::vector<uint8_t> ns((size_t)n * kNs);
  std::vector<uint64_t> leaf_off((size_t)n + 1);
  std::vector<uint32_t> root_idx(n);
  std::vector<uint8_t> roots((size_t)2 * W * kNode);
  std::memcpy(roots.data(), row_roots, (size_t)W * kNode);
  std::memcpy(roots.data() + (size_t)W * kNode, col_roots, (size_t)W * kNode);
  for (uint32_t i = 0; i < n; i++) {
    leaf_off[i] = i;
    const bool valid = rows[i] < W && cols[i] < W && axes[i] <= 1;
    if (!valid) {  // verdict 0 in the fold (start < 0)
      starts[i] = -1;
      ends[i] = 0;
      root_idx[i] = 0;
      std::memset(&ns[(size_t)i * kNs], 0, kNs);
      continue;
    }
    starts[i] = (int32_t)(axes[i] ? rows[i] : cols[i]);
    ends[i] = starts[i] + 1;
    root_idx[i] = axes[i] ? W + cols[i] : rows[i];
    if (rows[i] < k && cols[i] < k)
      std::memcpy(&ns[(size_t)i * kNs], shares + (size_t)i * kShare, kNs);
    else
      std::memset(&ns[(size_t)i * kNs], 0xFF, kNs);
  }
  leaf_off[n] = n;
  const Batch b{n, starts.data(), ends.data(), nullptr, ns.data(), leaf_off.data(), node_off, 2 * W, root_idx.data()};
  uint8_t *d_shares = nullptr, *d_lists = nullptr;
  cel_status st = verify_host(ctx, b, shares, nodes, roots.data(), ok_out, (size_t)n * 8, &d_shares, &d_lists);
  if (st) return st;
  // the writer of each absent cell: its accepted sample of lowest index
  uint32_t* hl = static_cast<uint32_t*>(host_stage(ctx, (size_t)n * 8));
  if (!hl) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  uint32_t nw = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!ok_out[i] || rows[i] >= W || cols[i] >= W) continue;
    const size_t cell = (size_t)rows[i] * W + cols[i];
    if (present[cell]) continue;
    present[cell] = 1;
    hl[nw] = i;
    hl[n + nw] = (uint32_t)cell;
    nw++;
  }
  if (nw == 0) return CEL_OK;
  hipStream_t s = ctx->stream;
  hipError_t e;
  if ((e = hipMemcpyAsync(d_lists, hl, (size_t)n * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  const uint32_t* dl = reinterpret_cast<const uint32_t*>(d_lists);
  if ((e = launch_place_shares(d_shares, dl, dl + n, nw, d_eds, s)) != hipSuccess) return hip_fail(ctx, e, "place");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

bool samples_nil(const uint8_t* row_roots, const uint8_t* col_roots, uint32_t n, const uint32_t* rows,
                 const uint32_t* cols, const uint8_t* axes, const uint8_t* shares, const uint8_t* nodes,
                 const uint64_t* node_off, const uint8_t* ok_out) {
  return !row_roots || !col_roots || (n && (!rows || !cols || !axes || !shares || !nodes || !node_off || !ok_out));
}

}  // namespace

extern "C" {

cel_status cel_nmt_verify_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                const uint8_t* namespaces, const uint8_t* leaves, const uint64_t* leaf_off,
                                const uint8_t* nodes, const uint64_t* node_off, const uint8_t* roots, uint32_t nroots,
                                const uint32_t* root_idx, uint8_t* ok_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (n == 0) return CEL_OK;
  if (!starts || !ends || !namespaces || !leaves || !leaf_off || !nodes || !node_off || !roots || !root_idx || !ok_out)
    return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  const Batch b{n, starts, ends, nullptr, namespaces, leaf_off, node_off, nroots, root_idx};
  return verify_host(ctx, b, leaves, nodes, roots, ok_out, 0, nullptr, nullptr);
}

size_t cel_dev_nmt_verify_workspace_size(uint64_t total_leaves, uint64_t total_nodes, uint32_t n) {
  return verify_carve(nullptr, total_leaves, total_nodes, n).bytes;
}

cel_status cel_dev_nmt_verify_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                    const uint8_t* namespaces, const void* d_leaves, const uint64_t* leaf_off,
                                    const void* d_nodes, const uint64_t* node_off, const void* d_roots,
                                    uint32_t nroots, const uint32_t* root_idx, void* d_ok, void* d_work,
                                    void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (n == 0) return CEL_OK;
  if (!starts || !ends || !namespaces || !d_leaves || !leaf_off || !d_nodes || !node_off || !d_roots || !root_idx ||
      !d_ok || !d_work)
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (reinterpret_cast<uintptr_t>(d_leaves) & 15) return fail(ctx, CEL_EINVAL, "d_leaves must be 16-byte aligned");
  const Batch b{n, starts, ends, nullptr, namespaces, leaf_off, node_off, nroots, root_idx};
  cel_status st = check_batch(ctx, b);
  if (st) return st;
  DeviceGuard g(ctx->device);
  return verify_enqueue(ctx, b, static_cast<const uint8_t*>(d_leaves) + leaf_off[0] * kShare,
                        static_cast<const uint8_t*>(d_nodes) + node_off[0] * kNode,
                        static_cast<const uint8_t*>(d_roots), static_cast<uint8_t*>(d_ok), d_work,
                        pick_stream(ctx, stream));
}

size_t cel_dev_nmt_verify_namespace_workspace_size(uint64_t total_leaves, uint64_t total_nodes, uint32_t n) {
  return verify_ns_carve(nullptr, total_leaves, total_nodes, n).bytes;
}

cel_status cel_dev_nmt_verify_namespace_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                              const uint8_t* kinds, const uint8_t* namespaces, const void* d_leaves,
                                              const uint64_t* leaf_off, const void* d_nodes, const uint64_t* node_off,
                                              const void* d_roots, uint32_t nroots, const uint32_t* root_idx,
                                              void* d_ok, void* d_work, void* stream) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (n == 0) return CEL_OK;
  if (!starts || !ends || !kinds || !namespaces || !d_leaves || !leaf_off || !d_nodes || !node_off || !d_roots ||
      !root_idx || !d_ok || !d_work)
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (reinterpret_cast<uintptr_t>(d_leaves) & 15) return fail(ctx, CEL_EINVAL, "d_leaves must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_work) & 15) return fail(ctx, CEL_EINVAL, "d_work must be 16-byte aligned");
  const Batch b{n, starts, ends, kinds, namespaces, leaf_off, node_off, nroots, root_idx};
  cel_status st = check_batch(ctx, b);
  if (st) return st;
  DeviceGuard g(ctx->device);
  return verify_enqueue(ctx, b, static_cast<const uint8_t*>(d_leaves) + leaf_off[0] * kShare,
                        static_cast<const uint8_t*>(d_nodes) + node_off[0] * kNode, static_cast<const uint8_t*>(d_roots),
                        static_cast<uint8_t*>(d_ok), d_work, pick_stream(ctx, stream));
}

cel_status cel_nmt_verify_namespace_batch(cel_ctx* ctx, uint32_t n, const int32_t* starts, const int32_t* ends,
                                          const uint8_t* kinds, const uint8_t* namespaces, const uint8_t* leaves,
                                          const uint64_t* leaf_off, const uint8_t* nodes, const uint64_t* node_off,
                                          const uint8_t* roots, uint32_t nroots, const uint32_t* root_idx,
                                          uint8_t* ok_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (n == 0) return CEL_OK;
  if (!starts || !ends || !kinds || !namespaces || !leaves || !leaf_off || !nodes || !node_off || !roots || !root_idx ||
      !ok_out)
    return fail(ctx, CEL_EINVAL, "nil argument");
  DeviceGuard g(ctx->device);
  const Batch b{n, starts, ends, kinds, namespaces, leaf_off, node_off, nroots, root_idx};
  return verify_host(ctx, b, leaves, nodes, roots, ok_out, 0, nullptr, nullptr);
}

cel_status cel_dev_place_samples(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k, const uint8_t* row_roots,
                                 const uint8_t* col_roots, uint32_t n, const uint32_t* rows, const uint32_t* cols,
                                 const uint8_t* axes, const uint8_t* shares, const uint8_t* nodes,
                                 const uint64_t* node_off, uint8_t* ok_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!d_eds || !present || samples_nil(row_roots, col_roots, n, rows, cols, axes, shares, nodes, node_off, ok_out))
    return fail(ctx, CEL_EINVAL, "nil argument");
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  if (n == 0) return CEL_OK;
  DeviceGuard g(ctx->device);
  return place_samples_locked(ctx, static_cast<uint8_t*>(d_eds), present, k, row_roots, col_roots, n, rows, cols, axes,
                              shares, nodes, node_off, ok_out);
}

cel_status cel_repair_samples(cel_ctx* ctx, uint32_t k, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t n,
                              const uint32_t* rows, const uint32_t* cols, const uint8_t* axes, const uint8_t* shares,
                              const uint8_t* nodes, const uint64_t* node_off, uint8_t* ok_out, uint8_t* eds_out,
                              uint8_t* present_out, int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                              uint8_t* byz_present) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!eds_out || !present_out ||
      samples_nil(row_roots, col_roots, n, rows, cols, axes, shares, nodes, node_off, ok_out))
    return fail(ctx, CEL_EINVAL, "nil argument");
  cel_status st = validate_square(ctx, k, kShare);
  if (st) return st;
  DeviceGuard g(ctx->device);
  const size_t cells = (size_t)4 * k * k, eds_b = cells * kShare;
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  if (!d_eds) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  hipStream_t s = ctx->stream;
  if ((e = hipMemsetAsync(d_eds, 0, eds_b, s)) != hipSuccess) return hip_fail(ctx, e, "memset");
  std::memset(present_out, 0, cells);
  if (n && (st = place_samples_locked(ctx, d_eds, present_out, k, row_roots, col_roots, n, rows, cols, axes, shares,
                                      nodes, node_off, ok_out)) != CEL_OK)
    return st;
  st = dev_repair_locked(ctx, d_eds, present_out, k, row_roots, col_roots, bad_axis, bad_index, byz_shares,
                         byz_present);
  if (st != CEL_OK && st != CEL_EBYZANTINE && st != CEL_EBADROOT && st != CEL_EUNREPAIRABLE) return st;
  // as cel_repair: the (partially) repaired square goes back with the mask it is valid under
  if ((e = hipMemcpyAsync(eds_out, d_eds, eds_b, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return st;
}

}  // extern "C"
