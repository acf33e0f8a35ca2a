// C ABI of the bad-encoding fraud proofs (include/celestia_eds.h):
//   cel_befp_verify_batch  <- celestia-node share/eds/byzantine BadEncodingProof.Validate for a
//       batch of proofs: every entry's NMT proof, then the accused axis rebuilt from the
//       entries (Codec.Decode, Codec.Encode of the data half) and its root compared with the
//       accused root (specs/src/specs/fraud_proofs.md:3-13)
//   cel_dev_befp_build / cel_befp_build  <- NewBadEncodingProof's share collection: the known
//       cells of the axis a repair reported (CEL_EBYZANTINE), each with its single-leaf proof
//       in the orthogonal tree, where that tree is complete and matches the header
// The host decides what needs no device and lays out one upload (befp_plan.hpp); the chain
// verify -> place -> decode -> encode -> roots -> verdict runs on one stream with no host
// round trip (nmt_verify.hip, befp_kernels.hip, rs_*.hip, nmt_trees.hip), then one download.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "befp_kernels.hpp"
#include "befp_plan.hpp"
#include "cel_internal.hpp"
#include "nmt_verify.hpp"

using namespace cel;
using namespace cel::abi;

namespace {

constexpr uint64_t kMaxRecords = 1ull << 31;  // as the NMT verifier: record indices fit 32 bits with room

static_assert(befp::kNotFraud == CEL_BEFP_NOT_FRAUD && befp::kFraud == CEL_BEFP_FRAUD &&
                  befp::kBadShare == CEL_BEFP_BAD_SHARE && befp::kTooFew == CEL_BEFP_TOO_FEW &&
                  befp::kMalformed == CEL_BEFP_MALFORMED,
              "the planner's verdict bytes are the header's");

// The verifier's upload, laid out once for the device block (S_IN) and for the page-locked
// stage: shares, nodes, roots (one per entry, then one accused root per live proof), each
// entry's dense cell, each live proof's axis index, and last the NMT verifier's workspace, whose
// head (the proof table) is the end of the upload; its records lie behind.
struct VerifyUp {
  uint8_t *shares, *nodes, *roots;
  uint32_t* cell;
  int32_t* axis_idx;
  VerifyWork vw;
  size_t up_bytes, bytes;
};
VerifyUp carve_up(void* base, uint64_t ne, uint64_t nn, uint32_t live) {
  Carver c(base);
  VerifyUp u;
  u.shares = c.take<uint8_t>((size_t)ne * kShare);
  u.nodes = c.take<uint8_t>((size_t)nn * kNode);
  u.roots = c.take<uint8_t>((size_t)(ne + live) * kNode);
  u.cell = c.take<uint32_t>((size_t)ne * 4);
  u.axis_idx = c.take<int32_t>((size_t)live * 4);
  const size_t at = c.size();
  u.vw = verify_carve(base ? static_cast<uint8_t*>(base) + at : nullptr, ne, nn, (uint32_t)ne);
  u.up_bytes = at + u.vw.head_bytes;
  u.bytes = at + u.vw.bytes;
  return u;
}

// The device's answers, one download: verdicts, then the rebuilt roots.
struct VerifyDown {
  uint8_t *verdict, *rebuilt;
  size_t bytes;
};
VerifyDown carve_down(void* base, uint32_t live) {
  Carver c(base);
  VerifyDown d;
  d.verdict = c.take<uint8_t>(live);
  d.rebuilt = c.take<uint8_t>((size_t)live * kNode);
  d.bytes = c.size();
  return d;
}

// The producer's upload (the gathered axes' indices, the node records of every candidate's proof,
// the header roots to compare with) and download (root verdicts, packed proof nodes), each laid
// out once for the device block and for the page-locked stage.
struct BuildUp {
  int32_t *idx, *rec;
  uint8_t* want;
  size_t bytes;
};
BuildUp carve_build_up(void* base, uint32_t nc, uint32_t L) {
  Carver c(base);
  BuildUp u;
  u.idx = c.take<int32_t>((size_t)nc * 4);
  u.rec = c.take<int32_t>((size_t)nc * L * 4);
  u.want = c.take<uint8_t>((size_t)nc * kNode);
  u.bytes = c.size();
  return u;
}
struct BuildDown {
  uint8_t *ok, *nodes;
  size_t bytes;
};
BuildDown carve_build_down(void* base, uint32_t nc, uint32_t L) {
  Carver c(base);
  BuildDown d;
  d.ok = c.take<uint8_t>(nc);
  d.nodes = c.take<uint8_t>((size_t)nc * L * kNode);
  d.bytes = c.size();
  return d;
}

// The producer over the square resident at d_eds, ctx->mu held, arguments checked.
cel_status build_locked(cel_ctx* ctx, const uint8_t* d_eds, const uint8_t* present, uint32_t k,
                        const uint8_t* row_roots, const uint8_t* col_roots, uint32_t bad_axis, uint32_t bad_index,
                        uint32_t* positions_out, uint8_t* ent_axes_out, uint8_t* shares_out, uint8_t* nodes_out,
                        uint32_t* count_out) {
  const uint32_t W = 2 * k, L = befp::log2_width(W);
  *count_out = 0;
  const std::vector<uint32_t> pos = befp::select_positions(present, W, bad_axis, bad_index);
  const uint32_t nc = (uint32_t)pos.size();
  if (!nc) return CEL_OK;
  const int orth = bad_axis ? 0 : 1;  // the direction of the trees the entries are proved in
  const uint8_t* hdr = orth ? col_roots : row_roots;
  const size_t nodes_b = (size_t)L * kNode;
  // device: gathered axes | their trees | the lists and the header roots (uploaded) | outputs
  hipError_t e = hipSuccess;
  uint8_t* d_dense = static_cast<uint8_t*>(scratch(ctx, S_IN, (size_t)nc * W * kShare, &e));
  uint32_t* d_trees = static_cast<uint32_t*>(scratch(ctx, S_WORK, axes_trees_nodes(k, nc) * kNodeWords * 4, &e));
  const BuildUp up_size = carve_build_up(nullptr, nc, L);
  const BuildDown dn_size = carve_build_down(nullptr, nc, L);
  const size_t up_b = up_size.bytes, dn_b = dn_size.bytes, sh_b = (size_t)nc * kShare;
  uint8_t* d_up = static_cast<uint8_t*>(scratch(ctx, S_AUX, up_b, &e));
  uint8_t* d_dn = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, dn_b, &e));
  // every gathered axis is complete: launch_gather_axes reads its mask from a square of ones
  uint8_t* d_ones = static_cast<uint8_t*>(scratch(ctx, S_MASK, (size_t)W * W + (size_t)nc * W, &e));
  if (!d_dense || !d_trees || !d_up || !d_dn || !d_ones) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  // the page-locked stage: the upload, the download, then the shares (a strided copy of their own)
  uint8_t* hs = static_cast<uint8_t*>(host_stage(ctx, up_b + dn_b + sh_b));
  if (!hs) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  const BuildUp hup = carve_build_up(hs, nc, L), dup = carve_build_up(d_up, nc, L);
  const BuildDown hdn = carve_build_down(hs + up_b, nc, L), ddn = carve_build_down(d_dn, nc, L);
  uint8_t* h_shares = hs + up_b + dn_b;
  for (uint32_t a = 0; a < nc; a++) {
    hup.idx[a] = (int32_t)pos[a];
    befp::proof_records(W, nc, a, bad_index, hup.rec + (size_t)a * L);
    std::memcpy(hup.want + (size_t)a * kNode, hdr + (size_t)pos[a] * kNode, kNode);
  }
  hipStream_t s = ctx->stream;
  const Range range("befp.build");
  if ((e = hipMemcpyAsync(d_up, hs, up_b, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((e = hipMemsetAsync(d_ones, 1, (size_t)W * W, s)) != hipSuccess) return hip_fail(ctx, e, "memset");
  if ((e = launch_gather_axes(d_eds, d_ones, W, dup.idx, orth, nc, d_dense, d_ones + (size_t)W * W, s)) != hipSuccess)
    return hip_fail(ctx, e, "gather");
  if ((e = launch_axes_trees(d_dense, k, dup.idx, nc, d_trees, s)) != hipSuccess) return hip_fail(ctx, e, "axis trees");
  if ((e = launch_befp_roots_ok(d_trees, befp::root_record(W, nc, 0), dup.want, nc, ddn.ok, s)) != hipSuccess)
    return hip_fail(ctx, e, "root check");
  if ((e = launch_gather_nodes(d_trees, dup.rec, nc * L, ddn.nodes, s)) != hipSuccess) return hip_fail(ctx, e, "gather nodes");
  // the accused axis's cell of every gathered axis: leaf bad_index of each
  if ((e = hipMemcpyAsync(hs + up_b, d_dn, dn_b, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipMemcpy2DAsync(h_shares, kShare, d_dense + (size_t)bad_index * kShare, (size_t)W * kShare, kShare, nc,
                            hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  std::vector<uint32_t> p(pos);
  const uint32_t m = befp::compact_entries(hdn.ok, nc, p.data(), h_shares, kShare, hdn.nodes, nodes_b);
  std::memcpy(positions_out, p.data(), (size_t)m * 4);
  std::memset(ent_axes_out, orth, m);
  std::memcpy(shares_out, h_shares, (size_t)m * kShare);
  std::memcpy(nodes_out, hdn.nodes, (size_t)m * nodes_b);
  *count_out = m;
  return CEL_OK;
}

bool build_nil(const uint8_t* present, const uint8_t* row_roots, const uint8_t* col_roots, const uint32_t* positions_out,
               const uint8_t* ent_axes_out, const uint8_t* shares_out, const uint8_t* nodes_out,
               const uint32_t* count_out) {
  return !present || !row_roots || !col_roots || !positions_out || !ent_axes_out || !shares_out || !nodes_out ||
         !count_out;
}

}  // namespace

extern "C" {

cel_status cel_befp_verify_batch(cel_ctx* ctx, uint32_t n, uint32_t k, const uint8_t* axes, const uint32_t* index,
                                 const uint64_t* ent_off, const uint32_t* positions, const uint8_t* ent_axes,
                                 const uint8_t* shares, const uint8_t* nodes, const uint64_t* node_off,
                                 const uint8_t* row_roots, const uint8_t* col_roots, uint8_t* verdict_out,
                                 uint8_t* rebuilt_roots_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!befp::valid_width(k))
    return fail(ctx, CEL_EINVAL, "square width must be a power of 2 up to 512: got " + std::to_string(k));
  if (n == 0) return CEL_OK;
  if (!axes || !index || !ent_off || !row_roots || !col_roots || !verdict_out)
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (ent_off[n] > ent_off[0] && (!positions || !ent_axes || !shares || !nodes || !node_off))
    return fail(ctx, CEL_EINVAL, "nil argument");
  befp::VerifyPlan plan;
  if (!befp::plan_verify(n, k, axes, index, ent_off, positions, ent_axes, node_off, &plan))
    return fail(ctx, CEL_EINVAL, "entry and node offsets must be non-decreasing");
  std::memcpy(verdict_out, plan.verdict.data(), n);
  if (rebuilt_roots_out) std::memset(rebuilt_roots_out, 0, (size_t)n * kNode);
  const uint32_t live = (uint32_t)plan.live.size();
  if (!live) return CEL_OK;
  const uint32_t W = 2 * k;
  const uint64_t ne = plan.entries(), nn = plan.nodes();
  // every entry is one proof of the NMT verifier: its limits (api_verify.cpp: check_batch)
  if (ne + live >= kMaxRecords || nn + ne >= kMaxRecords)
    return fail(ctx, CEL_EINVAL, "too many entries or nodes for one device batch");

  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  const VerifyUp size = carve_up(nullptr, ne, nn, live);
  const VerifyDown dsize = carve_down(nullptr, live);
  const size_t dense_b = (size_t)live * W * kShare, flags_b = (size_t)live * W + live;
  uint8_t* d_up = static_cast<uint8_t*>(scratch(ctx, S_IN, size.bytes, &e));
  uint8_t* d_dense = static_cast<uint8_t*>(scratch(ctx, S_EDS, dense_b, &e));
  // presence [live][W], then the proofs' failed-entry flags [live] (zeroed together), then the
  // entries' verdicts
  uint8_t* d_dmask = static_cast<uint8_t*>(scratch(ctx, S_MASK, align256(flags_b) + (size_t)ne, &e));
  void* d_rwork = scratch(ctx, S_WORK, axes_roots_workspace_size(k, live), &e);
  // root records [live], then the download
  uint8_t* d_res = static_cast<uint8_t*>(scratch(ctx, S_ROOTS, align256((size_t)live * kNodeWords * 4) + dsize.bytes, &e));
  if (!d_up || !d_dense || !d_dmask || !d_rwork || !d_res) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  uint8_t* hs = static_cast<uint8_t*>(host_stage(ctx, size.up_bytes + dsize.bytes));
  if (!hs) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  const VerifyUp host = carve_up(hs, ne, nn, live), dev = carve_up(d_up, ne, nn, live);
  uint8_t* d_bad = d_dmask + (size_t)live * W;
  uint8_t* d_ok = d_dmask + align256(flags_b);
  uint32_t* d_rec = reinterpret_cast<uint32_t*>(d_res);
  const VerifyDown ddn = carve_down(d_res + align256((size_t)live * kNodeWords * 4), live);
  const VerifyDown hdn = carve_down(hs + size.up_bytes, live);

  // the table: packed entry t of live proof sl is NMT proof t, one leaf (share t) at the
  // entry's leaf of its tree, root t; the accused roots follow the entries' roots
  for (uint32_t sl = 0; sl < live; sl++) {
    const uint32_t i = plan.live[sl];
    const uint64_t e0 = ent_off[i], cnt = ent_off[i + 1] - e0, t0 = plan.ent0[sl];
    const uint8_t* rr = row_roots + (size_t)i * W * kNode;
    const uint8_t* cr = col_roots + (size_t)i * W * kNode;
    std::memcpy(host.shares + t0 * kShare, shares + e0 * kShare, cnt * kShare);
    std::memcpy(host.nodes + plan.node0[sl] * kNode, nodes + node_off[e0] * kNode,
                (plan.node0[sl + 1] - plan.node0[sl]) * kNode);
    std::memcpy(host.roots + (ne + sl) * kNode, (axes[i] ? cr : rr) + (size_t)index[i] * kNode, kNode);
    host.axis_idx[sl] = (int32_t)index[i];
    for (uint64_t j = 0; j < cnt; j++) {
      const uint64_t t = t0 + j, src = e0 + j;
      const befp::EntryAt at = befp::entry_at(k, axes[i], index[i], positions[src], ent_axes[src]);
      std::memcpy(host.roots + t * kNode, (at.root_axis ? cr : rr) + (size_t)at.root_index * kNode, kNode);
      host.cell[t] = sl * W + positions[src];
      VerifyProof& p = host.vw.proofs[t];
      p.start = (int32_t)at.leaf;
      p.end = p.start + 1;
      p.nleaves = 1;
      p.nnodes = (uint32_t)(node_off[src + 1] - node_off[src]);
      p.leaf0 = t;
      p.node0 = plan.node0[sl] + (node_off[src] - node_off[e0]);
      p.root = (uint32_t)t;
      p.pad = 0;
      uint8_t* ns = reinterpret_cast<uint8_t*>(host.vw.ns) + (size_t)t * 32;
      if (at.q0) std::memcpy(ns, shares + src * kShare, kNs);
      else std::memset(ns, 0xFF, kNs);
      ns[29] = ns[30] = ns[31] = 0;
      host.vw.leaf_proof[t] = (uint32_t)t;
    }
  }
  const Range range("befp.verify");
  if ((e = hipMemcpyAsync(d_up, hs, size.up_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(ctx, e, "H2D");
  if ((e = hipMemsetAsync(d_dmask, 0, flags_b, s)) != hipSuccess) return hip_fail(ctx, e, "memset");
  if ((e = launch_verify(dev.vw, dev.shares, ne, dev.nodes, nn, dev.roots, (uint32_t)ne, d_ok, kVerifyAll, s)) != hipSuccess)
    return hip_fail(ctx, e, "nmt verify");
  if ((e = launch_befp_place(dev.shares, dev.cell, d_ok, ne, W, d_dense, d_dmask, d_bad, s)) != hipSuccess)
    return hip_fail(ctx, e, "place");
  if ((e = launch_rs_decode(d_dense, d_dmask, live, k, kShare, ctx->tables, s)) != hipSuccess)
    return hip_fail(ctx, e, "decode");
  // the parity half of every axis <- Encode(its data half), in place
  RsGeom gm{};
  gm.in = d_dense;
  gm.out = d_dense + (size_t)k * kShare;
  gm.in_axis = gm.out_axis = (uint64_t)W * kShare;
  gm.in_sq = gm.out_sq = dense_b;
  gm.in_shard = gm.out_shard = kShare;
  gm.n = k;
  gm.len = kShare;
  gm.axes = live;
  gm.nsq = 1;
  if ((e = launch_rs_encode(gm, ctx->tables, s)) != hipSuccess) return hip_fail(ctx, e, "encode");
  if ((e = launch_axes_roots(d_dense, k, dev.axis_idx, live, d_rec, d_rwork, s)) != hipSuccess)
    return hip_fail(ctx, e, "roots");
  if ((e = launch_befp_verdict(d_bad, d_rec, dev.roots + ne * kNode, live, ddn.verdict, ddn.rebuilt, s)) != hipSuccess)
    return hip_fail(ctx, e, "verdict");
  if ((e = hipMemcpyAsync(hs + size.up_bytes, ddn.verdict, dsize.bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  for (uint32_t sl = 0; sl < live; sl++) {
    verdict_out[plan.live[sl]] = hdn.verdict[sl];
    if (rebuilt_roots_out)
      std::memcpy(rebuilt_roots_out + (size_t)plan.live[sl] * kNode, hdn.rebuilt + (size_t)sl * kNode, kNode);
  }
  return CEL_OK;
}

cel_status cel_dev_befp_build(cel_ctx* ctx, const void* d_eds, const uint8_t* present, uint32_t k,
                              const uint8_t* row_roots, const uint8_t* col_roots, uint32_t bad_axis,
                              uint32_t bad_index, uint32_t* positions_out, uint8_t* ent_axes_out,
                              uint8_t* shares_out, uint8_t* nodes_out, uint32_t* count_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!d_eds || build_nil(present, row_roots, col_roots, positions_out, ent_axes_out, shares_out, nodes_out, count_out))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (!befp::valid_width(k))
    return fail(ctx, CEL_EINVAL, "square width must be a power of 2 up to 512: got " + std::to_string(k));
  if (bad_axis > 1 || bad_index >= 2 * k) return fail(ctx, CEL_EINVAL, "accused axis outside the square");
  if (reinterpret_cast<uintptr_t>(d_eds) & 15) return fail(ctx, CEL_EINVAL, "d_eds must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return build_locked(ctx, static_cast<const uint8_t*>(d_eds), present, k, row_roots, col_roots, bad_axis, bad_index,
                      positions_out, ent_axes_out, shares_out, nodes_out, count_out);
}

cel_status cel_befp_build(cel_ctx* ctx, const uint8_t* eds, const uint8_t* present, uint32_t k,
                          const uint8_t* row_roots, const uint8_t* col_roots, uint32_t bad_axis, uint32_t bad_index,
                          uint32_t* positions_out, uint8_t* ent_axes_out, uint8_t* shares_out, uint8_t* nodes_out,
                          uint32_t* count_out) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!eds || build_nil(present, row_roots, col_roots, positions_out, ent_axes_out, shares_out, nodes_out, count_out))
    return fail(ctx, CEL_EINVAL, "nil argument");
  if (!befp::valid_width(k))
    return fail(ctx, CEL_EINVAL, "square width must be a power of 2 up to 512: got " + std::to_string(k));
  if (bad_axis > 1 || bad_index >= 2 * k) return fail(ctx, CEL_EINVAL, "accused axis outside the square");
  DeviceGuard g(ctx->device);
  const size_t eds_b = (size_t)4 * k * k * kShare;
  hipError_t e = hipSuccess;
  uint8_t* d_eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, eds_b, &e));
  if (!d_eds) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  if ((e = hipMemcpyAsync(d_eds, eds, eds_b, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  return build_locked(ctx, d_eds, present, k, row_roots, col_roots, bad_axis, bad_index, positions_out, ent_axes_out,
                      shares_out, nodes_out, count_out);
}

}  // extern "C"
