// C ABI of the repair (include/celestia_eds.h): cel_repair, cel_dev_repair, their batch forms
// (cel_dev_repair_batch, cel_repair_batch) and their test hooks, split from api.cpp. Device control of rsmt2d's Repair over a device-resident
// EDS: the buffers, the two streams and what is enqueued on them. What to solve and check,
// and in which order, is the host planner's (repair_plan.hpp); every decode, re-encode,
// compare and root runs in the HIP kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "cel_internal.hpp"
#include "repair_plan.hpp"

using namespace cel;
using namespace cel::abi;
using namespace cel::repair;

extern "C" {

// ------------------------------------------------------------------- repair

// rsmt2d v0.14.0 ExtendedDataSquare.Repair [dep] (extendeddatacrossword.go), with the
// oracle's restatement (oracle/eds.c) as the checker. The crossword control loop runs on
// the host over the presence mask; decoding, re-encoding, byte comparisons and root
// computation run on the device over the EDS kept resident.
namespace {

// Axis lists of the passes of one repair: each pass gets its own slot of a page-locked
// host buffer and of the device index buffer, so its upload is asynchronous and no pass
// waits for the previous one's kernels (a pageable upload into one shared buffer
// serialised the host against the stream). Slots wrap with one stream sync.
constexpr uint32_t kIdxSlots = 64;

struct RepairBufs {
  uint32_t W;
  uint8_t* eds;
  uint8_t* mask;
  int32_t* list0;     // the first pass's axis list, right after the mask (one upload for both)
  uint8_t* dense[2];  // gathered axes of the solve passes, alternating (main stream)
  uint8_t* dmask;
  uint8_t* dchk;      // gathered axes of the check passes (side stream)
  uint8_t* dmask_chk;
  uint8_t* tmp;       // re-encoded parity halves (side stream)
  uint8_t* work;      // NMT workspace of the final verification, or repair_exact's axes roots
  uint32_t* rec;      // [2][W][kNodeWords] repair_exact's root records, in the same slot
  uint8_t* roots;     // [2][W][90] row then column roots of the final verification, then flags
  int32_t* flags;     // [2][W] encoding-check flags by (direction, axis), right after the roots
  uint8_t* hroots;    // page-locked copy of roots + flags (one D2H of res_bytes at the end)
  int32_t* hflags;
  size_t res_bytes;
  int32_t* idx;       // [kIdxSlots][W] device axis lists
  int32_t* hidx;      // [kIdxSlots][W] page-locked staging of the same
  uint8_t* hmask;     // [W][W] page-locked staging of the presence mask, then of the first list
  int32_t* hlist0;
  uint32_t slot;      // next free slot
  uint32_t solves;    // solve passes so far (which dense buffer is next)
  // Two streams: the solve chain (gather -> decode -> scatter) runs on `main`; every
  // re-encode check (of the solved axes, the sanity and the orthogonal checks) runs on
  // `side`, off the chain's critical path: its outcome is only read at the end.
  hipStream_t main, side;
  hipEvent_t ev_main;     // the square after the main stream's latest pass
  hipEvent_t ev_side[2];  // the side stream is done with dense[i]
  hipEvent_t ev_done;     // the side stream's last check
};

// The layout of each scratch slot and of the page-locked stage, one walk per buffer (b.W
// set). carved() runs a walk: on a null base it gives the size to allocate, on the
// allocation the pointers into it.
static void carve_in(Carver& c, RepairBufs& b) {  // S_IN
  for (uint8_t** p : {&b.dense[0], &b.dense[1], &b.dchk}) *p = c.take<uint8_t>((size_t)b.W * b.W * kShare);
}
static void carve_aux(Carver& c, RepairBufs& b) {  // S_AUX
  b.tmp = c.take<uint8_t>((size_t)b.W * b.W * kShare / 2);
  b.idx = c.take<int32_t>((size_t)kIdxSlots * b.W * 4);
}
// The presence mask, then the first pass's axis list directly after it: one upload carries
// both, so the device buffer and the stage take them by the same walk.
static void take_mask_list(Carver& c, uint32_t W, uint8_t** mask, int32_t** list0) {
  *mask = c.take<uint8_t>((size_t)W * W);
  *list0 = c.take<int32_t>((size_t)W * 4);
}
static void carve_mask(Carver& c, RepairBufs& b) {  // S_MASK
  take_mask_list(c, b.W, &b.mask, &b.list0);
  for (uint8_t** p : {&b.dmask, &b.dmask_chk}) *p = c.take<uint8_t>((size_t)b.W * b.W);
}
// Every root of the square, then the flags directly after them: one download (res_bytes,
// from the first root to the last flag) brings both back, into the same walk of the stage.
static void take_results(Carver& c, uint32_t W, uint8_t** roots, int32_t** flags) {
  *roots = c.take<uint8_t>(2 * (size_t)W * kNode);
  *flags = c.take<int32_t>(2 * (size_t)W * 4);
}
static void carve_roots(Carver& c, RepairBufs& b) { take_results(c, b.W, &b.roots, &b.flags); }  // S_ROOTS
// repair_exact's axes-roots workspace of one direction's 2k axes, then, after it, the root
// records of both directions; the whole-square commit's workspace lies over the two.
static void carve_work(Carver& c, RepairBufs& b) {  // S_WORK
  b.work = c.take<uint8_t>(axes_roots_workspace_size(b.W / 2, b.W));
  b.rec = c.take<uint32_t>(2 * (size_t)b.W * kNodeWords * 4);
  c.overlay(nmt_workspace_size(b.W / 2, 1));
}
static void carve_stage(Carver& c, RepairBufs& b) {  // the page-locked stage
  b.hidx = c.take<int32_t>((size_t)kIdxSlots * b.W * 4);
  take_mask_list(c, b.W, &b.hmask, &b.hlist0);  // hmask followed by its list
  take_results(c, b.W, &b.hroots, &b.hflags);
}
static size_t carved(void (*walk)(Carver&, RepairBufs&), void* base, RepairBufs& b) {
  Carver c(base);
  walk(c, b);
  return c.size();
}

// `list` into the next axis-list slot, uploaded on stream s. Every slot in flight: drain
// both streams (the side stream's compares read the lists too), then reuse.
static cel_status upload_list(cel_ctx* ctx, RepairBufs& b, const std::vector<int32_t>& list, hipStream_t s,
                              int32_t** d_list) {
  hipError_t e;
  if (b.slot == kIdxSlots) {
    if ((e = hipStreamSynchronize(b.main)) != hipSuccess || (e = hipStreamSynchronize(b.side)) != hipSuccess)
      return hip_fail(ctx, e, "sync");
    b.slot = 0;
  }
  int32_t* hidx = b.hidx + (size_t)b.slot * b.W;
  *d_list = b.idx + (size_t)b.slot * b.W;
  b.slot++;
  std::memcpy(hidx, list.data(), list.size() * 4);
  if ((e = hipMemcpyAsync(*d_list, hidx, list.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  return CEL_OK;
}

// Randomised idle time in front of an enqueue point (cel_debug_schedule_fuzz; off = 0).
static cel_status fuzz(cel_ctx* ctx, hipStream_t s) {
  if (!ctx->fuzz_max_us) return CEL_OK;
  uint64_t x = (ctx->fuzz_state += 0x9E3779B97F4A7C15ull);  // splitmix64
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  const hipError_t e = launch_delay((uint32_t)(x % (ctx->fuzz_max_us + 1ull)), s);
  return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "delay");
}

// Re-encode check of na gathered axes at `dense` on stream s: the data half of each axis
// is encoded again and compared with its parity half; mismatches set flags[is_col*W + axis].
// k = 256, 512: one launch of the GF(2^16) register kernel in check mode; else encode into
// b.tmp and k_cmp.
static cel_status encode_check(cel_ctx* ctx, RepairBufs& b, uint32_t k, int is_col, uint32_t na, const uint8_t* dense,
                               const int32_t* idx, hipStream_t s) {
  const uint64_t axis_b = (uint64_t)2 * k * kShare, half_b = (uint64_t)k * kShare;
  const bool fused = k == 256 || k == 512;  // GF(2^16): the register kernel compares with the parity half as it goes
  int32_t* flags = b.flags + (size_t)is_col * 2 * k;
  RsGeom g{};
  g.in = dense;
  g.in_axis = axis_b;
  g.out = fused ? const_cast<uint8_t*>(dense) + half_b : b.tmp;
  g.out_axis = fused ? axis_b : half_b;
  g.in_sq = na * g.in_axis;
  g.out_sq = na * g.out_axis;
  g.in_shard = g.out_shard = kShare;
  g.n = k;
  g.len = kShare;
  g.axes = na;
  g.nsq = 1;
  g.chk_flags = fused ? flags : nullptr;
  g.chk_idx = fused ? idx : nullptr;
  hipError_t e;
  if ((e = launch_rs_encode(g, ctx->tables, s)) != hipSuccess)
    return hip_fail(ctx, e, fused ? "encoding check" : "re-encode");
  if (!fused && (e = launch_cmp(b.tmp, half_b, dense + half_b, axis_b, half_b, na, flags, s, idx)) != hipSuccess)
    return hip_fail(ctx, e, "compare");
  return CEL_OK;
}

// Encoding check of na complete axes of the square (list idx on the device) on stream s:
// one in-place launch for k = 32..128 (k_rs_check_axes) and k = 256/512 (k_rs_gf16x in
// check mode), else gather into dchk and encode_check.
static cel_status check_in_square(cel_ctx* ctx, RepairBufs& b, uint32_t k, int is_col, uint32_t na,
                                  const int32_t* idx, hipStream_t s) {
  const uint32_t W = 2 * k;
  hipError_t e;
  if (k >= 32 && k <= kMaxGf8Width) {
    if ((e = launch_rs_check_axes(b.eds, k, idx, is_col, na, b.flags + (size_t)is_col * W, s)) != hipSuccess)
      return hip_fail(ctx, e, "encoding check");
    return CEL_OK;
  }
  if (k == 256 || k == 512) {  // the GF(2^16) register kernel in check mode, in place
    RsGeom g = square_axis_geom(b.eds, k, is_col, na, 1);
    g.chk_flags = b.flags + (size_t)is_col * W;
    g.chk_idx = idx;
    g.chk_axes = idx;
    if ((e = launch_rs_encode(g, ctx->tables, s)) != hipSuccess) return hip_fail(ctx, e, "encoding check");
    return CEL_OK;
  }
  if ((e = launch_gather_axes(b.eds, b.mask, W, idx, is_col, na, b.dchk, b.dmask_chk, s)) != hipSuccess)
    return hip_fail(ctx, e, "gather");
  return encode_check(ctx, b, k, is_col, na, b.dchk, idx, s);
}

// Decode of na listed axes (rows, columns, or with is_col < 0 every entry's direction in
// bit 30: the register decoder only) on stream s. W = 32 .. 256: the register decoder in
// place, erased cells straight into the square (no gather / scatter on the chain); else
// gather -> decode -> scatter through `dense`.
static hipError_t decode_axes(cel_ctx* ctx, RepairBufs& b, uint32_t k, const int32_t* idx, int is_col, uint32_t na,
                              uint8_t* dense, hipStream_t s) {
  const uint32_t W = 2 * k;
  if (rs_decode_axis_supported(W, kShare))
    return launch_rs_decode_in_square(b.eds, b.mask, W, idx, is_col, na, ctx->tables.mul8, s);
  hipError_t e;
  if ((e = launch_gather_axes(b.eds, b.mask, W, idx, is_col, na, dense, b.dmask, s)) != hipSuccess ||
      (e = launch_rs_decode(dense, b.dmask, na, k, kShare, ctx->tables, s)) != hipSuccess)
    return e;
  return launch_scatter_axes(b.eds, b.mask, W, idx, is_col, na, dense, s);
}

// rsmt2d solveCrossword's decode of `list` (incomplete axes of one direction), in two
// halves so the host can put other side-stream work between them:
//   solve_issue  the decode on the main stream (in place in the square, or gather ->
//                decode -> scatter), then ev_main;
//   solve_check  the encoding check of the solved axes on the side stream, after ev_main.
// Nothing is synchronised: every flag is read back once at the end of the repair.
struct Issued {
  uint32_t na = 0;
  uint32_t d = 0;
  int32_t* idx = nullptr;
};

static cel_status solve_issue(cel_ctx* ctx, RepairBufs& b, uint32_t k, int is_col, const std::vector<int32_t>& list,
                              Issued* out, int32_t* uploaded = nullptr) {
  const Range range("repair.solve");
  const uint32_t W = 2 * k, na = (uint32_t)list.size();
  out->na = na;
  if (!na) return CEL_OK;
  const uint32_t d = out->d = b.solves++ & 1u;
  cel_status st;
  if (uploaded) out->idx = uploaded;  // `list` is already on the device there
  else if ((st = upload_list(ctx, b, list, b.main, &out->idx)) != CEL_OK) return st;
  if ((st = fuzz(ctx, b.main)) != CEL_OK) return st;
  hipError_t e = hipSuccess;
  // dense path: the side stream is done with dense[d]
  if (!rs_decode_axis_supported(W, kShare)) e = hipStreamWaitEvent(b.main, b.ev_side[d], 0);
  if (e != hipSuccess || (e = decode_axes(ctx, b, k, out->idx, is_col, na, b.dense[d], b.main)) != hipSuccess ||
      (e = hipEventRecord(b.ev_main, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "solve");
  return CEL_OK;
}

// The side half of a solve_issue, enqueued after it with ev_main that solve's record or a
// later one of the main stream (the axes it checks are final from their pass on). Dense
// path: it must be enqueued before the solve after next, which reuses dense[s.d] once
// this check has recorded ev_side[s.d].
static cel_status solve_check(cel_ctx* ctx, RepairBufs& b, uint32_t k, int is_col, const Issued& s) {
  if (!s.na) return CEL_OK;
  const uint32_t W = 2 * k;
  hipError_t e;
  if ((e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess) return hip_fail(ctx, e, "event");
  cel_status st;
  if ((st = fuzz(ctx, b.side)) != CEL_OK) return st;
  if (rs_decode_axis_supported(W, kShare))  // the completed axes are checked in the square
    return check_in_square(ctx, b, k, is_col, s.na, s.idx, b.side);
  if ((st = encode_check(ctx, b, k, is_col, s.na, b.dense[s.d], s.idx, b.side)) != CEL_OK) return st;
  if ((e = hipEventRecord(b.ev_side[s.d], b.side)) != hipSuccess) return hip_fail(ctx, e, "event");
  return CEL_OK;
}

// Encoding check of complete axes (preRepairSanityCheck, and the orthogonal axes a solve
// completed) on the side stream. wait_main: after the main stream's latest work; without
// it the caller guarantees the axes are final in the side stream's order already (the
// orthogonal axes of a pass whose solve_check the side stream has passed).
static cel_status check_pass(cel_ctx* ctx, RepairBufs& b, uint32_t k, int is_col, const std::vector<int32_t>& list,
                             bool wait_main) {
  const Range range("repair.check");
  const uint32_t na = (uint32_t)list.size();
  if (!na) return CEL_OK;
  hipError_t e;
  if (wait_main &&
      ((e = hipEventRecord(b.ev_main, b.main)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess))
    return hip_fail(ctx, e, "event");
  int32_t* idx;
  cel_status st;
  if ((st = upload_list(ctx, b, list, b.side, &idx)) != CEL_OK || (st = fuzz(ctx, b.side)) != CEL_OK) return st;
  return check_in_square(ctx, b, k, is_col, na, idx, b.side);
}

struct RepairOut {
  int32_t* bad_axis;
  int32_t* bad_index;
  uint8_t* byz_shares;   // nullable, W * 512
  uint8_t* byz_present;  // nullable, W
};

// Report a failing axis: status, axis, index, and for CEL_EBYZANTINE rsmt2d's
// ErrByzantineData.Shares: the axis's cells from the square (complete axes never change;
// cells of a solved axis present before its solve kept their bytes), with the axis's mask
// from hm (masked: hm is rolled back to the mask before the failing solve) or all present.
static cel_status fail_axis(cel_ctx* ctx, const RepairBufs& b, const std::vector<uint8_t>& hm, const RepairOut& out,
                            cel_status code, int is_col, int32_t idx, bool masked) {
  const uint32_t W = b.W;
  if (out.bad_axis) *out.bad_axis = is_col;
  if (out.bad_index) *out.bad_index = idx;
  if (code == CEL_EBYZANTINE && (out.byz_shares || out.byz_present)) {
    std::vector<uint8_t> axis((size_t)W * kShare);
    const uint8_t* src = b.eds + (is_col ? (size_t)idx * kShare : (size_t)idx * W * kShare);
    const hipError_t ce = is_col ? hipMemcpy2D(axis.data(), kShare, src, (size_t)W * kShare, kShare, W,
                                                hipMemcpyDeviceToHost)
                                 : hipMemcpy(axis.data(), src, axis.size(), hipMemcpyDeviceToHost);
    if (ce != hipSuccess) return hip_fail(ctx, ce, "byzantine shares");
    for (uint32_t j = 0; j < W; j++) {
      const uint8_t p = masked ? hm[is_col ? (size_t)j * W + (uint32_t)idx : (size_t)idx * W + j] : 1;
      if (out.byz_present) out.byz_present[j] = p;
      if (out.byz_shares) {
        if (p) std::memcpy(out.byz_shares + (size_t)j * kShare, axis.data() + (size_t)j * kShare, kShare);
        else std::memset(out.byz_shares + (size_t)j * kShare, 0, kShare);
      }
    }
  }
  const char* dir = is_col ? "col" : "row";
  return fail(ctx, code, code == CEL_EBADROOT
                             ? std::string("bad root input: ") + dir + " " + std::to_string(idx)
                             : std::string("byzantine ") + (is_col ? "column" : "row") + " " + std::to_string(idx));
}

// Commit every root of the square on the main stream beside the side stream's last checks,
// join the streams and read roots and flags back (one page-locked copy: b.hroots, b.hflags).
static cel_status verify_square(cel_ctx* ctx, RepairBufs& b, uint32_t k, int last_col, const Issued& last,
                                int pending_col, const std::vector<int32_t>& pending) {
  const size_t roots_b = (size_t)b.W * kNode;
  hipError_t e;
  cel_status st;
  if ((st = fuzz(ctx, b.main)) != CEL_OK) return st;
  // the last pass's checks go to the side stream ahead of the commit's dozen launches, so
  // they run beside its leaf hashing instead of trailing its tree levels
  if ((st = solve_check(ctx, b, k, last_col, last)) != CEL_OK ||
      (st = check_pass(ctx, b, k, pending_col, pending, false)) != CEL_OK)
    return st;
  if ((e = launch_commit(b.eds, k, 1, b.roots, b.roots + roots_b, nullptr, nullptr, b.work, false, b.main)) !=
      hipSuccess)
    return hip_fail(ctx, e, "roots");
  if ((e = hipEventRecord(b.ev_done, b.side)) != hipSuccess || (e = hipStreamWaitEvent(b.main, b.ev_done, 0)) != hipSuccess)
    return hip_fail(ctx, e, "join");
  if ((e = hipMemcpyAsync(b.hroots, b.roots, b.res_bytes, hipMemcpyDeviceToHost, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(b.main)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
}

// rsmt2d's own solve order, for a square the pass-parallel schedule found byzantine.
//
// solveCrossword sweeps `for i { solveCrosswordRow(i); solveCrosswordCol(i) }`, and on
// inconsistent data which axis fails first, and with which Shares, depends on that order.
// The host replays the sweeps over the mask alone (plan_sweeps): the solve sequence, the
// orthogonal axes each solve completes, and each solve's level. Solves of one level touch
// no cell another of them fills, so a level runs as one row and one column launch; level
// by level the device sees every axis exactly as rsmt2d's sequence does. hm: the mask the
// repair started from; cells present in it still hold their bytes (every decoder stores
// erased cells only). Every check gathers its axes into dchk first, also where an in-place
// check exists: the root kernel wants them dense anyway.
static cel_status repair_exact(cel_ctx* ctx, RepairBufs& b, std::vector<uint8_t>& hm, uint32_t k,
                               const uint8_t* row_roots, const uint8_t* col_roots, const RepairOut& out) {
  const Range range("repair.exact");
  const uint32_t W = 2 * k;
  const size_t cells = (size_t)W * W;
  const SweepPlan plan = plan_sweeps(hm, k);
  const std::vector<Solve>& solves = plan.solves;
  const std::vector<int32_t>& level = plan.level;
  const std::vector<Check>& order = plan.order;
  const size_t S = solves.size();
  // order[first[t] .. first[t + 1]) = solve t's checks (SOLVE, then its ORTH axes)
  std::vector<size_t> first(S + 1, order.size());
  for (size_t o = 0; o < order.size(); o++)
    if (order[o].kind == Check::SOLVE) first[(size_t)order[o].solve] = o;
  const bool in_square = rs_decode_axis_supported(W, kShare);
  // roots of the checked axes: 96-byte records, each direction's in the order of its list
  const uint8_t* const exp[2] = {row_roots, col_roots};
  std::vector<uint8_t> h_rec((size_t)2 * W * kNodeWords * 4);
  std::vector<int32_t> h_flags((size_t)2 * W);
  hipError_t e;
  cel_status st;
  // both streams are idle (verify_square synchronised the joined streams); the square keeps
  // the bytes of every cell known at the start (decoders store erased cells only)
  std::memcpy(b.hmask, hm.data(), cells);
  if ((e = hipMemcpyAsync(b.mask, b.hmask, cells, hipMemcpyHostToDevice, b.main)) != hipSuccess ||
      (e = hipMemsetAsync(b.flags, 0, 2 * (size_t)W * 4, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  // The sequence runs in prefixes of CH solves. A prefix's solves depend only on earlier
  // solves, so each prefix runs level by level after the previous one; then its checks
  // (encoding and root of every axis it solves or completes) come back, and the first
  // failure in sweep order ends the replay there: rsmt2d returns at its first failing check.
  const size_t CH = std::max<size_t>(16, W / 4);
  for (size_t s0 = 0; s0 < S; s0 += CH) {
    const size_t s1 = std::min(S, s0 + CH);
    std::vector<int32_t> lists;
    struct Group {
      uint32_t off, n;
      int is_col;  // -1: mixed (register decoder, direction in bit 30)
    };
    std::vector<Group> groups;
    {
      int32_t lo = INT32_MAX, hi = 0;
      for (size_t t = s0; t < s1; t++) {
        lo = std::min(lo, level[t]);
        hi = std::max(hi, level[t]);
      }
      std::vector<std::vector<int32_t>> by[2];
      by[0].resize((size_t)(hi - lo + 1));
      by[1].resize((size_t)(hi - lo + 1));
      for (size_t t = s0; t < s1; t++) by[solves[t].is_col][(size_t)(level[t] - lo)].push_back(solves[t].idx);
      for (size_t L = 0; L < by[0].size(); L++) {
        if (in_square) {
          const uint32_t off = (uint32_t)lists.size();
          for (int d = 0; d < 2; d++)
            for (int32_t i : by[d][L]) lists.push_back(d ? (int32_t)((uint32_t)i | (1u << 30)) : i);
          if ((uint32_t)lists.size() > off) groups.push_back({off, (uint32_t)lists.size() - off, -1});
          continue;
        }
        for (int d = 0; d < 2; d++)
          if (!by[d][L].empty()) {
            groups.push_back({(uint32_t)lists.size(), (uint32_t)by[d][L].size(), d});
            lists.insert(lists.end(), by[d][L].begin(), by[d][L].end());
          }
      }
    }
    // the axes this prefix's checks look at, by direction (each axis is checked once)
    std::vector<int32_t> chk[2];
    for (size_t o = first[s0]; o < first[s1]; o++) chk[order[o].is_col].push_back(order[o].idx);
    const uint32_t off_chk0 = (uint32_t)lists.size();
    lists.insert(lists.end(), chk[0].begin(), chk[0].end());
    const uint32_t off_chk1 = (uint32_t)lists.size();
    lists.insert(lists.end(), chk[1].begin(), chk[1].end());
    std::memcpy(b.hidx, lists.data(), lists.size() * 4);
    if ((e = hipMemcpyAsync(b.idx, b.hidx, lists.size() * 4, hipMemcpyHostToDevice, b.main)) != hipSuccess)
      return hip_fail(ctx, e, "H2D");
    for (const Group& g : groups) {
      const int32_t* idx = b.idx + g.off;
      if ((st = fuzz(ctx, b.main)) != CEL_OK) return st;
      if ((e = decode_axes(ctx, b, k, idx, g.is_col, g.n, b.dense[0], b.main)) != hipSuccess)
        return hip_fail(ctx, e, "solve");
    }
    // encoding check and root of every checked axis, one direction at a time through dchk
    for (int d = 0; d < 2; d++) {
      const uint32_t na = (uint32_t)chk[d].size();
      if (!na) continue;
      const int32_t* idx = b.idx + (d ? off_chk1 : off_chk0);
      uint32_t* rec = b.rec + (size_t)d * W * kNodeWords;
      if ((e = launch_gather_axes(b.eds, b.mask, W, idx, d, na, b.dchk, b.dmask_chk, b.main)) != hipSuccess)
        return hip_fail(ctx, e, "gather");
      if ((st = encode_check(ctx, b, k, d, na, b.dchk, idx, b.main)) != CEL_OK) return st;
      if ((e = launch_axes_roots(b.dchk, k, idx, na, rec, b.work, b.main)) != hipSuccess)
        return hip_fail(ctx, e, "roots");
    }
    if ((e = hipMemcpyAsync(h_flags.data(), b.flags, h_flags.size() * 4, hipMemcpyDeviceToHost, b.main)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(h_rec.data(), b.rec, h_rec.size(), hipMemcpyDeviceToHost, b.main)) != hipSuccess ||
        (e = hipStreamSynchronize(b.main)) != hipSuccess)
      return hip_fail(ctx, e, "D2H");
    // replay the prefix's checks in sweep order
    cel_status code;
    const long f = first_failure(order.data() + first[s0], first[s1] - first[s0],
                                 {h_rec.data(), kNodeWords * 4, RootRecords::BY_RANK}, exp, h_flags.data(), W, &code);
    if (f >= 0) {  // no SANITY check in a sweep plan: code is CEL_EBYZANTINE
      const Check& c = order[first[s0] + (size_t)f];
      rollback(hm, W, solves, (size_t)c.solve);
      return fail_axis(ctx, b, hm, out, code, c.is_col, c.idx, c.kind == Check::SOLVE);
    }
  }
  // not reached for a square the pass schedule found byzantine (the outcome does not depend
  // on the order when every check passes), kept for completeness
  if (!plan.solved) {
    rollback(hm, W, solves, S);
    return fail(ctx, CEL_EUNREPAIRABLE, "failed to solve data square");
  }
  std::fill(hm.begin(), hm.end(), (uint8_t)1);
  return CEL_OK;
}

// rsmt2d Repair over the EDS resident at b.eds. hm = host presence mask (updated: all
// ones on success, the mask before the failing solve on a byzantine / bad-root error,
// the mask after the last solve when stuck). No pass waits for the device. Root checks
// are deferred: an axis, once complete, never changes, so one commit pass over the final
// square gives every root rsmt2d checks on the way, and the checks are replayed in
// rsmt2d's order, reporting the first failure.
//
// The solves run in passes (every solvable row, then every solvable column, ...), which
// decodes whole directions at once. When every check passes, the outcome equals that of
// rsmt2d's sweep order (row i, then column i): all cells of the final square then agree
// with valid codewords whose roots match, so any order decodes the same bytes and passes
// the same checks, and the set of axes that can be solved is the same closure. Only a
// failing solve or orthogonal check depends on the order; that square is replayed in
// rsmt2d's order by repair_exact.
static cel_status repair_core(cel_ctx* ctx, RepairBufs& b, std::vector<uint8_t>& hm, uint32_t k,
                              const uint8_t* row_roots, const uint8_t* col_roots, const RepairOut& out) {
  const uint32_t W = 2 * k;
  const size_t cells = (size_t)W * W;
  hipStream_t s = b.main;
  hipError_t e = hipSuccess;
  cel_status st;
  // an early return leaves no side-stream work running on the ctx's scratch buffers
  struct SideDrain {
    hipStream_t side;
    ~SideDrain() { (void)hipStreamSynchronize(side); }
  } drain{b.side};
  // The first row pass goes to the device before the host builds its bookkeeping (the
  // mask bitsets, the sanity lists), which then runs beside the decode; its axis list
  // rides in the mask's upload.
  std::vector<int32_t> list, orth;
  const std::vector<int32_t> first = first_row_pass(hm, k);
  std::memcpy(b.hmask, hm.data(), cells);
  if (!first.empty()) std::memcpy(b.hlist0, first.data(), first.size() * 4);
  const size_t up_b = (size_t)(reinterpret_cast<uint8_t*>(b.hlist0) - b.hmask) + first.size() * 4;
  // the flags are the side stream's (its checks), zeroed there after the mask is up
  if ((e = hipMemcpyAsync(b.mask, b.hmask, up_b, hipMemcpyHostToDevice, s)) != hipSuccess ||
      (e = hipEventRecord(b.ev_main, s)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess ||
      (e = hipMemsetAsync(b.flags, 0, 2 * (size_t)W * 4, b.side)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  // Each pass's encoding check (side stream) is enqueued after the next pass's decode, so
  // the host's enqueue of it is off the solve chain (the checked axes are final from their
  // pass on; the dense path's buffer dense[d] is reused two passes later, after the check
  // has recorded ev_side[d]).
  Issued prev;
  int prev_col = 0;
  if ((st = solve_issue(ctx, b, k, 0, first, &prev, b.list0)) != CEL_OK) return st;
  bool first_issued = !first.empty();
  std::unique_ptr<Range> plan_range(new Range("repair.plan"));
  MaskBits mb(hm, W);
  std::vector<Check> order;
  std::vector<Solve> solves;
  // preRepairSanityCheck: for i: row i, column i
  {
    std::vector<int32_t> comp[2];
    for (uint32_t i = 0; i < W; i++)
      for (int is_col = 0; is_col < 2; is_col++)
        if (mb.cnt[is_col][i] == W) {
          order.push_back({Check::SANITY, is_col, (int32_t)i, -1});
          comp[is_col].push_back((int32_t)i);
        }
    for (int is_col = 0; is_col < 2; is_col++)
      if ((st = check_pass(ctx, b, k, is_col, comp[is_col], true)) != CEL_OK) return st;
  }
  // The orthogonal checks of a pass are issued after the next pass's decode (or the final
  // commit), so the host's enqueue of them is not on the solve chain; the side stream runs
  // them right after that pass's own encoding checks.
  std::vector<int32_t> pending;
  int pending_col = 0;
  plan_range.reset();
  // passes: all solvable rows, then all solvable columns, until solved or stuck
  bool solved = false;
  std::vector<std::vector<int32_t>> by_solve;
  for (;;) {
    bool progress = false;
    for (int is_col = 0; is_col < 2; is_col++) {
      list.clear();
      for (uint32_t i = 0; i < W; i++)
        if (mb.cnt[is_col][i] >= k && mb.cnt[is_col][i] < W) list.push_back((int32_t)i);
      if (list.empty()) continue;
      if (first_issued) {  // the first row pass (the same list, issued above)
        first_issued = false;
      } else {
        Issued s1;
        if ((st = solve_issue(ctx, b, k, is_col, list, &s1)) != CEL_OK ||
            (st = solve_check(ctx, b, k, prev_col, prev)) != CEL_OK ||
            (st = check_pass(ctx, b, k, pending_col, pending, false)) != CEL_OK)
          return st;
        prev = s1;
        prev_col = is_col;
        pending.clear();
      }
      // sequential view of the pass: solve i fills its missing cells, completing the
      // orthogonal axes whose last missing cell it held
      const Range fill_range("repair.fill");
      mb.fill_pass(is_col, list, by_solve);
      log_pass(is_col, list, by_solve, order, solves, orth);
      // pending is empty here: the previous pass's orthogonal checks were issued (and
      // cleared) right after this pass's solve above, or this is the first pass
      pending.swap(orth);
      pending_col = !is_col;
      progress = true;
    }
    if (mb.total == cells) {
      solved = true;
      break;
    }
    if (!progress) break;
  }
  if ((st = verify_square(ctx, b, k, prev_col, prev, pending_col, pending)) != CEL_OK) return st;
  const uint8_t* const exp[2] = {row_roots, col_roots};
  cel_status code;
  const long f = first_failure(order.data(), order.size(), {b.hroots, kNode, RootRecords::BY_AXIS}, exp, b.hflags, W, &code);
  if (f >= 0) {
    const Check& c = order[(size_t)f];
    if (c.kind == Check::SANITY) return fail_axis(ctx, b, hm, out, code, c.is_col, c.idx, false);
    return repair_exact(ctx, b, hm, k, row_roots, col_roots, out);
  }
  if (!solved) {
    rollback(hm, W, solves, solves.size());
    return fail(ctx, CEL_EUNREPAIRABLE, "failed to solve data square");
  }
  std::fill(hm.begin(), hm.end(), (uint8_t)1);
  return CEL_OK;
}

static cel_status repair_bufs(cel_ctx* ctx, uint32_t k, bool own_eds, RepairBufs* b) {
  hipError_t e = hipSuccess;
  b->W = 2 * k;
  if (own_eds) b->eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, (size_t)b->W * b->W * kShare, &e));
  if (!b->eds) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  auto slot = [&](int sl, void (*walk)(Carver&, RepairBufs&)) {
    void* p = scratch(ctx, sl, carved(walk, nullptr, *b), &e);
    if (p) carved(walk, p, *b);
    return p != nullptr;
  };
  if (!slot(S_IN, carve_in) || !slot(S_AUX, carve_aux) || !slot(S_MASK, carve_mask) || !slot(S_WORK, carve_work) ||
      !slot(S_ROOTS, carve_roots))
    return fail(ctx, CEL_ENOMEM, "device allocation failed");
  b->res_bytes = (size_t)(reinterpret_cast<uint8_t*>(b->flags) - b->roots) + 2 * (size_t)b->W * 4;  // roots .. last flag
  if (!host_stage(ctx, carved(carve_stage, nullptr, *b))) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  carved(carve_stage, ctx->hstage, *b);
  b->slot = 0;
  b->solves = 0;
  // the side stream is the batch pipeline's (the ctx lock is held); the events are the repair's own
  b->main = ctx->stream;
  b->side = ctx->sub[0];
  b->ev_main = ctx->ev_repair_main;
  b->ev_side[0] = ctx->ev_repair_side[0];
  b->ev_side[1] = ctx->ev_repair_side[1];
  b->ev_done = ctx->ev_repair_done;
  // no stale record of an earlier call may gate this one: both streams start from here
  if ((e = hipEventRecord(b->ev_side[0], b->side)) != hipSuccess || (e = hipEventRecord(b->ev_side[1], b->side)) != hipSuccess)
    return hip_fail(ctx, e, "event");
  return CEL_OK;
}

// Both entry points with ctx->mu held: the repair of the caller's device square d_eds, or,
// with d_eds null, of the host square h_eds through the ctx's own buffer (uploaded before,
// downloaded after). `present` is handed back whenever the repair itself ran to an outcome.
static cel_status repair_locked(cel_ctx* ctx, uint8_t* h_eds, void* d_eds, uint8_t* present, uint32_t k,
                                uint32_t share_size, const uint8_t* row_roots, const uint8_t* col_roots,
                                const RepairOut& out) {
  if ((!h_eds && !d_eds) || !present || !row_roots || !col_roots) return fail(ctx, CEL_EINVAL, "nil argument");
  cel_status st = validate_square(ctx, k, share_size);
  if (st) return st;
  if (out.bad_axis) *out.bad_axis = -1;
  if (out.bad_index) *out.bad_index = -1;
  DeviceGuard g(ctx->device);
  const size_t cells = (size_t)4 * k * k, eds_b = cells * kShare;
  RepairBufs b{};
  b.eds = static_cast<uint8_t*>(d_eds);
  if ((st = repair_bufs(ctx, k, !d_eds, &b)) != CEL_OK) return st;
  hipStream_t s = ctx->stream;
  hipError_t e;
  std::vector<uint8_t> hm = normalise_mask(present, cells);
  if (!d_eds && (e = hipMemcpyAsync(b.eds, h_eds, eds_b, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  st = repair_core(ctx, b, hm, k, row_roots, col_roots, out);
  if (st != CEL_OK && st != CEL_EBYZANTINE && st != CEL_EBADROOT && st != CEL_EUNREPAIRABLE) return st;
  if (!d_eds) {  // the (partially) repaired square goes back either way, with the mask it is valid under
    if ((e = hipMemcpyAsync(h_eds, b.eds, eds_b, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  }
  std::memcpy(present, hm.data(), cells);
  return st;
}

// ------------------------------------------------------------ batch of squares
//
// cel_dev_repair_batch: the schedule of repair_core over n squares of one k (32, 64, 128: the
// in-square kernels) at once. Every pass is the merged pass of repair_plan.hpp (BatchPasses):
// one decode launch on the main stream and one check launch on the side stream serve every
// square that has axes in it, one commit takes all n squares' roots, and one copy brings the
// roots and flags back. Only the verdict is per square.
//
// Every scratch slot and the page-locked stage start with the single-square layout (the same
// walk as RepairBufs), the batch's regions after it: a square whose SOLVE or ORTH check
// fails is replayed alone by repair_exact through a RepairBufs whose eds is that square's
// slice of the batch, without a reallocation under the batch's buffers.
struct BatchBufs {
  uint32_t W, n;
  RepairBufs one;     // the single-square prefix of every slot (eds unset)
  uint8_t* eds;       // [n][W][W][512]
  uint8_t* mask;      // [n][W*W], then the first pass's entries (one upload for both)
  int32_t* list0;     // [n*W]
  uint8_t* work;      // the n-square commit's workspace
  uint8_t* roots;     // [n][W][90] row roots, [n][W][90] column roots, then the flags
  int32_t* flags;     // [n][2][W] by (square, direction, axis)
  uint8_t* hroots;    // page-locked copy of roots + flags (one D2H of res_bytes)
  int32_t* hflags;
  size_t res_bytes;
  int32_t* idx;       // [kIdxSlots][n*W] device entry lists
  int32_t* hidx;      // page-locked staging of the same
  uint8_t* hmask;     // page-locked staging of masks + first entries
  int32_t* hlist0;
  uint32_t slot;
  hipStream_t main, side;
  hipEvent_t ev_main, ev_done;
  size_t slot_len() const { return (size_t)n * W; }
};

static void take_batch_mask_list(Carver& c, const BatchBufs& b, uint8_t** mask, int32_t** list0) {
  *mask = c.take<uint8_t>((size_t)b.n * b.W * b.W);
  *list0 = c.take<int32_t>(b.slot_len() * 4);
}
static void take_batch_results(Carver& c, const BatchBufs& b, uint8_t** roots, int32_t** flags) {
  *roots = c.take<uint8_t>((size_t)b.n * 2 * b.W * kNode);
  *flags = c.take<int32_t>((size_t)b.n * 2 * b.W * 4);
}
static void carve_batch_in(Carver& c, BatchBufs& b) { carve_in(c, b.one); }  // S_IN: the replay's alone
static void carve_batch_aux(Carver& c, BatchBufs& b) {                       // S_AUX
  carve_aux(c, b.one);
  b.idx = c.take<int32_t>((size_t)kIdxSlots * b.slot_len() * 4);
}
static void carve_batch_mask(Carver& c, BatchBufs& b) {  // S_MASK
  carve_mask(c, b.one);
  take_batch_mask_list(c, b, &b.mask, &b.list0);
}
static void carve_batch_work(Carver& c, BatchBufs& b) {  // S_WORK
  carve_work(c, b.one);
  b.work = c.take<uint8_t>(nmt_workspace_size(b.W / 2, b.n));
}
static void carve_batch_roots(Carver& c, BatchBufs& b) {  // S_ROOTS
  carve_roots(c, b.one);
  take_batch_results(c, b, &b.roots, &b.flags);
}
static void carve_batch_stage(Carver& c, BatchBufs& b) {  // the page-locked stage
  carve_stage(c, b.one);
  b.hidx = c.take<int32_t>((size_t)kIdxSlots * b.slot_len() * 4);
  take_batch_mask_list(c, b, &b.hmask, &b.hlist0);
  take_batch_results(c, b, &b.hroots, &b.hflags);
}
static size_t carved(void (*walk)(Carver&, BatchBufs&), void* base, BatchBufs& b) {
  Carver c(base);
  walk(c, b);
  return c.size();
}
constexpr struct {
  int slot;
  void (*walk)(Carver&, BatchBufs&);
} kBatchSlots[] = {{S_IN, carve_batch_in},     {S_AUX, carve_batch_aux},     {S_MASK, carve_batch_mask},
                   {S_WORK, carve_batch_work}, {S_ROOTS, carve_batch_roots}};

// k = 32, 64, 128 and more than one square: the merged schedule; else square after square.
static bool batch_merged(uint32_t k, uint32_t n) {
  return n > 1 && (k == 32 || k == 64 || k == 128) && entries_fit(n, 2 * k);
}

static cel_status batch_bufs(cel_ctx* ctx, uint32_t k, uint32_t n, BatchBufs* b) {
  hipError_t e = hipSuccess;
  b->W = b->one.W = 2 * k;
  b->n = n;
  for (const auto& s : kBatchSlots) {
    void* p = scratch(ctx, s.slot, carved(s.walk, nullptr, *b), &e);
    if (!p) return fail(ctx, CEL_ENOMEM, "device allocation failed");
    carved(s.walk, p, *b);
  }
  b->res_bytes = (size_t)(reinterpret_cast<uint8_t*>(b->flags) - b->roots) + (size_t)n * 2 * b->W * 4;
  if (!host_stage(ctx, carved(carve_batch_stage, nullptr, *b))) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  carved(carve_batch_stage, ctx->hstage, *b);
  b->slot = 0;
  b->main = ctx->stream;
  b->side = ctx->sub[0];
  b->ev_main = ctx->ev_repair_main;
  b->ev_done = ctx->ev_repair_done;
  return CEL_OK;
}

// `list` into the next entry-list slot, uploaded on stream s (upload_list's rule).
static cel_status upload_entries(cel_ctx* ctx, BatchBufs& b, const std::vector<int32_t>& list, hipStream_t s,
                                 int32_t** d_list) {
  hipError_t e;
  if (b.slot == kIdxSlots) {
    if ((e = hipStreamSynchronize(b.main)) != hipSuccess || (e = hipStreamSynchronize(b.side)) != hipSuccess)
      return hip_fail(ctx, e, "sync");
    b.slot = 0;
  }
  int32_t* hidx = b.hidx + (size_t)b.slot * b.slot_len();
  *d_list = b.idx + (size_t)b.slot * b.slot_len();
  b.slot++;
  std::memcpy(hidx, list.data(), list.size() * 4);
  if ((e = hipMemcpyAsync(*d_list, hidx, list.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  return CEL_OK;
}

// A merged pass's decode on the main stream, then ev_main (solve_issue); `uploaded`: the
// entries are on the device already (the first pass, in the masks' upload).
static cel_status batch_solve_issue(cel_ctx* ctx, BatchBufs& b, const std::vector<int32_t>& list, Issued* out,
                                    int32_t* uploaded = nullptr) {
  const Range range("repair.batch.solve");
  out->na = (uint32_t)list.size();
  if (!out->na) return CEL_OK;
  cel_status st;
  if (uploaded) out->idx = uploaded;
  else if ((st = upload_entries(ctx, b, list, b.main, &out->idx)) != CEL_OK) return st;
  if ((st = fuzz(ctx, b.main)) != CEL_OK) return st;
  hipError_t e;
  if ((e = launch_rs_decode_in_squares(b.eds, b.mask, b.W, b.n, out->idx, out->na, ctx->tables.mul8, b.main)) !=
          hipSuccess ||
      (e = hipEventRecord(b.ev_main, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "solve");
  return CEL_OK;
}

// Its encoding check on the side stream, after ev_main (solve_check).
static cel_status batch_solve_check(cel_ctx* ctx, BatchBufs& b, const Issued& s) {
  if (!s.na) return CEL_OK;
  hipError_t e;
  if ((e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess) return hip_fail(ctx, e, "event");
  cel_status st;
  if ((st = fuzz(ctx, b.side)) != CEL_OK) return st;
  if ((e = launch_rs_check_axes_batch(b.eds, b.W / 2, b.n, s.idx, s.na, b.flags, b.side)) != hipSuccess)
    return hip_fail(ctx, e, "encoding check");
  return CEL_OK;
}

// Encoding check of complete axes (sanity, orthogonal completions) on the side stream (check_pass).
static cel_status batch_check_pass(cel_ctx* ctx, BatchBufs& b, const std::vector<int32_t>& list, bool wait_main) {
  const Range range("repair.batch.check");
  if (list.empty()) return CEL_OK;
  hipError_t e;
  if (wait_main &&
      ((e = hipEventRecord(b.ev_main, b.main)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess))
    return hip_fail(ctx, e, "event");
  int32_t* idx;
  cel_status st;
  if ((st = upload_entries(ctx, b, list, b.side, &idx)) != CEL_OK || (st = fuzz(ctx, b.side)) != CEL_OK) return st;
  if ((e = launch_rs_check_axes_batch(b.eds, b.W / 2, b.n, idx, (uint32_t)list.size(), b.flags, b.side)) != hipSuccess)
    return hip_fail(ctx, e, "encoding check");
  return CEL_OK;
}

struct BatchOut {
  cel_status* status;
  int32_t* bad_axis;
  int32_t* bad_index;
  uint8_t* byz_shares;   // nullable, [n][W][512]
  uint8_t* byz_present;  // nullable, [n][W]
  RepairOut of(uint32_t i, uint32_t W) const {
    return RepairOut{bad_axis ? bad_axis + i : nullptr, bad_index ? bad_index + i : nullptr,
                     byz_shares ? byz_shares + (size_t)i * W * kShare : nullptr,
                     byz_present ? byz_present + (size_t)i * W : nullptr};
  }
};

// The squares resident at b.eds, masks hm ([n][W*W] bytes 0 / 1, updated per square as
// repair_core leaves its own). CEL_OK when every square ran to an outcome (out.status).
static cel_status repair_batch_core(cel_ctx* ctx, BatchBufs& b, std::vector<uint8_t>& hm, uint32_t k,
                                    const uint8_t* row_roots, const uint8_t* col_roots, const BatchOut& out,
                                    std::string* first_error) {
  const uint32_t W = 2 * k, n = b.n;
  const size_t cells = (size_t)W * W;
  hipError_t e = hipSuccess;
  cel_status st;
  struct SideDrain {
    hipStream_t side;
    ~SideDrain() { (void)hipStreamSynchronize(side); }
  } drain{b.side};
  // every square's first row pass goes to the device before any bookkeeping exists; its
  // entries ride in the masks' upload
  const std::vector<int32_t> first = first_row_pass_batch(hm, n, k);
  std::memcpy(b.hmask, hm.data(), n * cells);
  if (!first.empty()) std::memcpy(b.hlist0, first.data(), first.size() * 4);
  const size_t up_b = (size_t)(reinterpret_cast<uint8_t*>(b.hlist0) - b.hmask) + first.size() * 4;
  if ((e = hipMemcpyAsync(b.mask, b.hmask, up_b, hipMemcpyHostToDevice, b.main)) != hipSuccess ||
      (e = hipEventRecord(b.ev_main, b.main)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess ||
      (e = hipMemsetAsync(b.flags, 0, (size_t)n * 2 * W * 4, b.side)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  Issued prev;
  if ((st = batch_solve_issue(ctx, b, first, &prev, b.list0)) != CEL_OK) return st;
  bool first_issued = !first.empty();
  std::unique_ptr<Range> plan_range(new Range("repair.batch.plan"));
  BatchPasses bp(hm, n, k);
  for (int is_col = 0; is_col < 2; is_col++)
    if ((st = batch_check_pass(ctx, b, bp.sanity[is_col], true)) != CEL_OK) return st;
  plan_range.reset();
  // each pass's checks (its own, then the orthogonal completions) follow the next pass's decode
  std::vector<int32_t> list, pending;
  int is_col;
  while (bp.next(&is_col, list)) {
    if (first_issued) {  // the first row pass (the same entries, issued above)
      first_issued = false;
    } else {
      Issued s1;
      if ((st = batch_solve_issue(ctx, b, list, &s1)) != CEL_OK || (st = batch_solve_check(ctx, b, prev)) != CEL_OK ||
          (st = batch_check_pass(ctx, b, pending, false)) != CEL_OK)
        return st;
      prev = s1;
    }
    const Range fill_range("repair.batch.fill");
    bp.apply(pending);
  }
  // the last pass's checks beside the commit of all n squares, the join, one download
  const size_t roots_b = (size_t)n * W * kNode;
  if ((st = fuzz(ctx, b.main)) != CEL_OK || (st = batch_solve_check(ctx, b, prev)) != CEL_OK ||
      (st = batch_check_pass(ctx, b, pending, false)) != CEL_OK)
    return st;
  if ((e = launch_commit(b.eds, k, n, b.roots, b.roots + roots_b, nullptr, nullptr, b.work, false, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "roots");
  if ((e = hipEventRecord(b.ev_done, b.side)) != hipSuccess || (e = hipStreamWaitEvent(b.main, b.ev_done, 0)) != hipSuccess)
    return hip_fail(ctx, e, "join");
  if ((e = hipMemcpyAsync(b.hroots, b.roots, b.res_bytes, hipMemcpyDeviceToHost, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(b.main)) != hipSuccess) return hip_fail(ctx, e, "sync");
  // The verdicts, square by square. A replay (repair_exact) reuses the single-square prefix of
  // the slots and of the stage, so the batch's results leave the stage first.
  const std::vector<uint8_t> got_all(b.hroots, b.hroots + 2 * roots_b);
  const std::vector<int32_t> flags_all(b.hflags, b.hflags + (size_t)n * 2 * W);
  std::vector<uint8_t> got(2 * (size_t)W * kNode);
  for (uint32_t i = 0; i < n; i++) {
    SquarePasses& sq = bp.sq[i];
    const uint8_t* const exp[2] = {row_roots + (size_t)i * W * kNode, col_roots + (size_t)i * W * kNode};
    square_roots(got_all.data(), n, W, i, got.data());
    std::vector<uint8_t> m(hm.begin() + (ptrdiff_t)(i * cells), hm.begin() + (ptrdiff_t)((i + 1) * cells));
    const RepairOut o = out.of(i, W);
    RepairBufs one = b.one;
    one.eds = b.eds + i * cells * kShare;
    cel_status code;
    const long f = first_failure(sq.order.data(), sq.order.size(), {got.data(), kNode, RootRecords::BY_AXIS}, exp,
                                 flags_all.data() + (size_t)i * 2 * W, W, &code);
    if (f >= 0) {
      const Check& c = sq.order[(size_t)f];
      if (c.kind == Check::SANITY) {
        st = fail_axis(ctx, one, m, o, code, c.is_col, c.idx, false);
      } else {  // the order decides which axis fails first: this square again, alone, in rsmt2d's order
        if ((st = repair_bufs(ctx, k, false, &one)) != CEL_OK) return st;
        st = repair_exact(ctx, one, m, k, exp[0], exp[1], o);
      }
    } else if (!sq.solved()) {
      rollback(m, W, sq.solves, sq.solves.size());
      st = fail(ctx, CEL_EUNREPAIRABLE, "failed to solve data square");
    } else {
      std::fill(m.begin(), m.end(), (uint8_t)1);
      st = CEL_OK;
    }
    if (st != CEL_OK && st != CEL_EBYZANTINE && st != CEL_EBADROOT && st != CEL_EUNREPAIRABLE) return st;
    if (st != CEL_OK && first_error->empty()) *first_error = "square " + std::to_string(i) + ": " + ctx->last_error;
    out.status[i] = st;
    std::memcpy(hm.data() + i * cells, m.data(), cells);
  }
  return CEL_OK;
}

// Both batch entry points with ctx->mu held: the caller's device squares d_eds, or, with d_eds
// null, the host squares h_eds through the ctx's own buffer.
static cel_status repair_batch_locked(cel_ctx* ctx, uint8_t* h_eds, void* d_eds, uint8_t* present, uint32_t n,
                                      uint32_t k, uint32_t share_size, const uint8_t* row_roots,
                                      const uint8_t* col_roots, const BatchOut& out) {
  if ((!h_eds && !d_eds) || !present || !row_roots || !col_roots || !out.status)
    return fail(ctx, CEL_EINVAL, "nil argument");
  // the call's own arguments fail with CEL_EINVAL; the statuses of a repair are the squares'
  cel_status st = validate_square(ctx, k, share_size);
  if (st) return st == CEL_ECHUNK ? st : CEL_EINVAL;
  if (n == 0) return CEL_OK;
  const uint32_t W = 2 * k;
  const size_t cells = (size_t)W * W, eds_b = cells * kShare;
  std::string first_error;
  if (!batch_merged(k, n)) {  // square after square through the single repair
    for (uint32_t i = 0; i < n; i++) {
      st = repair_locked(ctx, h_eds ? h_eds + i * eds_b : nullptr, d_eds ? static_cast<uint8_t*>(d_eds) + i * eds_b : nullptr,
                         present + i * cells, k, share_size, row_roots + (size_t)i * W * kNode,
                         col_roots + (size_t)i * W * kNode, out.of(i, W));
      if (st != CEL_OK && st != CEL_EBYZANTINE && st != CEL_EBADROOT && st != CEL_EUNREPAIRABLE) return st;
      if (st != CEL_OK && first_error.empty()) first_error = "square " + std::to_string(i) + ": " + ctx->last_error;
      out.status[i] = st;
    }
    if (!first_error.empty()) ctx->last_error = first_error;
    return CEL_OK;
  }
  for (int32_t* bad : {out.bad_axis, out.bad_index})
    if (bad) std::fill(bad, bad + n, -1);
  DeviceGuard g(ctx->device);
  BatchBufs b{};
  if ((st = batch_bufs(ctx, k, n, &b)) != CEL_OK) return st;
  hipError_t e = hipSuccess;
  b.eds = static_cast<uint8_t*>(d_eds);
  if (!d_eds) {
    if (!(b.eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, n * eds_b, &e)))) return fail(ctx, CEL_ENOMEM, "device allocation failed");
    if ((e = hipMemcpyAsync(b.eds, h_eds, n * eds_b, hipMemcpyHostToDevice, b.main)) != hipSuccess)
      return hip_fail(ctx, e, "H2D");
  }
  std::vector<uint8_t> hm = normalise_mask(present, n * cells);
  if ((st = repair_batch_core(ctx, b, hm, k, row_roots, col_roots, out, &first_error)) != CEL_OK) return st;
  if (!d_eds) {  // every (partially) repaired square goes back, with the mask it is valid under
    if ((e = hipMemcpyAsync(h_eds, b.eds, n * eds_b, hipMemcpyDeviceToHost, b.main)) != hipSuccess) return hip_fail(ctx, e, "D2H");
    if ((e = hipStreamSynchronize(b.main)) != hipSuccess) return hip_fail(ctx, e, "sync");
  }
  std::memcpy(present, hm.data(), n * cells);
  if (!first_error.empty()) ctx->last_error = first_error;
  return CEL_OK;
}

}  // namespace

cel_status cel_repair(cel_ctx* ctx, uint8_t* eds, uint8_t* present, uint32_t k, uint32_t share_size,
                      const uint8_t* row_roots, const uint8_t* col_roots, int32_t* bad_axis, int32_t* bad_index,
                      uint8_t* byz_shares, uint8_t* byz_present) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  return repair_locked(ctx, eds, nullptr, present, k, share_size, row_roots, col_roots,
                       RepairOut{bad_axis, bad_index, byz_shares, byz_present});
}

cel_status cel_debug_repair_plan(const uint8_t* present, uint32_t k, int32_t* solve_axis, int32_t* solve_index,
                                 int32_t* solve_level, uint32_t* nsolves, int32_t* solved) {
  if (!present || !solve_axis || !solve_index || !solve_level || !nsolves || !solved || !k || (k & (k - 1)) ||
      k > 512)
    return CEL_EINVAL;
  const SweepPlan p = plan_sweeps(normalise_mask(present, (size_t)4 * k * k), k);
  for (size_t t = 0; t < p.solves.size(); t++) {
    solve_axis[t] = p.solves[t].is_col;
    solve_index[t] = p.solves[t].idx;
    solve_level[t] = p.level[t];
  }
  *nsolves = (uint32_t)p.solves.size();
  *solved = p.solved ? 1 : 0;
  return CEL_OK;
}

cel_status cel_debug_schedule_fuzz(cel_ctx* ctx, uint64_t seed, uint32_t max_us) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (max_us > 100000) return fail(ctx, CEL_EINVAL, "max_us above 100 ms");
  ctx->fuzz_state = seed;
  ctx->fuzz_max_us = max_us;
  return CEL_OK;
}

cel_status cel_dev_repair(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k, const uint8_t* row_roots,
                          const uint8_t* col_roots, int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares,
                          uint8_t* byz_present) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  return dev_repair_locked(ctx, d_eds, present, k, row_roots, col_roots, bad_axis, bad_index, byz_shares, byz_present);
}

size_t cel_dev_repair_batch_scratch_size(uint32_t k, uint32_t n) {
  if (!k || (k & (k - 1)) || k > 512 || n == 0) return 0;
  size_t total = 0;
  if (!batch_merged(k, n)) {  // one square at a time
    RepairBufs b{};
    b.W = 2 * k;
    for (auto walk : {carve_in, carve_aux, carve_mask, carve_work, carve_roots}) total += carved(walk, nullptr, b);
    return total;
  }
  BatchBufs b{};
  b.W = b.one.W = 2 * k;
  b.n = n;
  for (const auto& s : kBatchSlots) total += carved(s.walk, nullptr, b);
  return total;
}

cel_status cel_dev_repair_batch(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t n, uint32_t k,
                                const uint8_t* row_roots, const uint8_t* col_roots, cel_status* status,
                                int32_t* bad_axis, int32_t* bad_index, uint8_t* byz_shares, uint8_t* byz_present) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  return repair_batch_locked(ctx, nullptr, d_eds, present, n, k, kShare, row_roots, col_roots,
                             BatchOut{status, bad_axis, bad_index, byz_shares, byz_present});
}

cel_status cel_repair_batch(cel_ctx* ctx, uint8_t* eds, uint8_t* present, uint32_t n, uint32_t k, uint32_t share_size,
                            const uint8_t* row_roots, const uint8_t* col_roots, cel_status* status, int32_t* bad_axis,
                            int32_t* bad_index, uint8_t* byz_shares, uint8_t* byz_present) {
  if (!ctx) return CEL_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  return repair_batch_locked(ctx, eds, nullptr, present, n, k, share_size, row_roots, col_roots,
                             BatchOut{status, bad_axis, bad_index, byz_shares, byz_present});
}

cel_status cel_debug_repair_batch_plan(const uint8_t* present, uint32_t n, uint32_t k, int32_t* pass_dir,
                                       uint32_t* pass_off, uint32_t* npasses, uint32_t* ent_square,
                                       int32_t* ent_axis) {
  if (!present || !pass_dir || !pass_off || !npasses || !ent_square || !ent_axis || !n || !k || (k & (k - 1)) ||
      !entries_fit(n, 2 * k))
    return CEL_EINVAL;
  const std::vector<uint8_t> hm = normalise_mask(present, (size_t)n * 4 * k * k);
  BatchPasses bp(hm, n, k);
  const std::vector<BatchPass> passes = plan_batch(bp);
  uint32_t at = 0;
  for (size_t p = 0; p < passes.size(); p++) {
    pass_dir[p] = passes[p].is_col;
    pass_off[p] = at;
    for (int32_t e : passes[p].entries) {
      ent_square[at] = entry_square(e);
      ent_axis[at++] = (int32_t)entry_axis(e);
    }
  }
  pass_off[passes.size()] = at;
  *npasses = (uint32_t)passes.size();
  return CEL_OK;
}

}  // extern "C"

// cel_dev_repair with ctx->mu held (also the second half of cel_repair_samples, api_verify.cpp).
cel_status cel::abi::dev_repair_locked(cel_ctx* ctx, void* d_eds, uint8_t* present, uint32_t k,
                                       const uint8_t* row_roots, const uint8_t* col_roots, int32_t* bad_axis,
                                       int32_t* bad_index, uint8_t* byz_shares, uint8_t* byz_present) {
  return repair_locked(ctx, nullptr, d_eds, present, k, kShare, row_roots, col_roots,
                       RepairOut{bad_axis, bad_index, byz_shares, byz_present});
}
