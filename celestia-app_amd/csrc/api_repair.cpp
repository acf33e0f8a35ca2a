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

// What the pass schedule works on, of one square (RepairBufs) or of the n squares of a merged
// batch (BatchBufs): a list slot holds a pass of either, up to n * W entries.
struct PassBufs {
  uint32_t W, n = 1;
  uint8_t* eds;       // [n][W][W][512]
  uint8_t* mask;      // [n][W*W]
  int32_t* list0;     // the first pass's list, right after the masks (one upload for both)
  uint8_t* work;      // NMT workspace of the n-square commit (one square: or repair_exact's axes roots)
  uint8_t* roots;     // [n][W][90] row roots, [n][W][90] column roots, then the flags
  int32_t* flags;     // [n][2][W] encoding-check flags by (square, direction, axis), right after the roots
  uint8_t* hroots;    // page-locked copy of roots + flags (one D2H of res_bytes at the end)
  int32_t* hflags;
  size_t res_bytes;
  int32_t* idx;       // [kIdxSlots][n*W] device lists
  int32_t* hidx;      // [kIdxSlots][n*W] page-locked staging of the same
  uint8_t* hmask;     // page-locked staging of the masks, then of the first list
  int32_t* hlist0;
  uint32_t slot;      // next free slot
  // Two streams: the solve chain runs on `main`; every re-encode check (of the solved axes,
  // the sanity and the orthogonal checks) runs on `side`, off the chain's critical path: its
  // outcome is only read at the end.
  hipStream_t main, side;
  hipEvent_t ev_main;  // the squares after the main stream's latest pass
  hipEvent_t ev_done;  // the side stream's last check
  size_t slot_len() const { return (size_t)n * W; }
};

// One square, any k: with the dense path's buffers (gather -> decode -> scatter where no
// in-square kernel exists) and repair_exact's.
struct RepairBufs : PassBufs {
  uint8_t* dense[2];  // gathered axes of the solve passes, alternating (main stream)
  uint8_t* dmask;
  uint8_t* dchk;      // gathered axes of the check passes (side stream)
  uint8_t* dmask_chk;
  uint8_t* tmp;       // re-encoded parity halves (side stream)
  uint32_t* rec;      // [2][W][kNodeWords] repair_exact's root records, in work's slot
  uint32_t solves;    // solve passes so far (which dense buffer is next)
  hipEvent_t ev_side[2];  // the side stream is done with dense[i]
};

// Every scratch slot and the page-locked stage of a batch start with the single-square layout
// (the same walks), the batch's regions after it: a square whose SOLVE or ORTH check fails is
// replayed alone by repair_exact through a RepairBufs whose eds is that square's slice of the
// batch, without a reallocation under the batch's buffers.
struct BatchBufs : PassBufs {
  RepairBufs one;  // the single-square prefix of every slot (eds, streams and events unset)
};

// The layout of each scratch slot and of the page-locked stage, one walk per buffer (W and n
// set). carved() runs a walk: on a null base it gives the size to allocate, on the
// allocation the pointers into it.
static void carve_in(Carver& c, RepairBufs& b) {  // S_IN
  for (uint8_t** p : {&b.dense[0], &b.dense[1], &b.dchk}) *p = c.take<uint8_t>((size_t)b.W * b.W * kShare);
}
static void carve_aux(Carver& c, RepairBufs& b) {  // S_AUX
  b.tmp = c.take<uint8_t>((size_t)b.W * b.W * kShare / 2);
  b.idx = c.take<int32_t>((size_t)kIdxSlots * b.W * 4);
}
// The presence masks, then the first pass's list directly after them: one upload carries
// both, so the device buffer and the stage take them by the same walk.
static void take_mask_list(Carver& c, uint32_t n, uint32_t W, uint8_t** mask, int32_t** list0) {
  *mask = c.take<uint8_t>((size_t)n * W * W);
  *list0 = c.take<int32_t>((size_t)n * W * 4);
}
static void carve_mask(Carver& c, RepairBufs& b) {  // S_MASK
  take_mask_list(c, 1, b.W, &b.mask, &b.list0);
  for (uint8_t** p : {&b.dmask, &b.dmask_chk}) *p = c.take<uint8_t>((size_t)b.W * b.W);
}
// Every root of the squares, then the flags directly after them: one download (res_bytes,
// from the first root to the last flag) brings both back, into the same walk of the stage.
static void take_results(Carver& c, uint32_t n, uint32_t W, uint8_t** roots, int32_t** flags) {
  *roots = c.take<uint8_t>((size_t)n * 2 * W * kNode);
  *flags = c.take<int32_t>((size_t)n * 2 * W * 4);
}
static void carve_roots(Carver& c, RepairBufs& b) { take_results(c, 1, b.W, &b.roots, &b.flags); }  // S_ROOTS
// repair_exact's axes-roots workspace of one direction's 2k axes, then, after it, the root
// records of both directions; the whole-square commit's workspace lies over the two.
static void carve_work(Carver& c, RepairBufs& b) {  // S_WORK
  b.work = c.take<uint8_t>(axes_roots_workspace_size(b.W / 2, b.W));
  b.rec = c.take<uint32_t>(2 * (size_t)b.W * kNodeWords * 4);
  c.overlay(nmt_workspace_size(b.W / 2, 1));
}
static void carve_stage(Carver& c, RepairBufs& b) {  // the page-locked stage
  b.hidx = c.take<int32_t>((size_t)kIdxSlots * b.W * 4);
  take_mask_list(c, 1, b.W, &b.hmask, &b.hlist0);  // hmask followed by its list
  take_results(c, 1, b.W, &b.hroots, &b.hflags);
}
static void carve_batch_in(Carver& c, BatchBufs& b) { carve_in(c, b.one); }  // S_IN: the replay's alone
static void carve_batch_aux(Carver& c, BatchBufs& b) {                       // S_AUX
  carve_aux(c, b.one);
  b.idx = c.take<int32_t>((size_t)kIdxSlots * b.slot_len() * 4);
}
static void carve_batch_mask(Carver& c, BatchBufs& b) {  // S_MASK
  carve_mask(c, b.one);
  take_mask_list(c, b.n, b.W, &b.mask, &b.list0);
}
static void carve_batch_work(Carver& c, BatchBufs& b) {  // S_WORK
  carve_work(c, b.one);
  b.work = c.take<uint8_t>(nmt_workspace_size(b.W / 2, b.n));
}
static void carve_batch_roots(Carver& c, BatchBufs& b) {  // S_ROOTS
  carve_roots(c, b.one);
  take_results(c, b.n, b.W, &b.roots, &b.flags);
}
static void carve_batch_stage(Carver& c, BatchBufs& b) {  // the page-locked stage
  carve_stage(c, b.one);
  b.hidx = c.take<int32_t>((size_t)kIdxSlots * b.slot_len() * 4);
  take_mask_list(c, b.n, b.W, &b.hmask, &b.hlist0);
  take_results(c, b.n, b.W, &b.hroots, &b.hflags);
}
template <class B>
static size_t carved(void (*walk)(Carver&, B&), void* base, B& b) {
  Carver c(base);
  walk(c, b);
  return c.size();
}
// The scratch slots of either form, with their walks: what is allocated, and what
// cel_dev_repair_batch_scratch_size adds up.
template <class B>
struct SlotWalk {
  int slot;
  void (*walk)(Carver&, B&);
};
constexpr SlotWalk<RepairBufs> kSquareSlots[] = {
    {S_IN, carve_in}, {S_AUX, carve_aux}, {S_MASK, carve_mask}, {S_WORK, carve_work}, {S_ROOTS, carve_roots}};
constexpr SlotWalk<BatchBufs> kBatchSlots[] = {{S_IN, carve_batch_in},     {S_AUX, carve_batch_aux},     {S_MASK, carve_batch_mask},
                                               {S_WORK, carve_batch_work}, {S_ROOTS, carve_batch_roots}};
template <class B, size_t N>
static size_t slots_size(const SlotWalk<B> (&slots)[N], B& b) {
  size_t total = 0;
  for (const auto& s : slots) total += carved(s.walk, nullptr, b);
  return total;
}

// b's scratch slots and page-locked stage (W and n set), the ctx's streams and the repair's
// own events: everything of PassBufs but eds.
template <class B, size_t N>
static cel_status carve_bufs(cel_ctx* ctx, const SlotWalk<B> (&slots)[N], void (*stage)(Carver&, B&), B* b) {
  hipError_t e = hipSuccess;
  for (const auto& s : slots) {
    void* p = scratch(ctx, s.slot, carved(s.walk, nullptr, *b), &e);
    if (!p) return fail(ctx, CEL_ENOMEM, "device allocation failed");
    carved(s.walk, p, *b);
  }
  b->res_bytes = (size_t)(reinterpret_cast<uint8_t*>(b->flags) - b->roots) + (size_t)b->n * 2 * b->W * 4;  // roots .. last flag
  if (!host_stage(ctx, carved(stage, nullptr, *b))) return fail(ctx, CEL_ENOMEM, "page-locked allocation failed");
  carved(stage, ctx->hstage, *b);
  b->slot = 0;
  // the side stream is the batch pipeline's (the ctx lock is held); the events are the repair's own
  b->main = ctx->stream;
  b->side = ctx->sub[0];
  b->ev_main = ctx->ev_repair_main;
  b->ev_done = ctx->ev_repair_done;
  return CEL_OK;
}

// `list` into the next list slot, uploaded on stream s. Every slot in flight: drain both
// streams (the side stream's compares read the lists too), then reuse.
static cel_status upload_list(cel_ctx* ctx, PassBufs& b, const std::vector<int32_t>& list, hipStream_t s,
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

// A pass's decode as issued: what its encoding check, enqueued later, needs.
struct Issued {
  uint32_t na = 0;
  int is_col = 0;
  uint32_t d = 0;  // dense path: which dense buffer
  int32_t* idx = nullptr;
};

// The names of the schedule's ranges in a trace.
struct RangeNames {
  const char *solve, *check, *plan, *fill;
};

// What differs on the device between the schedule of one square and of a merged batch: the
// decode of a pass (main stream), the encoding check of the axes it solved and of complete
// axes (side stream). run_passes enqueues everything around them.
//
// One square, any k. W = 32 .. 256 decode and check in the square; else the decode is gather ->
// decode -> scatter through dense[d], d alternating, and its check reads dense[d]: the decode
// waits for ev_side[d] (the side stream is done with the buffer), the check records it. That
// check must be enqueued before the solve after next, which reuses dense[d].
struct SquareOps {
  static constexpr RangeNames kRanges = {"repair.solve", "repair.check", "repair.plan", "repair.fill"};
  cel_ctx* ctx;
  RepairBufs& b;
  const uint32_t k = b.W / 2;
  const bool in_square = rs_decode_axis_supported(b.W, kShare);
  hipError_t decode(Issued& s) {
    s.d = b.solves++ & 1u;
    hipError_t e;
    if (!in_square && (e = hipStreamWaitEvent(b.main, b.ev_side[s.d], 0)) != hipSuccess) return e;
    return decode_axes(ctx, b, k, s.idx, s.is_col, s.na, b.dense[s.d], b.main);
  }
  cel_status check_solved(const Issued& s) {
    if (in_square) return check_complete(s.is_col, s.na, s.idx);  // the completed axes are checked in the square
    const cel_status st = encode_check(ctx, b, k, s.is_col, s.na, b.dense[s.d], s.idx, b.side);
    if (st != CEL_OK) return st;
    const hipError_t e = hipEventRecord(b.ev_side[s.d], b.side);
    return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "event");
  }
  cel_status check_complete(int is_col, uint32_t na, const int32_t* idx) {
    return check_in_square(ctx, b, k, is_col, na, idx, b.side);
  }
};

// The merged batch, k = 32, 64, 128: one launch serves every square with entries in the list
// (square and direction are in the entry).
struct BatchOps {
  static constexpr RangeNames kRanges = {"repair.batch.solve", "repair.batch.check", "repair.batch.plan",
                                         "repair.batch.fill"};
  cel_ctx* ctx;
  BatchBufs& b;
  hipError_t decode(Issued& s) {
    return launch_rs_decode_in_squares(b.eds, b.mask, b.W, b.n, s.idx, s.na, ctx->tables.mul8, b.main);
  }
  cel_status check_solved(const Issued& s) { return check_complete(s.is_col, s.na, s.idx); }
  cel_status check_complete(int, uint32_t na, const int32_t* idx) {
    const hipError_t e = launch_rs_check_axes_batch(b.eds, b.W / 2, b.n, idx, na, b.flags, b.side);
    return e == hipSuccess ? CEL_OK : hip_fail(ctx, e, "encoding check");
  }
};

// rsmt2d solveCrossword's decode of `list` (incomplete axes of one direction), in two
// halves so the host can put other side-stream work between them:
//   solve_issue  the decode on the main stream, then ev_main; `uploaded`: the list is on the
//                device there already (the first pass, in the masks' upload);
//   solve_check  the encoding check of the solved axes on the side stream, after ev_main
//                (that solve's record or a later one of the main stream: the axes it checks
//                are final from their pass on).
// Nothing is synchronised: every flag is read back once at the end of the repair.
template <class Ops>
static cel_status solve_issue(Ops& ops, int is_col, const std::vector<int32_t>& list, Issued* out,
                              int32_t* uploaded = nullptr) {
  const Range range(Ops::kRanges.solve);
  PassBufs& b = ops.b;
  out->is_col = is_col;
  out->na = (uint32_t)list.size();
  if (!out->na) return CEL_OK;
  cel_status st;
  if (uploaded) out->idx = uploaded;
  else if ((st = upload_list(ops.ctx, b, list, b.main, &out->idx)) != CEL_OK) return st;
  if ((st = fuzz(ops.ctx, b.main)) != CEL_OK) return st;
  hipError_t e;
  if ((e = ops.decode(*out)) != hipSuccess || (e = hipEventRecord(b.ev_main, b.main)) != hipSuccess)
    return hip_fail(ops.ctx, e, "solve");
  return CEL_OK;
}

template <class Ops>
static cel_status solve_check(Ops& ops, const Issued& s) {
  if (!s.na) return CEL_OK;
  PassBufs& b = ops.b;
  hipError_t e;
  if ((e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess) return hip_fail(ops.ctx, e, "event");
  const cel_status st = fuzz(ops.ctx, b.side);
  return st != CEL_OK ? st : ops.check_solved(s);
}

// Encoding check of complete axes (preRepairSanityCheck, and the orthogonal axes a solve
// completed) on the side stream. wait_main: after the main stream's latest work; without
// it the caller guarantees the axes are final in the side stream's order already (the
// orthogonal axes of a pass whose solve_check the side stream has passed).
template <class Ops>
static cel_status check_pass(Ops& ops, int is_col, const std::vector<int32_t>& list, bool wait_main) {
  const Range range(Ops::kRanges.check);
  if (list.empty()) return CEL_OK;
  PassBufs& b = ops.b;
  hipError_t e;
  if (wait_main &&
      ((e = hipEventRecord(b.ev_main, b.main)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess))
    return hip_fail(ops.ctx, e, "event");
  int32_t* idx;
  cel_status st;
  if ((st = upload_list(ops.ctx, b, list, b.side, &idx)) != CEL_OK || (st = fuzz(ops.ctx, b.side)) != CEL_OK) return st;
  return ops.check_complete(is_col, (uint32_t)list.size(), idx);
}

// The pipelined pass schedule of a repair, of one square (SquarePasses, SquareOps) or of a
// merged batch (BatchPasses, BatchOps), over the squares resident at b.eds with the host masks
// hm. `first`: the first row pass by the plan's byte scan. No pass waits for the device; one
// sync at the end, after which b.hroots holds every root of the final squares and b.hflags
// every encoding-check flag, and both streams are idle. plan: built here from plan_args, left
// for the verdicts.
//
// Streams and events. The solve chain (upload of a pass's list, its decode) is the main
// stream's; every encoding check is the side stream's, and its outcome is only read at the
// end, so no check is on the chain's critical path.
// - The masks go up with the first row pass's list riding behind them, and that pass's decode
//   is enqueued before the host builds any bookkeeping (the mask bitsets, the sanity lists),
//   which then runs beside it. The flags are the side stream's (its checks): zeroed there,
//   after ev_main says the masks are up.
// - The sanity checks come next, each after a fresh ev_main (everything the main stream has
//   been given so far); the axes they read are complete from the start and never change.
// - Each pass's encoding check is enqueued after the next pass's decode, so the host's
//   enqueue of it is off the chain. It waits for ev_main as last recorded, the next decode's:
//   later than it needs, and right, since the axes it checks are final from their own pass on.
// - A pass's orthogonal checks follow that pass's own check on the side stream, which has
//   then passed the ev_main that completed them: they wait for nothing more. They are held
//   back (`pending`) until the next decode is enqueued, for the same reason.
// - The last pass's checks go to the side stream ahead of the commit's dozen launches, so they
//   run beside its leaf hashing instead of trailing its tree levels. The main stream then
//   waits for ev_done, the side stream's last check, before the one download of roots and flags.
// - An early return drains the side stream: no check is left running on the ctx's scratch.
template <class Plan, class Ops, class... PlanArgs>
static cel_status run_passes(Ops& ops, const std::vector<uint8_t>& hm, const std::vector<int32_t>& first,
                             std::unique_ptr<Plan>& plan, const PlanArgs&... plan_args) {
  cel_ctx* ctx = ops.ctx;
  PassBufs& b = ops.b;
  const uint32_t W = b.W, n = b.n;
  hipError_t e = hipSuccess;
  cel_status st;
  struct SideDrain {
    hipStream_t side;
    ~SideDrain() { (void)hipStreamSynchronize(side); }
  } drain{b.side};
  std::memcpy(b.hmask, hm.data(), hm.size());
  if (!first.empty()) std::memcpy(b.hlist0, first.data(), first.size() * 4);
  const size_t up_b = (size_t)(reinterpret_cast<uint8_t*>(b.hlist0) - b.hmask) + first.size() * 4;
  if ((e = hipMemcpyAsync(b.mask, b.hmask, up_b, hipMemcpyHostToDevice, b.main)) != hipSuccess ||
      (e = hipEventRecord(b.ev_main, b.main)) != hipSuccess || (e = hipStreamWaitEvent(b.side, b.ev_main, 0)) != hipSuccess ||
      (e = hipMemsetAsync(b.flags, 0, (size_t)n * 2 * W * 4, b.side)) != hipSuccess)
    return hip_fail(ctx, e, "H2D");
  Issued prev;
  if ((st = solve_issue(ops, 0, first, &prev, b.list0)) != CEL_OK) return st;
  bool first_issued = !first.empty();
  {
    const Range plan_range(Ops::kRanges.plan);
    plan.reset(new Plan(plan_args...));
    for (int is_col = 0; is_col < 2; is_col++)
      if ((st = check_pass(ops, is_col, plan->sanity[is_col], true)) != CEL_OK) return st;
  }
  // the checks of the pass `prev`: its own, then the orthogonal axes it completed
  std::vector<int32_t> list, pending;
  auto checks = [&] {
    const cel_status sc = solve_check(ops, prev);
    return sc != CEL_OK ? sc : check_pass(ops, !prev.is_col, pending, false);
  };
  int is_col;
  while (plan->next(&is_col, list)) {
    if (first_issued) {  // the first row pass (the same list, issued above)
      first_issued = false;
    } else {
      Issued s1;
      if ((st = solve_issue(ops, is_col, list, &s1)) != CEL_OK || (st = checks()) != CEL_OK) return st;
      prev = s1;
    }
    // sequential view of the pass: each solve fills its missing cells, completing the
    // orthogonal axes whose last missing cell it held
    const Range fill_range(Ops::kRanges.fill);
    plan->apply(pending);
  }
  if ((st = fuzz(ctx, b.main)) != CEL_OK || (st = checks()) != CEL_OK) return st;
  if ((e = launch_commit(b.eds, W / 2, n, b.roots, b.roots + (size_t)n * W * kNode, nullptr, nullptr, b.work, false,
                         b.main)) != hipSuccess)
    return hip_fail(ctx, e, "roots");
  if ((e = hipEventRecord(b.ev_done, b.side)) != hipSuccess || (e = hipStreamWaitEvent(b.main, b.ev_done, 0)) != hipSuccess)
    return hip_fail(ctx, e, "join");
  if ((e = hipMemcpyAsync(b.hroots, b.roots, b.res_bytes, hipMemcpyDeviceToHost, b.main)) != hipSuccess)
    return hip_fail(ctx, e, "D2H");
  if ((e = hipStreamSynchronize(b.main)) != hipSuccess) return hip_fail(ctx, e, "sync");
  return CEL_OK;
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
  // both streams are idle (run_passes synchronised the joined streams); the square keeps
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

static cel_status repair_bufs(cel_ctx* ctx, uint32_t k, bool own_eds, RepairBufs* b) {
  hipError_t e = hipSuccess;
  b->W = 2 * k;
  if (own_eds) b->eds = static_cast<uint8_t*>(scratch(ctx, S_EDS, (size_t)b->W * b->W * kShare, &e));
  if (!b->eds) return fail(ctx, CEL_ENOMEM, "device allocation failed");
  const cel_status st = carve_bufs(ctx, kSquareSlots, carve_stage, b);
  if (st != CEL_OK) return st;
  b->solves = 0;
  b->ev_side[0] = ctx->ev_repair_side[0];
  b->ev_side[1] = ctx->ev_repair_side[1];
  // no stale record of an earlier call may gate this one: both streams start from here
  if ((e = hipEventRecord(b->ev_side[0], b->side)) != hipSuccess || (e = hipEventRecord(b->ev_side[1], b->side)) != hipSuccess)
    return hip_fail(ctx, e, "event");
  return CEL_OK;
}

// A status a repair ends with for its square, against an error of the call.
static bool is_outcome(cel_status st) {
  return st == CEL_OK || st == CEL_EBYZANTINE || st == CEL_EBADROOT || st == CEL_EUNREPAIRABLE;
}

// One square's verdict after run_passes: its checks replayed in rsmt2d's order (sq.order) over
// its roots (`got`, [2][W] by direction and axis) and flags, the first failure reported. hm:
// the square's host mask, updated: all ones on success, the mask before the failing solve on
// a byzantine / bad-root error, the mask after the last solve when stuck. Root checks are
// deferred: an axis, once complete, never changes, so the commit over the final square gives
// every root rsmt2d checks on the way.
//
// The solves ran in passes (every solvable row, then every solvable column, ...), which
// decodes whole directions at once. When every check passes, the outcome equals that of
// rsmt2d's sweep order (row i, then column i): all cells of the final square then agree
// with valid codewords whose roots match, so any order decodes the same bytes and passes
// the same checks, and the set of axes that can be solved is the same closure. Only a
// failing solve or orthogonal check depends on the order; that square is replayed in
// rsmt2d's order by repair_exact, through b (b.eds: the square).
static cel_status verdict(cel_ctx* ctx, RepairBufs& b, const SquarePasses& sq, const uint8_t* got, const int32_t* flags,
                          const uint8_t* row_roots, const uint8_t* col_roots, std::vector<uint8_t>& hm,
                          const RepairOut& out) {
  const uint8_t* const exp[2] = {row_roots, col_roots};
  cel_status code;
  const long f = first_failure(sq.order.data(), sq.order.size(), {got, kNode, RootRecords::BY_AXIS}, exp, flags, sq.W, &code);
  if (f >= 0) {
    const Check& c = sq.order[(size_t)f];
    if (c.kind == Check::SANITY) return fail_axis(ctx, b, hm, out, code, c.is_col, c.idx, false);
    // a batch's single-square prefix has its pointers, not yet its streams and events
    cel_status st;
    if (!b.main && (st = repair_bufs(ctx, sq.k, false, &b)) != CEL_OK) return st;
    return repair_exact(ctx, b, hm, sq.k, row_roots, col_roots, out);
  }
  if (!sq.solved()) {
    rollback(hm, sq.W, sq.solves, sq.solves.size());
    return fail(ctx, CEL_EUNREPAIRABLE, "failed to solve data square");
  }
  std::fill(hm.begin(), hm.end(), (uint8_t)1);
  return CEL_OK;
}

// rsmt2d Repair over the EDS resident at b.eds, hm = host presence mask (updated as verdict
// leaves it): the plan's first pass, the pass schedule, the verdict.
static cel_status repair_core(cel_ctx* ctx, RepairBufs& b, std::vector<uint8_t>& hm, uint32_t k,
                              const uint8_t* row_roots, const uint8_t* col_roots, const RepairOut& out) {
  SquareOps ops{ctx, b};
  std::unique_ptr<SquarePasses> plan;
  const cel_status st = run_passes(ops, hm, first_row_pass(hm, k), plan, hm.data(), k);
  if (st != CEL_OK) return st;
  return verdict(ctx, b, *plan, b.hroots, b.hflags, row_roots, col_roots, hm, out);
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
  if (!is_outcome(st)) return st;
  if (!d_eds) {  // the (partially) repaired square goes back either way, with the mask it is valid under
    if ((e = hipMemcpyAsync(h_eds, b.eds, eds_b, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(ctx, e, "D2H");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "sync");
  }
  std::memcpy(present, hm.data(), cells);
  return st;
}

// ------------------------------------------------------------ batch of squares
//
// cel_dev_repair_batch: the same schedule over n squares of one k (32, 64, 128: the in-square
// kernels) at once. Every pass is the merged pass of repair_plan.hpp (BatchPasses): one decode
// launch on the main stream and one check launch on the side stream serve every square that
// has axes in it, one commit takes all n squares' roots, and one copy brings the roots and
// flags back. Only the verdict is per square.

// k = 32, 64, 128 and more than one square: the merged schedule; else square after square.
static bool batch_merged(uint32_t k, uint32_t n) {
  return n > 1 && (k == 32 || k == 64 || k == 128) && entries_fit(n, 2 * k);
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
  // Square i ended with st. false: st is an error of the call, not a square's outcome.
  bool record(cel_ctx* ctx, uint32_t i, cel_status st, std::string* first_error) const {
    if (!is_outcome(st)) return false;
    if (st != CEL_OK && first_error->empty()) *first_error = "square " + std::to_string(i) + ": " + ctx->last_error;
    status[i] = st;
    return true;
  }
};

// The squares resident at b.eds, masks hm ([n][W*W] bytes 0 / 1, updated per square as
// repair_core leaves its own). CEL_OK when every square ran to an outcome (out.status).
static cel_status repair_batch_core(cel_ctx* ctx, BatchBufs& b, std::vector<uint8_t>& hm, uint32_t k,
                                    const uint8_t* row_roots, const uint8_t* col_roots, const BatchOut& out,
                                    std::string* first_error) {
  const uint32_t W = 2 * k, n = b.n;
  const size_t cells = (size_t)W * W, roots_b = (size_t)W * kNode;
  BatchOps ops{ctx, b};
  std::unique_ptr<BatchPasses> plan;
  cel_status st = run_passes(ops, hm, first_row_pass_batch(hm, n, k), plan, hm, n, k);
  if (st != CEL_OK) return st;
  // The verdicts, square by square. A replay (repair_exact) reuses the single-square prefix of
  // the slots and of the stage, so the batch's results leave the stage first.
  const std::vector<uint8_t> got_all(b.hroots, b.hroots + 2 * n * roots_b);
  const std::vector<int32_t> flags_all(b.hflags, b.hflags + (size_t)n * 2 * W);
  std::vector<uint8_t> got(2 * roots_b);
  for (uint32_t i = 0; i < n; i++) {
    square_roots(got_all.data(), n, W, i, got.data());
    std::vector<uint8_t> m(hm.begin() + (ptrdiff_t)(i * cells), hm.begin() + (ptrdiff_t)((i + 1) * cells));
    RepairBufs one = b.one;
    one.eds = b.eds + i * cells * kShare;
    st = verdict(ctx, one, plan->sq[i], got.data(), flags_all.data() + (size_t)i * 2 * W, row_roots + i * roots_b,
                 col_roots + i * roots_b, m, out.of(i, W));
    if (!out.record(ctx, i, st, first_error)) return st;
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
      if (!out.record(ctx, i, st, &first_error)) return st;
    }
    if (!first_error.empty()) ctx->last_error = first_error;
    return CEL_OK;
  }
  for (int32_t* bad : {out.bad_axis, out.bad_index})
    if (bad) std::fill(bad, bad + n, -1);
  DeviceGuard g(ctx->device);
  BatchBufs b{};
  b.W = b.one.W = W;
  b.n = n;
  if ((st = carve_bufs(ctx, kBatchSlots, carve_batch_stage, &b)) != CEL_OK) return st;
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

extern "C" {

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
  BatchBufs b{};
  b.W = b.one.W = 2 * k;
  b.n = n;
  return batch_merged(k, n) ? slots_size(kBatchSlots, b) : slots_size(kSquareSlots, b.one);  // else one square at a time
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
