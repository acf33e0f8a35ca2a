// The extension entry points' host planner (api.cpp, api_block.cpp, api_multi.cpp): everything
// they decide from (k, n, flags, row range) alone. The result block every path brings back,
// the rectangles of an EDS copy-back, and the chunk plans of the two batch pipelines and of
// the k = 512 upload. Plain C++ with no HIP in it: tools/extend_plan_check.cpp includes this
// header alone and walks it on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/celestia_eds.h"

namespace cel {
namespace ext {

constexpr size_t kCell = CEL_SHARE_SIZE, kRoot = CEL_NMT_NODE_SIZE, kDah = 32;

// The results of n squares of width k as one block: row roots | col roots | dah | status, each
// part for all n squares, no padding between or behind them. launch_commit_trees' host_out mode
// stores exactly this block (n = 1), the shard plan's `out` is it, and every host path brings
// it back in one copy. Padding is the caller's: extend_one rounds the size up to the 16-byte
// elements the DAH launch stores, the block path to 256 because the commitments follow.
struct ResultBlock {
  size_t roots;  // bytes of one direction's roots, all squares
  uint32_t n;
  ResultBlock(uint32_t k, uint32_t nsq) : roots((size_t)nsq * 2 * k * kRoot), n(nsq) {}
  size_t row_roots() const { return 0; }
  size_t col_roots() const { return roots; }
  size_t dah() const { return 2 * roots; }
  size_t status() const { return 2 * roots + n * kDah; }
  size_t bytes() const { return status() + (size_t)n * 4; }
  // A host copy of the block into the caller's buffers (each nullable; status_out: n entries).
  // Returns the first status that is not CEL_OK, or CEL_OK.
  int32_t unpack(const void* h, uint8_t* row_roots_out, uint8_t* col_roots_out, uint8_t* dah_out,
                 int32_t* status_out) const {
    const uint8_t* b = static_cast<const uint8_t*>(h);
    if (row_roots_out) std::memcpy(row_roots_out, b + row_roots(), roots);
    if (col_roots_out) std::memcpy(col_roots_out, b + col_roots(), roots);
    if (dah_out) std::memcpy(dah_out, b + dah(), n * kDah);
    int32_t worst = CEL_OK;
    for (uint32_t i = 0; i < n; i++) {
      int32_t st;
      std::memcpy(&st, b + status() + (size_t)i * 4, 4);
      if (status_out) status_out[i] = st;
      if (st != CEL_OK && worst == CEL_OK) worst = st;
    }
    return worst;
  }
};

// One copy of `rows` runs of `width` bytes, pitches apart. A rectangle whose width equals both
// pitches is one contiguous run of width * rows bytes.
struct Rect {
  size_t dst_off, dst_pitch, src_off, src_pitch, width, rows;
  bool contiguous() const { return width == dst_pitch && width == src_pitch; }
};
struct Rects {
  uint32_t n;
  Rect r[2];
};

// The copy-back of rows [r0, r1), columns [c0, c0 + w) of one 2k x 2k EDS into a row-major
// host square (pitch 2k cells), from a device buffer that holds those w columns of every row
// (pitch w cells): the whole square (c0 = 0, w = 2k) or a rank's column slab. At most two
// rectangles, the rows above k first. With parity_only no Q0 cell is written: the upper
// rectangle starts at column max(c0, k) and is dropped when nothing is left of it (Q1 is one
// strided copy, Q2|Q3 stay whole rows).
inline Rects copy_back_rects(uint32_t k, uint32_t r0, uint32_t r1, bool parity_only, uint32_t c0, uint32_t w) {
  const size_t rowb = (size_t)2 * k * kCell, slabb = (size_t)w * kCell;
  const uint32_t t0 = parity_only ? std::max(c0, k) : c0;  // first column of the upper rectangle
  const uint32_t top1 = std::min(r1, k), bot0 = std::max(r0, k);
  Rects out{};
  if (r0 < top1 && t0 < c0 + w)
    out.r[out.n++] = {r0 * rowb + t0 * kCell, rowb, r0 * slabb + (t0 - c0) * kCell, slabb, (c0 + w - t0) * kCell,
                      top1 - r0};
  if (bot0 < r1) out.r[out.n++] = {bot0 * rowb + c0 * kCell, rowb, bot0 * slabb, slabb, slabb, r1 - bot0};
  return out;
}
inline Rects copy_back_rects(uint32_t k, uint32_t r0, uint32_t r1, bool parity_only) {
  return copy_back_rects(k, r0, r1, parity_only, 0, 2 * k);
}

// Chunking of a device batch over the internal streams: chunk c runs RS extension then NMT +
// DAH on stream sub[c]; the chunks start together, so one chunk's latency-bound tree top + DAH
// runs beside the other's work. Two chunks (profiles/r1g_pipe_chunks_ab.txt); chaining the
// extensions so each runs beside the previous chunk's hashing buys nothing, the step is the sum
// of the two VALU-bound phases (profiles/r2_pipe_overlap_ab.txt). Equal halves: uneven splits
// (5/8 .. 7/8 of the batch in the first chunk, so the small chunk's tree top would run under
// the large chunk's bulk) measured slower at both k=64 B=128 and k=128 B=256
// (profiles/r4_pipe_split_ab.txt).
constexpr uint32_t kPipeChunks = 2;

struct PipePlan {
  uint32_t nchunks;
  uint32_t first[kPipeChunks], cnt[kPipeChunks];
  size_t work_off[kPipeChunks], work_bytes;  // NMT workspace of each chunk
};

// work(k, cnt): the aligned NMT workspace of a chunk of cnt squares (the kernels' own figure).
inline PipePlan pipe_plan(uint32_t k, uint32_t n, size_t (*work)(uint32_t k, uint32_t cnt)) {
  PipePlan p{};
  const uint32_t c0 = (n + 1) / 2;
  p.nchunks = c0 < n ? 2 : 1;
  p.cnt[0] = c0;
  p.first[1] = c0;
  p.cnt[1] = n - c0;
  for (uint32_t c = 0; c < p.nchunks; c++) {
    p.work_off[c] = p.work_bytes;
    p.work_bytes += work(k, p.cnt[c]);
  }
  return p;
}

// Chunks of the host-buffer pipeline: the upload of chunk c + 1, the compute of chunk c and the
// copy-back of chunk c - 1 overlap (profiles/r1c_host_io.txt). Chunk c runs on internal stream
// and workspace slot c % kPipeStreams; with kHostChunks <= kPipeStreams that is c itself.
constexpr uint32_t kHostChunks = 4;
constexpr uint32_t kPipeStreams = 4;  // the ctx's internal streams
static_assert(kHostChunks <= kPipeStreams && kPipeChunks <= kPipeStreams, "one stream per chunk in flight");

struct HostPlan {
  uint32_t n, chunk, nchunks, nslots;  // squares, squares per chunk, chunks, workspace slots in use
  uint32_t first(uint32_t c) const { return c * chunk; }
  uint32_t cnt(uint32_t c) const { return std::min(chunk, n - first(c)); }
  static uint32_t slot(uint32_t c) { return c % kPipeStreams; }
};

inline HostPlan host_plan(uint32_t n) {
  const uint32_t nc = std::min(n, kHostChunks);
  const uint32_t chunk = (n + nc - 1) / nc, nchunks = (n + chunk - 1) / chunk;
  return {n, chunk, nchunks, std::min(nchunks, kPipeStreams)};
}

// One k = 512 square from page-locked memory crosses PCIe in kUp chunks of k / kUp ODS rows.
constexpr uint32_t kUp = 4;
inline uint32_t upload_rows(uint32_t k) { return k / kUp; }

}  // namespace ext
}  // namespace cel
