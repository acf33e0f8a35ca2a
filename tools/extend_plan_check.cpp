// Stand-alone host check of the extension paths' planner (celestia-app_amd/csrc/extend_plan.hpp):
// no HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/extend_plan_check.cpp -o extend_plan_check && ./extend_plan_check
// For every k = 1 .. 512 that is a power of two and n = 1 .. 40:
// 1. the device batch's and the host pipeline's chunks partition [0, n) in order, their counts,
//    workspace offsets and slots follow the formulas restated here, and the k = 512 upload's
//    chunks partition [0, k) (k >= kUp);
// 2. ResultBlock's offsets are row roots at 0, column roots behind n * 2k * 90 bytes, the DAHs
//    behind both, the statuses behind n * 32 more and the end 4 n behind that; unpack hands out
//    exactly those bytes and the first status that is not OK.
// For k = 2 .. 64, full and parity-only: a 2k x 2k host map painted from a device map through
// copy_back_rects, for the whole square, the row ranges on the k = 512 upload's chunk boundaries,
// [0, k), [k, 2k), and every rank's column slab at N = 1, 2, 4, 8, against a map filled cell by
// cell: exactly the wanted cells are written, each once, and no Q0 cell under parity-only.
// One line per k with the counts (chunks, squares in the first halves, the sum of the host chunks'
// slots, workspace slots in use, rectangles, cells); tests/test_extend_plan_check.py builds and
// runs it, plain and under ASan + UBSan, and recomputes the counts.
#include <cstdio>
#include <vector>

#include "extend_plan.hpp"

using namespace cel::ext;

static int fails = 0;
static uint32_t cur_k = 0, cur_n = 0;
#define CHECK(c)                                                                                         \
  do {                                                                                                   \
    if (!(c)) {                                                                                          \
      if (fails < 20) std::printf("FAIL %s:%d: %s (k = %u, n = %u)\n", __FILE__, __LINE__, #c, cur_k, cur_n); \
      fails++;                                                                                           \
    }                                                                                                    \
  } while (0)

// a stand-in for the aligned NMT workspace of a chunk: distinct for every (k, cnt)
static size_t work(uint32_t k, uint32_t cnt) { return 256 * ((size_t)k * 64 + cnt); }

struct Counts {
  uint64_t pipe_chunks, first_half, host_chunks, slot_sum, nslots, up_chunks, rects, cells;
};

static void check_plans(uint32_t k, uint32_t n, Counts* cn) {
  const PipePlan p = pipe_plan(k, n, work);
  CHECK(p.nchunks == (n >= 2 ? 2u : 1u) && p.nchunks <= kPipeChunks);
  uint32_t at = 0;
  size_t off = 0;
  for (uint32_t c = 0; c < p.nchunks; c++) {
    CHECK(p.first[c] == at && p.cnt[c] > 0 && p.work_off[c] == off);
    CHECK(p.cnt[c] == (c == 0 ? (n + 1) / 2 : n / 2));
    at += p.cnt[c];
    off += work(k, p.cnt[c]);
  }
  CHECK(at == n && p.work_bytes == off);
  cn->pipe_chunks += p.nchunks;
  cn->first_half += p.cnt[0];

  const HostPlan h = host_plan(n);
  const uint32_t nc = n < 4 ? n : 4, chunk = (n + nc - 1) / nc;
  CHECK(h.n == n && h.chunk == chunk && h.nchunks == (n + chunk - 1) / chunk && h.nchunks <= kHostChunks);
  CHECK(h.nslots == (h.nchunks < 4 ? h.nchunks : 4));
  at = 0;
  for (uint32_t c = 0; c < h.nchunks; c++) {
    CHECK(h.first(c) == at && h.cnt(c) > 0 && h.cnt(c) <= chunk && HostPlan::slot(c) == c % 4);
    CHECK(HostPlan::slot(c) < h.nslots);
    at += h.cnt(c);
    cn->slot_sum += HostPlan::slot(c);
  }
  CHECK(at == n);
  cn->host_chunks += h.nchunks;
  cn->nslots += h.nslots;
}

static void check_results(uint32_t k, uint32_t n) {
  const ResultBlock rb(k, n);
  const size_t roots = (size_t)n * 2 * k * 90;
  CHECK(rb.row_roots() == 0 && rb.col_roots() == roots && rb.dah() == 2 * roots);
  CHECK(rb.status() == 2 * roots + (size_t)n * 32 && rb.bytes() == 2 * roots + (size_t)n * 32 + (size_t)n * 4);
  if (n == 1)  // the literals of the one-square paths
    CHECK(rb.col_roots() == (size_t)2 * k * 90 && rb.dah() == (size_t)2 * 2 * k * 90 && rb.status() == rb.dah() + 32 &&
          rb.bytes() == rb.status() + 4);
  std::vector<uint8_t> h(rb.bytes());
  for (size_t i = 0; i < h.size(); i++) h[i] = (uint8_t)(i * 131 + 7);
  const uint32_t bad = n / 2;  // statuses: OK up to `bad`, then 5, then 9s
  for (uint32_t i = 0; i < n; i++) {
    const int32_t st = i < bad ? 0 : i == bad ? 5 : 9;
    std::memcpy(h.data() + rb.status() + (size_t)i * 4, &st, 4);
  }
  std::vector<uint8_t> rr(roots), cr(roots), dah((size_t)n * 32);
  std::vector<int32_t> st(n);
  CHECK(rb.unpack(h.data(), rr.data(), cr.data(), dah.data(), st.data()) == 5);
  CHECK(std::memcmp(rr.data(), h.data(), roots) == 0 && std::memcmp(cr.data(), h.data() + roots, roots) == 0);
  CHECK(std::memcmp(dah.data(), h.data() + 2 * roots, (size_t)n * 32) == 0);
  CHECK(std::memcmp(st.data(), h.data() + rb.status(), (size_t)n * 4) == 0);
  CHECK(rb.unpack(h.data(), nullptr, nullptr, nullptr, nullptr) == 5);
  std::memset(h.data() + rb.status(), 0, (size_t)n * 4);
  CHECK(rb.unpack(h.data(), nullptr, nullptr, nullptr, nullptr) == 0);
}

// Rows [r0, r1), columns [c0, c0 + w) painted through the rectangles, against the cells wanted.
static void paint(uint32_t k, uint32_t r0, uint32_t r1, bool parity, uint32_t c0, uint32_t w, bool whole_square,
                  Counts* cn) {
  const uint32_t W = 2 * k;
  // the device map: row i, slab column j holds the id of square cell (i, c0 + j)
  std::vector<uint8_t> dev((size_t)W * w), host((size_t)W * W, 0), writes((size_t)W * W, 0);
  auto id = [&](uint32_t i, uint32_t j) { return (uint8_t)(1 + (i * 37 + j * 11) % 251); };
  for (uint32_t i = 0; i < W; i++)
    for (uint32_t j = 0; j < w; j++) dev[(size_t)i * w + j] = id(i, c0 + j);
  const Rects rs = whole_square ? copy_back_rects(k, r0, r1, parity) : copy_back_rects(k, r0, r1, parity, c0, w);
  CHECK(rs.n <= 2);
  uint64_t cells = 0;
  for (uint32_t q = 0; q < rs.n; q++) {
    const Rect& r = rs.r[q];
    CHECK(r.rows > 0 && r.width > 0 && r.width <= r.dst_pitch && r.width <= r.src_pitch);
    CHECK(r.dst_off % kCell == 0 && r.src_off % kCell == 0 && r.width % kCell == 0);
    CHECK(r.dst_pitch == (size_t)W * kCell && r.src_pitch == (size_t)w * kCell);
    if (q == 1) CHECK(rs.r[0].dst_off < r.dst_off);  // the rows above k first
    for (size_t row = 0; row < r.rows; row++)
      for (size_t x = 0; x < r.width / kCell; x++) {
        const size_t d = (r.dst_off + row * r.dst_pitch) / kCell + x, s = (r.src_off + row * r.src_pitch) / kCell + x;
        if (d >= host.size() || s >= dev.size()) {
          CHECK(!"rectangle inside both maps");
          continue;
        }
        host[d] = dev[s];
        writes[d]++;
        cells++;
      }
  }
  uint64_t want_cells = 0;
  for (uint32_t i = 0; i < W; i++)
    for (uint32_t j = 0; j < W; j++) {
      const bool q0 = i < k && j < k;
      const bool want = i >= r0 && i < r1 && j >= c0 && j < c0 + w && !(parity && q0);
      want_cells += want;
      CHECK(writes[(size_t)i * W + j] == (want ? 1 : 0));
      CHECK(host[(size_t)i * W + j] == (want ? id(i, j) : 0));
      if (parity && q0) CHECK(writes[(size_t)i * W + j] == 0);
    }
  CHECK(cells == want_cells);
  if (r0 == 0 && r1 == W && c0 == 0 && w == W) CHECK(cells == (parity ? (uint64_t)3 * k * k : (uint64_t)4 * k * k));
  cn->rects += rs.n;
  cn->cells += cells;
}

static void check_rects(uint32_t k, Counts* cn) {
  const uint32_t W = 2 * k;
  for (int parity = 0; parity < 2; parity++) {
    paint(k, 0, W, parity, 0, W, true, cn);
    paint(k, 0, k, parity, 0, W, true, cn);
    paint(k, k, W, parity, 0, W, true, cn);
    if (k >= kUp)
      for (uint32_t c = 0; c < kUp; c++) paint(k, c * upload_rows(k), (c + 1) * upload_rows(k), parity, 0, W, true, cn);
    for (uint32_t N = 1; N <= 8 && N <= W; N *= 2)
      for (uint32_t rank = 0; rank < N; rank++) paint(k, 0, W, parity, rank * (W / N), W / N, false, cn);
  }
}

int main() {
  for (uint32_t k = 1; k <= 512; k *= 2) {
    Counts cn{};
    cur_k = k;
    for (uint32_t n = 1; n <= 40; n++) {
      cur_n = n;
      check_plans(k, n, &cn);
      check_results(k, n);
    }
    cur_n = 0;
    if (k >= kUp) {
      uint32_t at = 0;
      for (uint32_t c = 0; c < kUp; c++) {
        CHECK(c * upload_rows(k) == at && upload_rows(k) == k / 4);
        at += upload_rows(k);
        cn.up_chunks++;
      }
      CHECK(at == k);
    }
    if (k >= 2 && k <= 64) check_rects(k, &cn);
    std::printf("k = %3u: %llu pipe chunks, %llu in first halves, %llu host chunks, %llu slot sum, %llu slots in use, "
                "%llu upload chunks, %llu rectangles, %llu cells\n",
                k, (unsigned long long)cn.pipe_chunks, (unsigned long long)cn.first_half,
                (unsigned long long)cn.host_chunks, (unsigned long long)cn.slot_sum, (unsigned long long)cn.nslots,
                (unsigned long long)cn.up_chunks, (unsigned long long)cn.rects, (unsigned long long)cn.cells);
  }
  std::printf("extend plan check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
