// Stand-alone host check of the batch tree index's arithmetic
// (celestia-app_amd/csrc/nmt_prove.hpp and nmt_namespace.hpp): no HIP, no device. Build it with
// a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/index_batch_check.cpp -o index_batch_check && ./index_batch_check
// The batch index is n single-square indexes back to back. The kernels that build it and read
// it (k_leaf_index, k_level_index, k_merkle_index, k_prove_squares, k_ns_*_squares) add a
// 64-bit slice base to what the single-square kernels compute; this walks those sums.
// 1. For k = 1, 2, 4 .. 64 and n = 1 .. 5, every square sq < n: the closed forms (index_records,
//    index_bytes, the tail offsets) equal index_layout's; every (axis, tree, level, position)
//    lands, through slice_base + index_record * 96, inside level l of slice sq and nowhere
//    else (a table of exactly n * index_bytes / 16 marks: every leaf record named twice, every
//    other record once, every tail part once, no mark twice across squares); the level kernel's
//    own address (slice_level_off + node * 96) is that same byte; every request's cell lies in
//    square sq of the n squares' cells.
// 2. One shape whose offsets pass 2^32, k = 128 with n = 300: the last record, the tail and the
//    last cell of square 299, in 64-bit against a sum taken slice by slice.
// 3. The (square, namespace) query row and the entry's packed square round-trip for every
//    square a call takes, and the namespace's compare bytes stay as they were.
// tests/test_index_batch_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nmt_namespace.hpp"
#include "nmt_prove.hpp"

using namespace cel::prove;
namespace nsq = cel::nsq;

static int fails = 0;
#define CHECK(c)                                                                                          \
  do {                                                                                                    \
    if (!(c)) {                                                                                           \
      if (fails < 20) std::printf("FAIL %s:%d: %s (k = %u, n = %u, sq = %u)\n", __FILE__, __LINE__, #c, k, n, sq); \
      fails++;                                                                                            \
    }                                                                                                     \
  } while (0)

// Marks of 16 bytes each over n * index_bytes: how often each piece of the batch index is named.
static void check_batch(uint32_t k, uint32_t n) {
  const IndexLayout x = index_layout(k);
  const uint32_t W = 2 * k;
  uint32_t sq = 0;
  CHECK(index_records(W) == x.records);
  CHECK(index_bytes(W) == x.bytes && x.bytes % 16 == 0);
  CHECK(slice_leafd_off(W) == x.leafd_off && slice_dah_off(W) == x.dah_off);
  CHECK(slice_bad_off(W) == x.bad_off && slice_status_off(W) == x.status_off);
  for (uint32_t l = 0; l <= x.L; l++) CHECK(slice_level_off(W, l) == x.level_off[l]);
  const uint64_t total = (uint64_t)n * x.bytes, cells_total = (uint64_t)n * W * W * 512;
  std::vector<uint8_t> marks(total / 16, 0);  // exactly the batch index: a mark outside is out of bounds
  auto mark = [&](uint64_t byte, uint64_t len) {
    CHECK(byte % 16 == 0 && len % 16 == 0 && byte + len <= total);
    if (byte % 16 == 0 && byte + len <= total)
      for (uint64_t i = byte / 16; i < (byte + len) / 16; i++) marks[i]++;
  };
  for (sq = 0; sq < n; sq++) {
    const uint64_t base = slice_base(W, sq);
    CHECK(base == (uint64_t)sq * x.bytes && base % 16 == 0);
    CHECK(eds_base(W, sq) == (uint64_t)sq * W * W * 512);
    for (uint32_t axis = 0; axis < 2; axis++)
      for (uint32_t t = 0; t < W; t++)
        for (uint32_t l = 0; l <= x.L; l++)
          for (uint32_t p = 0; p < (W >> l); p++) {
            const uint64_t r = index_record(W, axis, t, l, p);
            const uint64_t byte = base + r * kRecordBytes;
            CHECK(r < x.records && r <= 0xFFFFFFFFull);  // a record number inside a square stays 32-bit
            CHECK(byte >= base + x.level_off[l]);
            CHECK(byte + kRecordBytes <= base + (l == x.L ? x.leafd_off : x.level_off[l + 1]));
            // the build's own address: the leaf kernel's cell, the level kernel's node
            const uint64_t node = l == 0 ? request_cell(W, axis, t, p) : (uint64_t)(axis ? W + t : t) * (W >> l) + p;
            CHECK(byte == base + slice_level_off(W, l) + node * kRecordBytes);
            mark(byte, kRecordBytes);
            if (l == 0) {  // the share of that leaf
              const uint64_t cell = request_cell(W, axis, t, p);
              CHECK(cell < (uint64_t)W * W);
              CHECK(cell == (axis ? (uint64_t)p * W + t : (uint64_t)t * W + p));
              CHECK(eds_base(W, sq) + (cell + 1) * 512 <= cells_total);
              CHECK(eds_base(W, sq) + cell * 512 >= (uint64_t)sq * W * W * 512);
              CHECK(eds_base(W, sq) + (cell + 1) * 512 <= (uint64_t)(sq + 1) * W * W * 512);
            }
          }
    mark(base + slice_leafd_off(W), (uint64_t)2 * W * 32);
    mark(base + slice_dah_off(W), 32);
    mark(base + slice_bad_off(W), 16);  // flag, status and the padding
    CHECK(slice_status_off(W) + 4 <= x.bytes);
  }
  for (sq = 0; sq < n; sq++)
    for (uint64_t i = 0; i < x.bytes / 16; i++) {
      const uint64_t off = i * 16;
      const uint8_t want = off < (uint64_t)W * W * kRecordBytes ? 2 : 1;  // a leaf: by row and by column
      CHECK(marks[((uint64_t)sq * x.bytes) / 16 + i] == want);
    }
}

// k = 128, n = 300: 5.6 GB of index and 39 GB of cells. The bases against a running sum.
static void check_large() {
  const uint32_t k = 128, n = 300, W = 2 * k;
  uint32_t sq = n - 1;
  const IndexLayout x = index_layout(k);
  uint64_t base = 0, cells = 0;
  for (uint32_t i = 0; i < sq; i++) {
    base += x.bytes;
    cells += (uint64_t)W * W * 512;
  }
  CHECK(slice_base(W, sq) == base && eds_base(W, sq) == cells);
  CHECK(base > 0xFFFFFFFFull && cells > 0xFFFFFFFFull);
  CHECK((uint32_t)base != base);  // a 32-bit base would have wrapped
  // the last record: the root of the last column tree
  const uint64_t last = index_record(W, 1, W - 1, x.L, 0);
  CHECK(last == x.records - 1 && last <= 0xFFFFFFFFull);
  CHECK(slice_base(W, sq) + (last + 1) * kRecordBytes == base + x.leafd_off);
  CHECK(slice_base(W, sq) + slice_status_off(W) + 4 <= (uint64_t)n * x.bytes);
  CHECK(slice_base(W, sq) + index_bytes(W) == (uint64_t)n * x.bytes);
  // the last cell, by its row and by its column
  const uint64_t cell = request_cell(W, 0, W - 1, W - 1);
  CHECK(cell == request_cell(W, 1, W - 1, W - 1) && cell == (uint64_t)W * W - 1);
  CHECK(eds_base(W, sq) + (cell + 1) * 512 == (uint64_t)n * W * W * 512);
  std::printf("k = %u, n = %u: square %u at index byte %llu, cell byte %llu\n", k, n, sq, (unsigned long long)base,
              (unsigned long long)cells);
}

static void check_queries() {
  const uint32_t k = 0, n = 0;
  uint32_t sq = 0;
  uint8_t ns[29], row[32];
  for (uint32_t j = 0; j < 29; j++) ns[j] = (uint8_t)(0xA0 + j);
  static_assert(kMaxSquares < nsq::kMaxPlanSquares, "a call's squares fit the query row");
  for (sq = 0; sq <= kMaxSquares; sq += (sq < 1024 ? 1 : 257)) {
    std::memset(row, 0xEE, sizeof row);
    nsq::query_row(row, ns, sq);
    CHECK(std::memcmp(row, ns, 29) == 0);
    uint32_t w7;
    std::memcpy(&w7, row + 28, 4);  // little-endian, as the device reads it
    CHECK(nsq::query_square(w7) == sq);
    CHECK((w7 << 24) == ((uint32_t)ns[28] << 24));  // the find kernel's compare word drops the square
    for (uint32_t kind = 0; kind < 2; kind++) {
      const uint32_t packed = nsq::entry_pack(kind, sq);
      CHECK(nsq::entry_kind(packed) == kind && nsq::entry_square(packed) == sq);
      CHECK((uint8_t)packed == kind);  // what the plan call hands the caller
    }
  }
  CHECK(nsq::entry_pack(nsq::kAbsence, 0) == nsq::kAbsence && nsq::entry_pack(nsq::kInclusion, 0) == nsq::kInclusion);
  std::printf("queries: squares 0 .. %u round-trip\n", kMaxSquares);
}

int main() {
  for (uint32_t k = 1; k <= 64; k *= 2)
    for (uint32_t n = 1; n <= 5; n++) {
      check_batch(k, n);
      std::printf("k = %2u, n = %u: %llu bytes\n", k, n, (unsigned long long)((uint64_t)n * index_bytes(2 * k)));
    }
  check_large();
  check_queries();
  std::printf("index batch check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
