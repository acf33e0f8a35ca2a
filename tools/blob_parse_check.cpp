// Stand-alone host check of the blob parser's arithmetic (celestia-app_amd/csrc/blob_parse.hpp):
// no HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/blob_parse_check.cpp -o blob_parse_check && ./blob_parse_check
// 1. bparse::walk_status against parseSparseShares' walk, share after share, for every sequence
//    of up to 8 share classes; bparse::classify over every info byte and padding kind.
// 2. bparse::is_short at every length around a share boundary and at 0xFFFFFFFF.
// 3. bparse::chunk_pieces: for blobs of the edge lengths every 16-byte chunk is cut into pieces
//    that take each byte below the length exactly once from the share and share byte a walk of
//    the blob puts it at; the five aligned dwords a piece reads lie inside the 512-byte cell
//    or are left out (index above 127), and every dword that holds a byte taken is read.
// 4. bparse::ranges_error on good and bad ranges; range_offsets / range_of over ranges with
//    empty ones among them; blob_of over offsets of padded lengths.
// 5. bparse::carve: the regions follow one another without overlap, sized for the worst case
//    (a blob per share), and the null base gives the same size.
// tests/test_blob_parse_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "blob_parse.hpp"

using namespace cel;
using namespace cel::bparse;

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      if (fails < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fails++;                                                            \
    }                                                                     \
  } while (0)

// parseSparseShares' first loop over classes: the status it ends with.
static uint32_t walk(const std::vector<uint32_t>& cls) {
  bool open = false;
  for (uint32_t c : cls) {
    if (c == kBadVer) return kEVersion;
    if (c == kPad) continue;
    if (c == kStart) open = true;
    else if (!open) return kENoStart;
  }
  return kOk;
}

static uint64_t check_walk() {
  uint64_t n = 0;
  for (uint32_t len = 0; len <= 8; len++)
    for (uint32_t code = 0; code < (1u << (2 * len)); code++) {
      std::vector<uint32_t> cls(len);
      uint32_t nsig = 0, nbad = 0, first = kPad;
      for (uint32_t i = 0; i < len; i++) {
        cls[i] = (code >> (2 * i)) & 3u;
        if (cls[i] != kPad && !nsig++) first = cls[i];
        if (cls[i] == kBadVer) nbad++;
      }
      CHECK(walk_status(nsig, first, nbad) == walk(cls));
      n++;
    }
  for (uint32_t info = 0; info < 256; info++)
    for (int pad = 0; pad < 3; pad++)
      for (uint32_t len : {0u, 1u, 0xFFFFFFFFu}) {
        const uint32_t c = classify(info, pad == 1, pad == 2, len);
        const uint32_t want = (info >> 1) ? kBadVer : pad ? kPad : (info & 1) ? (len ? kStart : kPad) : kCont;
        CHECK(c == want);
      }
  return n;
}

static uint64_t check_short() {
  uint64_t n = 0;
  for (uint32_t shares = 1; shares <= 40; shares++) {
    const uint64_t holds = blob::kSparseFirst + (uint64_t)blob::kSparseCont * (shares - 1);
    for (int64_t d = -2; d <= 2; d++) {
      const uint64_t len = holds + d;
      if (len == 0 || len > 0xFFFFFFFFull) continue;
      CHECK(is_short((uint32_t)len, shares) == (len > holds));
      CHECK(blob::sparse_shares_needed(len) == (len > holds ? shares + 1 : shares));  // is_short agrees with the planner
      n++;
    }
  }
  CHECK(is_short(0xFFFFFFFFu, 1) && is_short(0xFFFFFFFFu, 1u << 18) && is_short(0xFFFFFFFFu, 8910720u));
  CHECK(!is_short(0xFFFFFFFFu, 8910721u));
  CHECK(!is_short(1, 1) && !is_short(478, 1) && is_short(479, 1) && !is_short(479, 2) && !is_short(1, 1000));
  CHECK(pad16(0) == 0 && pad16(1) == 16 && pad16(16) == 16 && pad16(17) == 32 && pad16(0xFFFFFFFFull) == 0x100000000ull);
  return n;
}

// Byte x of a blob by a walk of its shares: (share, share byte).
static void place(uint32_t x, uint32_t& j, uint32_t& q) {
  if (x < blob::kSparseFirst) {
    j = 0;
    q = kFirstHdr + x;
    return;
  }
  j = 1;
  x -= blob::kSparseFirst;
  while (x >= blob::kSparseCont) {
    x -= blob::kSparseCont;
    j++;
  }
  q = kContHdr + x;
}

static uint64_t check_chunks() {
  uint64_t chunks = 0;
  for (uint32_t len : {1u, 15u, 16u, 17u, 477u, 478u, 479u, 480u, 481u, 959u, 960u, 961u, 1442u, 1443u, 6000u, 70000u}) {
    std::vector<uint8_t> taken(len, 0);
    for (uint32_t o = 0; o < len; o += 16) {
      Piece pc[2];
      chunk_pieces(o, len, pc[0], pc[1]);
      chunks++;
      CHECK(pc[0].lo == 0 && pc[0].hi > 0 && pc[0].hi <= 16);
      CHECK(pc[1].lo == pc[1].hi || (pc[1].lo == pc[0].hi && pc[1].hi <= 16 && pc[1].j == pc[0].j + 1));
      for (const Piece& p : pc) {
        if (p.lo >= p.hi) continue;
        CHECK(p.q >= 15 && p.q + p.hi <= 512);
        const uint32_t w0 = p.q >> 2;
        for (uint32_t t = p.lo; t < p.hi; t++) {
          uint32_t j, q;
          place(o + t, j, q);
          CHECK(j == p.j && q == p.q + t);
          CHECK(o + t < len && !taken[o + t]++);
          const uint32_t w = (p.q + t) >> 2;  // the dword the byte lies in: one of the five, inside the cell
          CHECK(w >= w0 && w <= w0 + 4 && w <= 127);
        }
      }
      const uint32_t last = pc[1].lo < pc[1].hi ? pc[1].hi : pc[0].hi;
      CHECK(o + last == (o + 16 < len ? o + 16 : len));
    }
    for (uint8_t v : taken) CHECK(v == 1);
  }
  return chunks;
}

static uint64_t check_ranges() {
  uint64_t total = 0, n = 0;
  const uint32_t s0[] = {0, 5, 5, 16, 3}, e0[] = {4, 5, 9, 16, 16};
  CHECK(ranges_error(4, 5, s0, e0, &total).empty() && total == 4 + 0 + 4 + 0 + 13);
  uint32_t roff[6];
  range_offsets(5, s0, e0, roff);
  CHECK(roff[0] == 0 && roff[1] == 4 && roff[2] == 4 && roff[3] == 8 && roff[4] == 8 && roff[5] == 21);
  for (uint32_t p = 0; p < 21; p++) {
    const uint32_t r = range_of(roff, 5, p);
    CHECK(r < 5 && roff[r] <= p && p < roff[r + 1] && s0[r] + (p - roff[r]) < e0[r]);
    n++;
  }
  const uint32_t s1[] = {3}, e1[] = {2}, e2[] = {17};
  CHECK(!ranges_error(4, 1, s1, e1, &total).empty());
  CHECK(!ranges_error(4, 1, s1, e2, &total).empty());
  CHECK(!ranges_error(3, 0, nullptr, nullptr, &total).empty() && !ranges_error(0, 0, nullptr, nullptr, &total).empty());
  CHECK(!ranges_error(1024, 0, nullptr, nullptr, &total).empty());
  CHECK(!ranges_error(4, 1, nullptr, e2, &total).empty());
  CHECK(ranges_error(512, 0, nullptr, nullptr, &total).empty() && total == 0);
  CHECK(ranges_error(1, 1, s0, e0 + 1, &total).empty() == false);  // end 5 > 1
  {
    // 8192 whole squares of k = 512 are 2^31 shares: one too many; 8191 pass
    std::vector<uint32_t> s(8192, 0), e(8192, 512u * 512u);
    CHECK(!ranges_error(512, 8192, s.data(), e.data(), &total).empty());
    CHECK(ranges_error(512, 8191, s.data(), e.data(), &total).empty() && total == 8191ull << 18);
  }
  std::vector<uint64_t> doff{0};
  for (uint32_t len : {1u, 16u, 17u, 478u, 70000u, 2u}) doff.push_back(doff.back() + pad16(len));
  for (uint64_t at = 0; at < doff.back(); at += 16) {
    const uint32_t b = blob_of(doff.data(), (uint32_t)doff.size() - 1, at);
    CHECK(doff[b] <= at && at < doff[b + 1]);
    n++;
  }
  return n;
}

static uint64_t check_carve() {
  uint64_t n = 0;
  for (uint64_t total : {0ull, 1ull, 255ull, 256ull, 257ull, 16384ull, 262144ull})
    for (uint32_t nr : {1u, 2u, 1024u}) {
      std::vector<uint8_t> base(16);
      const Work w = carve(base.data(), total, nr);  // the pointers are compared, never followed
      const Work z = carve(nullptr, total, nr);
      CHECK(z.bytes == w.bytes && !z.head && !z.recs && !z.rstart);
      const uint8_t* b = base.data();
      const uint8_t* at[] = {reinterpret_cast<uint8_t*>(w.head), reinterpret_cast<uint8_t*>(w.recs),
                             reinterpret_cast<uint8_t*>(w.doff), reinterpret_cast<uint8_t*>(w.first),
                             reinterpret_cast<uint8_t*>(w.roff), reinterpret_cast<uint8_t*>(w.range_short),
                             reinterpret_cast<uint8_t*>(w.range_status), reinterpret_cast<uint8_t*>(w.cls),
                             reinterpret_cast<uint8_t*>(w.pre), reinterpret_cast<uint8_t*>(w.src),
                             reinterpret_cast<uint8_t*>(w.cand), reinterpret_cast<uint8_t*>(w.sums1),
                             reinterpret_cast<uint8_t*>(w.sums2), b + w.bytes};
      const size_t need[] = {sizeof(Head), total * sizeof(cel_blob_rec), (total + 1) * 8, total * 4,
                             (2 * (size_t)nr + 1) * 4, (size_t)nr * 4, (size_t)nr * 4, total * sizeof(Class),
                             (total + 1) * sizeof(Pre), total * 4, total * sizeof(Cand), w.blocks * sizeof(Pre),
                             w.blocks * sizeof(BlobSums)};
      CHECK(at[0] == b && at[1] == b + kRecOff);
      for (int i = 0; i < 13; i++) {
        CHECK(at[i + 1] >= at[i] + need[i]);
        CHECK((at[i] - b) % 256 == 0);
      }
      CHECK(reinterpret_cast<uint8_t*>(w.rstart) == reinterpret_cast<uint8_t*>(w.roff) + ((size_t)nr + 1) * 4);
      CHECK(w.blocks >= 1 && w.blocks * kScanBlock >= total && w.total == total);
      n++;
    }
  CHECK(sizeof(cel_blob_rec) == 64 && sizeof(Cand) == 24 && sizeof(Pre) == 12 && sizeof(BlobSums) == 24);
  return n;
}

int main() {
  std::printf("walk: %llu sequences\n", (unsigned long long)check_walk());
  std::printf("short: %llu lengths\n", (unsigned long long)check_short());
  std::printf("chunks: %llu\n", (unsigned long long)check_chunks());
  std::printf("ranges: %llu positions\n", (unsigned long long)check_ranges());
  std::printf("carve: %llu workspaces\n", (unsigned long long)check_carve());
  std::printf("blob parse check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
