// Stand-alone host check of the square layout (celestia-app_amd/csrc/square.cpp,
// cel_square_layout): no HIP, no device. Build it with a host compiler, optionally under
// sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/square_layout_check.cpp celestia-app_amd/csrc/square.cpp -o square_layout_check \
//       && ./square_layout_check
// It builds random and edge blocks (normal txs, BlobTx protobufs, blobs at every share
// boundary, empty blocks, blocks that overflow the square, misordered blocks), expands each
// layout's segments and compact shares into bytes here, and compares them with
// cel_square_construct's square, status, k, included[] and error text, in exactly sized
// buffers. The last line is a digest of everything compared, equal in every build.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/celestia_eds.h"

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      fails++;                                                      \
    }                                                               \
  } while (0)

using Bytes = std::vector<uint8_t>;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 24;
}
static Bytes rnd_bytes(size_t n) {
  Bytes b(n);
  for (uint8_t& x : b) x = (uint8_t)rnd();
  return b;
}
static void put_uvarint(Bytes& o, uint64_t v) {
  while (v >= 0x80) {
    o.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
}
static void put_field(Bytes& o, uint32_t num, const Bytes& d) {
  put_uvarint(o, num << 3 | 2);
  put_uvarint(o, d.size());
  o.insert(o.end(), d.begin(), d.end());
}
// BlobTx {1: tx, 2: repeated Blob {1: namespace_id, 2: data, 3: share_version}, 3: "BLOB"}
static Bytes blob_tx(size_t inner, const std::vector<size_t>& blob_lens, uint32_t share_version = 0) {
  Bytes tx;
  put_field(tx, 1, rnd_bytes(inner));
  for (size_t n : blob_lens) {
    Bytes ns(28, 0), m;
    for (int i = 18; i < 28; i++) ns[i] = (uint8_t)rnd();
    put_field(m, 1, ns);
    put_field(m, 2, rnd_bytes(n));
    if (share_version) {
      put_uvarint(m, 3 << 3);
      put_uvarint(m, share_version);
    }
    put_field(tx, 2, m);
  }
  put_field(tx, 3, Bytes{'B', 'L', 'O', 'B'});
  return tx;
}

static uint64_t digest = 1469598103934665603ull;  // FNV-1a over everything compared
static void mix(const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; i++) digest = (digest ^ b[i]) * 1099511628211ull;
}

static uint32_t sparse_shares(uint64_t len) { return len == 0 ? 0 : len <= 478 ? 1 : 1 + (uint32_t)((len - 478 + 481) / 482); }

static void check_block(const std::vector<Bytes>& txs, uint32_t max_square_size, uint32_t greedy) {
  Bytes raw;  // exactly the txs' bytes: a read past them is a sanitizer finding
  std::vector<uint32_t> lens;
  for (const Bytes& t : txs) {
    raw.insert(raw.end(), t.begin(), t.end());
    lens.push_back((uint32_t)t.size());
  }
  const uint32_t ntx = (uint32_t)txs.size();
  const uint8_t* p = ntx ? raw.data() : nullptr;
  const uint32_t* l = ntx ? lens.data() : nullptr;
  std::vector<uint8_t> inc_c(ntx + 1, 9), inc_l(ntx + 1, 9);
  uint32_t k_c = 0, k_l = 0, nseg = 0, ncomp = 0;
  const cel_status st_c = cel_square_construct(p, l, ntx, max_square_size, 64, greedy, nullptr, 0, &k_c, inc_c.data());
  const std::string err_c = cel_square_last_error();
  const cel_status st_l =
      cel_square_layout(p, l, ntx, max_square_size, 64, greedy, &k_l, inc_l.data(), nullptr, 0, &nseg, nullptr, 0, &ncomp);
  const std::string err_l = cel_square_last_error();
  CHECK(st_c == st_l && err_c == err_l && inc_c == inc_l);
  mix(&st_c, sizeof st_c);
  mix(err_c.data(), err_c.size());
  mix(inc_c.data(), ntx);
  if (st_c != CEL_OK) return;
  CHECK(k_c == k_l && k_c <= max_square_size);
  const size_t n = (size_t)k_c * k_c;
  Bytes want(n * 512), got(n * 512, 0xEE), compact((size_t)ncomp * 512);
  std::vector<cel_square_segment> segs(nseg);
  CHECK(cel_square_construct(p, l, ntx, max_square_size, 64, greedy, want.data(), (uint32_t)n, &k_c, nullptr) == CEL_OK);
  uint32_t nseg2 = 0, ncomp2 = 0;
  CHECK(cel_square_layout(p, l, ntx, max_square_size, 64, greedy, &k_l, nullptr, segs.data(), nseg, &nseg2,
                          compact.data(), ncomp, &ncomp2) == CEL_OK);
  CHECK(nseg2 == nseg && ncomp2 == ncomp && nseg > 0);
  uint64_t at = 0;
  for (const cel_square_segment& s : segs) {
    CHECK(s.start == at && s.count > 0 && at + s.count <= n);
    if (s.start != at || at + s.count > n) return;
    uint8_t* dst = got.data() + (size_t)s.start * 512;
    if (s.kind == CEL_SEG_COMPACT) {
      CHECK(s.off + s.count <= ncomp);
      if (s.off + s.count <= ncomp) std::memcpy(dst, compact.data() + s.off * 512, (size_t)s.count * 512);
    } else if (s.kind == CEL_SEG_PAD) {
      std::memset(dst, 0, (size_t)s.count * 512);
      for (uint32_t j = 0; j < s.count; j++) {
        std::memcpy(dst + (size_t)j * 512, s.ns, 29);
        dst[(size_t)j * 512 + 29] = 1;
      }
    } else {
      CHECK(s.kind == CEL_SEG_BLOB && s.len > 0 && s.count == sparse_shares(s.len));
      CHECK(s.off + s.len <= raw.size() && s.tx_index < ntx && inc_l[s.tx_index] == 2);
      if (s.kind != CEL_SEG_BLOB || s.off + s.len > raw.size() || s.count != sparse_shares(s.len)) return;
      std::memset(dst, 0, (size_t)s.count * 512);
      for (uint32_t j = 0; j < s.count; j++) {
        uint8_t* sh = dst + (size_t)j * 512;
        std::memcpy(sh, s.ns, 29);
        sh[29] = (uint8_t)((s.share_version << 1) | (j == 0));
        const uint64_t from = j == 0 ? 0 : 478 + 482ull * (j - 1);
        const uint32_t header = j == 0 ? 34 : 30;
        if (j == 0) {
          sh[30] = (uint8_t)(s.len >> 24), sh[31] = (uint8_t)(s.len >> 16);
          sh[32] = (uint8_t)(s.len >> 8), sh[33] = (uint8_t)s.len;
        }
        const uint64_t take = std::min<uint64_t>(512 - header, s.len - from);
        std::memcpy(sh + header, raw.data() + s.off + from, take);
      }
    }
    at += s.count;
  }
  CHECK(at == n);
  CHECK(got == want);
  mix(&k_c, sizeof k_c);
  mix(want.data(), want.size());
  mix(segs.data(), segs.size() * sizeof(cel_square_segment));
}

static std::vector<Bytes> random_block(uint32_t normal, uint32_t blob_txs, size_t max_blob) {
  std::vector<Bytes> txs;
  for (uint32_t i = 0; i < normal; i++) txs.push_back(rnd_bytes(40 + rnd() % 660));
  for (uint32_t i = 0; i < blob_txs; i++) {
    std::vector<size_t> lens(1 + rnd() % 3);
    for (size_t& n : lens) n = 1 + rnd() % max_blob;
    txs.push_back(blob_tx(150 + rnd() % 250, lens));
  }
  return txs;
}

int main() {
  static_assert(sizeof(cel_square_segment) == 64, "segment record");
  for (uint32_t greedy = 0; greedy < 2; greedy++) {
    check_block({}, 128, greedy);                       // the empty square
    check_block(random_block(5, 0, 1), 128, greedy);    // no blobs
    check_block(random_block(0, 6, 6000), 128, greedy); // no normal txs
    check_block(random_block(3, 4, 60000), 128, greedy);
    check_block(random_block(4, 30, 3000), 8, greedy);  // overflows an 8 x 8 square
    check_block(random_block(300, 2, 2000), 128, greedy);
    check_block(random_block(1, 1, 1), 1, greedy);      // nothing fits a 1 x 1 square but one share
    // every share boundary, in one tx and one per tx
    const std::vector<size_t> edges = {1, 477, 478, 479, 959, 960, 961, 1442, 1443, 6000, 40000, 31000, 2, 70000};
    for (size_t inner = 200; inner < 204; inner++) {
      std::vector<Bytes> txs = random_block(3, 0, 1);
      txs.push_back(blob_tx(inner, edges));
      check_block(txs, 128, greedy);
    }
    {
      std::vector<Bytes> txs;
      for (size_t n : edges) txs.push_back(blob_tx(160, {n}));
      check_block(txs, 128, greedy);
    }
    {  // a normal tx after a blob tx; a blob of share version 1; a blob tx whose blob is empty
      std::vector<Bytes> txs = random_block(2, 1, 5000);
      txs.push_back(rnd_bytes(300));
      check_block(txs, 128, greedy);
      check_block({rnd_bytes(100), blob_tx(170, {1500}, 1)}, 128, greedy);
      check_block({blob_tx(170, {0, 700})}, 128, greedy);
    }
    check_block({blob_tx(200, {1u << 20}), blob_tx(201, {(1u << 20) + 1})}, 256, greedy);  // k = 64
    for (int i = 0; i < 40; i++)
      check_block(random_block((uint32_t)(rnd() % 20), (uint32_t)(rnd() % 12), 1 + rnd() % 20000),
                  1u << (rnd() % 8), greedy);
  }
  std::printf(fails ? "square layout check: %d failures\n" : "square layout check: ok\n", fails);
  std::printf("%016llx\n", (unsigned long long)digest);
  return fails ? 1 : 0;
}
