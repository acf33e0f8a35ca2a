// Stand-alone host check of the tx parser's arithmetic (celestia-app_amd/csrc/tx_parse.hpp): no
// HIP, no device. Build it with a host compiler, optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I celestia-app_amd/csrc
//       tools/tx_parse_check.cpp -o tx_parse_check && ./tx_parse_check
// 1. txparse::read_uvarint and read_step against a bytewise model (128-bit accumulator, the
//    terminator found first) for every 1-byte and 2-byte stream and for the overflow edges.
// 2. txparse::chunk_pieces for every first-share R and both header sizes: every chunk byte is
//    taken exactly once from the share byte a walk of the stream puts it at, and the five aligned
//    dwords a piece reads lie inside the 512-byte cell or are left out and hold every byte taken.
// 3. The hint rule: over all patterns of reserved values of short streams, hints_hold over the
//    walks equals the rule stated on the sequential parse alone; where it holds, the walks up to
//    T are that parse, and where it does not, serial_walk is.
// 4. txparse::carve: the regions follow one another without overlap, sized for their entries,
//    and the null base gives the same size.
// tests/test_tx_parse_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "tx_parse.hpp"

using namespace cel;
using namespace cel::txparse;

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      if (fails < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fails++;                                                            \
    }                                                                     \
  } while (0)

struct Bytes {
  const std::vector<uint8_t>* v;
  uint8_t operator()(uint64_t x) { return v->at(x); }  // at(): a read behind the stream throws
};

// binary.Uvarint by the book: the first byte below 0x80 ends it.
static bool model_uvarint(const std::vector<uint8_t>& s, uint64_t p, uint64_t* v, uint32_t* used) {
  unsigned __int128 x = 0;
  for (uint32_t i = 0;; i++) {
    if (i == 10) return false;
    const uint8_t b = p + i < s.size() ? s[p + i] : 0;
    x |= (unsigned __int128)(b & 0x7F) << (7 * i);
    if (b < 0x80) {
      if (x >> 64) return false;
      *v = (uint64_t)x;
      *used = i + 1;
      return true;
    }
  }
}

static uint32_t model_canonical(uint64_t v) {
  uint32_t n = 0;
  do {
    n++;
    v >>= 7;
  } while (v);
  return n;
}

static void check_stream_steps(const std::vector<uint8_t>& s) {
  Bytes f{&s};
  uint64_t v = 0, mv = 0;
  uint32_t used = 0;
  const bool ok = read_uvarint(f, 0, s.size(), &v), mok = model_uvarint(s, 0, &mv, &used);
  CHECK(ok == mok);
  if (ok && mok) CHECK(v == mv);
  const Step st = read_step(f, 0, s.size());
  if (!mok) {
    CHECK(st.kind == kStopVarint);
  } else if (mv == 0) {
    CHECK(st.kind == kStopZero);
  } else {
    const uint32_t n = model_canonical(mv);
    CHECK(st.n == n && st.len == mv && n <= s.size());
    const bool fits = mv <= s.size() - n;
    CHECK(st.kind == (fits ? kUnit : kStopCut));
  }
}

static uint64_t check_uvarint() {
  uint64_t n = 0;
  for (uint32_t a = 0; a < 256; a++, n++) check_stream_steps({(uint8_t)a});
  for (uint32_t a = 0; a < 256; a++)
    for (uint32_t b = 0; b < 256; b++, n++) check_stream_steps({(uint8_t)a, (uint8_t)b});
  // the overflow edges: 9 and 10 continuation bytes, the 10th byte 0, 1, 2, 0x7f, 0x80, an 11th byte
  for (uint32_t lead = 8; lead <= 11; lead++)
    for (uint32_t last : {0x00u, 0x01u, 0x02u, 0x7Fu, 0x80u, 0xFFu})
      for (uint32_t fill : {0x80u, 0xFFu})
        for (uint32_t tail = 0; tail < 3; tail++, n++) {
          std::vector<uint8_t> s(lead, (uint8_t)fill);
          s.push_back((uint8_t)last);
          s.insert(s.end(), tail, 0x01);
          check_stream_steps(s);
        }
  const std::vector<uint8_t> none;
  Bytes f{&none};
  CHECK(read_step(f, 0, 0).kind == kStopEnd);
  return n;
}

// One share's place in a stream for check_chunks.
static uint64_t check_share_chunks(uint32_t abegin, uint32_t acontrib) {
  uint64_t n = 0;
  const uint64_t abase = 1000;
  for (uint32_t nbegin : {kContHdr, kStartHdr})
    for (uint32_t at = 0; at < acontrib; at++)
      for (uint32_t nbytes = 1; nbytes <= 16; nbytes++, n++) {
        Piece a, b;
        chunk_pieces(abase + at, nbytes, abase, acontrib, abegin, nbegin, a, b);
        uint32_t taken[16] = {0};
        for (const Piece* pc : {&a, &b}) {
          if (pc->lo >= pc->hi) continue;
          CHECK(pc->hi <= nbytes && pc->q + pc->hi <= 512);
          const uint32_t w0 = pc->q >> 2;
          for (uint32_t i = pc->lo; i < pc->hi; i++) {
            taken[i]++;
            const uint32_t byte = pc->q + i;  // of the share
            const uint32_t want = pc == &a ? abegin + at + i : nbegin + (at + i - acontrib);
            CHECK(byte == want);
            CHECK((byte >> 2) >= w0 && (byte >> 2) <= w0 + 4 && (byte >> 2) <= 127);
          }
        }
        if (b.lo < b.hi) CHECK(b.q >= 19 && a.hi == b.lo);
        for (uint32_t i = 0; i < nbytes; i++) CHECK(taken[i] == 1);
      }
  return n;
}

static uint64_t check_chunks() {
  uint64_t n = 0;
  for (uint32_t r = 1; r < 512; r++) n += check_share_chunks(r, 512 - r);  // a first share
  n += check_share_chunks(kContHdr, 512 - kContHdr);
  n += check_share_chunks(kStartHdr, 512 - kStartHdr);
  return n;
}

// A short stream: a first share with reserved value r0, then continuation shares (share 1 a start
// share with start1), filled with units of the given lengths and ended in one of four ways.
struct Stream {
  uint32_t r0;
  bool start1;
  std::vector<uint32_t> lens;
  uint32_t tail;  // 0: zeros, 1: a cut unit, 2: a varint that overflows, 3: the stream ends with the last unit
};

static void put_uvarint(std::vector<uint8_t>& s, uint64_t v) {
  while (v >= 0x80) s.push_back((uint8_t)(v | 0x80)), v >>= 7;
  s.push_back((uint8_t)v);
}

static const uint32_t kFixedHints[8] = {0, 33, 512, 34, 35, 100, 300, 511};

static uint64_t check_hints(const Stream& sm) {
  std::vector<uint8_t> s;
  std::vector<uint64_t> starts;
  for (uint32_t len : sm.lens) {
    starts.push_back(s.size());
    put_uvarint(s, len);
    for (uint32_t i = 0; i < len; i++) s.push_back((uint8_t)(i * 37 + len));  // plausible prefixes among them
  }
  if (sm.tail == 1) put_uvarint(s, 5000);
  if (sm.tail == 2) s.insert(s.end(), 11, 0xFF);
  // the shares: enough for the bytes, the last one filled with zeros (tail 3: none left over)
  std::vector<Class> cls;
  std::vector<Pre> pre;
  uint64_t bytes = 0;
  for (uint32_t j = 0; bytes < s.size() || j == 0; j++) {
    const uint32_t info = (j == 0 || (j == 1 && sm.start1)) ? 1u : 0u;
    Class c = classify(info, true, j == 0 ? sm.r0 : 0u, j == 0, j);
    cls.push_back(c);
    pre.push_back(Pre{bytes, 0, 0, 0});
    bytes += c.contrib;
  }
  if (sm.tail == 3) CHECK(bytes == s.size());
  s.resize(bytes, 0);
  const uint32_t n = (uint32_t)cls.size();
  pre.push_back(Pre{bytes, 0, 0, 0});
  // the sequential parse
  Bytes f{&s};
  std::vector<uint64_t> seq;
  bool seq_verr = false;
  for (uint64_t p = 0;;) {
    const Step st = read_step(f, p, bytes);
    if (st.kind != kUnit) {
      seq_verr = st.kind == kStopVarint;
      break;
    }
    seq.push_back(p);
    p += st.n + st.len;
  }
  CHECK(seq == starts && seq_verr == (sm.tail == 2));
  auto share_of = [&](uint64_t x) {
    uint32_t j = n - 1;
    while (pre[j].bytes > x) j--;
    return j;
  };
  std::vector<int64_t> first_in(n, -1);  // the first unit that begins in each share
  for (uint64_t p : seq)
    if (first_in[share_of(p)] < 0) first_in[share_of(p)] = (int64_t)p;
  const uint32_t t_seq = seq.empty() ? 0 : share_of(seq.back());
  // every pattern of 10 values per later share
  uint64_t patterns = 1, count = 0;
  for (uint32_t j = 1; j < n; j++) patterns *= 10;
  for (uint64_t code = 0; code < patterns; code++, count++) {
    uint64_t c = code;
    for (uint32_t j = 1; j < n; j++, c /= 10) {
      const uint32_t h = data_begin(cls[j]);
      const uint32_t right = first_in[j] < 0 ? 0u : h + (uint32_t)((uint64_t)first_in[j] - pre[j].bytes);
      const uint32_t pick = (uint32_t)(c % 10);
      const uint32_t hint = pick < 8 ? kFixedHints[pick] : pick == 8 ? right : right + 1;
      cls[j] = classify(cls[j].flags & kSeqStart ? 1u : 0u, true, hint, false, j);
    }
    uint64_t walked = 0;
    for (uint32_t j = 0; j <= n; j++) {
      pre[j].walked = walked;
      if (j < n && (cls[j].flags & kWalkedShare)) walked++;
    }
    // by the sequential parse alone
    bool want = true;
    for (uint32_t j = 1; j <= t_seq && !seq.empty(); j++) {
      const bool usable = (cls[j].flags & kWalkedShare) != 0;
      if ((first_in[j] >= 0) != usable) want = false;
      else if (usable && hinted_start(cls[j], pre.data(), 0, j) != (uint64_t)first_in[j]) want = false;
    }
    // by the walks
    std::vector<Walk> wk(n, Walk{0, 0, 0, 0, 0});
    for (uint32_t j = 0; j < n; j++)
      if (cls[j].flags & kWalkedShare)
        wk[j] = walk_from(f, hinted_start(cls[j], pre.data(), 0, j), pre[j + 1].bytes, bytes);
    uint32_t t = kNone;
    const bool hold = hints_hold(cls.data(), wk.data(), pre.data(), 0, n, &t);
    CHECK(hold == want);
    bool verr;
    if (hold) {
      CHECK(t == t_seq);
      verr = (wk[t].flags & kVarintErr) != 0;
      for (uint32_t j = t + 1; j < n; j++) wk[j] = Walk{0, 0, 0, 0, 0};
      for (uint32_t j = 0; j <= t; j++)
        if (!(cls[j].flags & kWalkedShare)) CHECK(wk[j].cnt == 0);
    } else {
      verr = serial_walk(f, pre.data(), 0, n, wk.data());
    }
    CHECK(verr == seq_verr);
    // the walks are the parse, cut at the shares
    std::vector<uint64_t> got;
    for (uint32_t j = 0; j < n; j++) {
      uint64_t p = wk[j].start;
      for (uint32_t i = 0; i < wk[j].cnt; i++) {
        CHECK(share_of(p) == j);
        got.push_back(p);
        const Step st = read_step(f, p, bytes);
        p += st.n + st.len;
      }
    }
    CHECK(got == seq);
  }
  return count;
}

static uint64_t check_hint_rule() {
  const Stream streams[] = {
      {38, false, {498, 998, 40}, 0},         // 4 shares, none begins in share 2
      {38, false, {100, 100, 100, 100, 300, 20, 600}, 0},
      {38, false, {472}, 3},                  // one share, filled
      {38, false, {472, 476}, 3},             // two shares, both filled
      {38, true, {472, 472, 30}, 0},          // share 1 a start share
      {38, false, {1500}, 1},                 // a cut unit behind a long one
      {38, false, {470, 1, 1, 1, 1, 700}, 2}, // a varint error at the end
      {38, false, {}, 0},                     // zeros only
      {0, false, {300, 400}, 0},              // the first share gives nothing: the stream begins in share 1
      {100, false, {600, 5}, 0},              // R < h on the first share
      {511, false, {700, 9}, 0},              // one byte of the first share
  };
  uint64_t n = 0;
  for (const Stream& sm : streams) n += check_hints(sm);
  return n;
}

static uint64_t check_carve() {
  uint64_t n = 0;
  for (uint64_t total : {0ull, 1ull, 255ull, 256ull, 257ull, 16384ull, 262144ull})
    for (uint32_t ranges : {1u, 2u, 1000u}) {
      const Work z = carve(nullptr, total, ranges);
      std::vector<uint8_t> buf(z.bytes);
      const Work w = carve(buf.data(), total, ranges);
      CHECK(w.bytes == z.bytes && z.head == nullptr && z.wk == nullptr);
      const uint8_t* regions[] = {(uint8_t*)w.head,      (uint8_t*)w.roff,        (uint8_t*)w.range_status,
                                  (uint8_t*)w.range_flags, (uint8_t*)w.range_t,   (uint8_t*)w.range_bad,
                                  (uint8_t*)w.cls,       (uint8_t*)w.pre,         (uint8_t*)w.wk,
                                  (uint8_t*)w.upre,      (uint8_t*)w.sums1,       (uint8_t*)w.sums2,
                                  buf.data() + w.bytes};
      const size_t need[] = {sizeof(Head), (2 * (size_t)ranges + 1) * 4, (size_t)ranges * 4, (size_t)ranges * 4,
                             (size_t)ranges * 4, (size_t)ranges * 4, total * sizeof(Class), (total + 1) * sizeof(Pre),
                             total * sizeof(Walk), (total + 1) * sizeof(UnitPre), w.blocks * sizeof(Pre),
                             w.blocks * sizeof(UnitPre)};
      CHECK(regions[0] == buf.data());
      for (int i = 0; i < 12; i++) {
        CHECK(regions[i + 1] >= regions[i] + need[i]);
        CHECK((regions[i] - buf.data()) % 256 == 0);
      }
      CHECK(w.rstart == w.roff + ranges + 1);
      CHECK(w.blocks == (total ? (total + 255) / 256 : 1));
      // linear in the shares and the ranges, whatever the units
      CHECK(w.bytes <= 256 * 16 + total * 128 + (size_t)ranges * 32 + 13 * 256);
      n++;
    }
  return n;
}

int main() {
  std::printf("uvarint: %llu streams\n", (unsigned long long)check_uvarint());
  std::printf("chunks: %llu\n", (unsigned long long)check_chunks());
  std::printf("hints: %llu patterns\n", (unsigned long long)check_hint_rule());
  std::printf("carve: %llu workspaces\n", (unsigned long long)check_carve());
  std::printf("tx parse check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
