// Data-square construction: a block's txs -> the k*k ODS shares that da.ExtendShares
// receives.
//
// Restates go-square v1.1.0 (go.mod:9, [dep], not in /root/reference) as called by
//   app/extend_block.go:16-25      square.Construct(txs, SquareSizeUpperBound, SubtreeRootThreshold)
//   app/process_proposal.go:121-130 square.Construct(...)
//   app/prepare_proposal.go:48-61   square.Build(...)  (greedy: drops txs that do not fit)
// with the rules of specs/src/specs/shares.md:24-98 (compact and sparse shares),
// namespace.md:77-84 (reserved namespaces), data_square_layout.md:38-62 (blob
// placement) and SURVEY.md Appendix A.4. Host code: pure byte layout, sequential by
// nature. Builder::export_layout decides where every share goes (segments, start indexes,
// the compact shares) without touching a blob byte; expand_layout writes the bytes for
// cel_square_construct, and k_square_build (square_build.hip) writes them on the device
// from the same layout for cel_block_extend.
//
// Builder (go-square square/builder.go): normal txs first, then BlobTxs. Every append
// is admitted only if the worst-case square still fits maxSquareSize^2:
//   tx shares + PFB shares (index wrappers with worst-case share indexes)
//   + sum over blobs of (shares + SubTreeWidth(shares) - 1).
// Export: square width = RoundUpPow2(ceil(sqrt(worst case))); blobs stably sorted by
// namespace, each placed at the next multiple of its SubTreeWidth; PFB index wrappers
// carry the real start indexes; primary reserved padding up to the first blob,
// namespace padding (previous blob's namespace) between blobs, tail padding to k*k.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/celestia_eds.h"
#include "blob_plan.hpp"
#include "square_blobs.hpp"

namespace cel {
namespace sq {
namespace {  // internal linkage: only the C entry points are exported

constexpr uint32_t kShare = CEL_SHARE_SIZE;
constexpr uint32_t kNs = CEL_NAMESPACE_SIZE;
constexpr uint32_t kNsIdSize = 28;
// compact share payload: first share ns | info | sequence length(4) | reserved(4)
constexpr uint32_t kCompactFirst = kShare - kNs - 1 - 4 - 4;  // 474
constexpr uint32_t kCompactCont = kShare - kNs - 1 - 4;       // 478
// sparse share payloads (478 first, 482 after): blob_plan.hpp

using Bytes = std::vector<uint8_t>;
using Ns = std::array<uint8_t, kNs>;

static Ns ns_of(uint8_t version, uint8_t last) {
  Ns n{};
  n[0] = version;
  n[kNs - 1] = last;
  return n;
}
static const Ns kTxNs = ns_of(0, 0x01);              // namespace.md:79 TxNamespace
static const Ns kPfbNs = ns_of(0, 0x04);             // PayForBlobNamespace
static const Ns kPrimaryPadNs = ns_of(0, 0xFF);      // PrimaryReservedPaddingNamespace
static Ns tail_pad_ns() {                            // TailPaddingNamespace 0xFF*28 || 0xFE
  Ns n;
  n.fill(0xFF);
  n[kNs - 1] = 0xFE;
  return n;
}

static void put_uvarint(Bytes& out, uint64_t v) {
  while (v >= 0x80) {
    out.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  out.push_back((uint8_t)v);
}
static uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    n++;
  }
  return n;
}

// ----------------------------------------------------------- protobuf wire reads
struct Field {
  uint32_t num, wire;
  uint64_t varint;
  const uint8_t* p;
  size_t len;
};

static bool read_uvarint(const uint8_t*& p, const uint8_t* end, uint64_t& v) {
  v = 0;
  for (int shift = 0; shift < 64; shift += 7) {
    if (p >= end) return false;
    const uint8_t b = *p++;
    v |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) return true;
  }
  return false;
}

// Skips the rest of a group whose start key (wire type 3) was just read: nested fields up
// to the matching end-group key. The generated gogoproto skip function (skipBlob) does the
// same for unknown fields; false where it returns an error.
static bool skip_group(const uint8_t*& p, const uint8_t* end) {
  int depth = 1;
  while (p < end) {
    uint64_t key, v;
    if (!read_uvarint(p, end, key)) return false;
    switch (key & 7) {
      case 0:
        if (!read_uvarint(p, end, v)) return false;
        break;
      case 1:
        if (end - p < 8) return false;
        p += 8;
        break;
      case 2:
        if (!read_uvarint(p, end, v) || v > (uint64_t)(end - p)) return false;
        p += v;
        break;
      case 3:
        depth++;
        break;
      case 4:
        if (--depth == 0) return true;
        break;
      case 5:
        if (end - p < 4) return false;
        p += 4;
        break;
      default:
        return false;
    }
  }
  return false;
}

// Decodes one message level; false on malformed wire data (proto.Unmarshal error). The
// field number is the key's bits 3.. taken as an int32, and must be > 0 (gogoproto
// "illegal tag"); an end-group key outside a group is an error; a group (wire type 3) is
// kept as a field of wire type 3 so that a known field number rejects it.
static bool parse_fields(const uint8_t* p, size_t n, std::vector<Field>& out) {
  const uint8_t* end = p + n;
  while (p < end) {
    uint64_t key;
    if (!read_uvarint(p, end, key)) return false;
    Field f{(uint32_t)(key >> 3), (uint32_t)(key & 7), 0, nullptr, 0};
    if ((int32_t)f.num <= 0) return false;
    switch (f.wire) {
      case 0:
        if (!read_uvarint(p, end, f.varint)) return false;
        break;
      case 1:
        if (end - p < 8) return false;
        f.p = p;
        f.len = 8;
        p += 8;
        break;
      case 2: {
        uint64_t ln;
        if (!read_uvarint(p, end, ln) || ln > (uint64_t)(end - p)) return false;
        f.p = p;
        f.len = (size_t)ln;
        p += ln;
        break;
      }
      case 3:
        if (!skip_group(p, end)) return false;
        break;
      case 5:
        if (end - p < 4) return false;
        f.p = p;
        f.len = 4;
        p += 4;
        break;
      default:
        return false;
    }
    out.push_back(f);
  }
  return true;
}

struct Blob {
  Ns ns;
  const uint8_t* data;
  size_t len;
  uint32_t share_version;
};

// blob.UnmarshalBlobTx (go-square v1.1.0 blob/blob.go): BlobTx {1: tx, 2: repeated Blob,
// 3: type_id}; a blob tx iff it parses, type_id == "BLOB", it has blobs and every
// namespace id is 28 bytes. Blob {1: namespace_id, 2: data, 3: share_version,
// 4: namespace_version} (proto/celestia/core/v1/blob/blob.proto).
static bool unmarshal_blob_tx(const uint8_t* tx, size_t n, const uint8_t*& inner, size_t& inner_len,
                              std::vector<Blob>& blobs) {
  std::vector<Field> fs;
  if (!parse_fields(tx, n, fs)) return false;
  bool typed = false;
  inner = nullptr;
  inner_len = 0;
  blobs.clear();
  for (const Field& f : fs) {
    if (f.num == 1) {
      if (f.wire != 2) return false;
      inner = f.p;
      inner_len = f.len;
    } else if (f.num == 2) {
      if (f.wire != 2) return false;
      std::vector<Field> bf;
      if (!parse_fields(f.p, f.len, bf)) return false;
      Blob b{};
      const uint8_t* id = nullptr;
      size_t id_len = 0;
      uint64_t ns_version = 0;
      for (const Field& g : bf) {
        if (g.num == 1) {
          if (g.wire != 2) return false;
          id = g.p;
          id_len = g.len;
        } else if (g.num == 2) {
          if (g.wire != 2) return false;
          b.data = g.p;
          b.len = g.len;
        } else if (g.num == 3) {
          if (g.wire != 0) return false;
          b.share_version = (uint32_t)g.varint;
        } else if (g.num == 4) {
          if (g.wire != 0) return false;
          ns_version = g.varint;
        }
      }
      if (id_len != kNsIdSize) return false;
      b.ns[0] = (uint8_t)ns_version;
      std::memcpy(b.ns.data() + 1, id, kNsIdSize);
      blobs.push_back(b);
    } else if (f.num == 3) {
      if (f.wire != 2) return false;
      typed = f.len == 4 && std::memcmp(f.p, "BLOB", 4) == 0;
    }
  }
  return typed && !blobs.empty();
}

// IndexWrapper {1: tx, 2: packed share_indexes, 3: type_id "INDX"} (gogoproto Marshal).
static Bytes marshal_index_wrapper(const uint8_t* tx, size_t n, const std::vector<uint32_t>& idx) {
  Bytes packed;
  for (uint32_t i : idx) put_uvarint(packed, i);
  Bytes out;
  if (n) {  // proto3 omits empty bytes fields
    out.push_back(0x0A);
    put_uvarint(out, n);
    out.insert(out.end(), tx, tx + n);
  }
  if (!packed.empty()) {
    out.push_back(0x12);
    put_uvarint(out, packed.size());
    out.insert(out.end(), packed.begin(), packed.end());
  }
  out.push_back(0x1A);
  out.push_back(4);
  out.insert(out.end(), {'I', 'N', 'D', 'X'});
  return out;
}

// ------------------------------------------------------------------ share counts
// shares.CompactShareCounter: units are uvarint(len) || unit, packed in one sequence.
static uint32_t compact_shares_for(uint64_t seq_bytes) {
  if (seq_bytes == 0) return 0;
  if (seq_bytes <= kCompactFirst) return 1;
  return 1 + (uint32_t)((seq_bytes - kCompactFirst + kCompactCont - 1) / kCompactCont);
}
// shares.SparseSharesNeeded
static uint32_t sparse_shares_for(uint64_t len) { return (uint32_t)blob::sparse_shares_needed(len); }
// inclusion.BlobMinSquareSize / SubTreeWidth (blob_plan.hpp) / NextShareIndex (go-square v1.1.0)
using blob::blob_min_square_size;
using blob::pow2ceil;
using blob::subtree_width;
static uint32_t next_share_index(uint32_t cursor, uint32_t shares, uint32_t threshold) {
  const uint32_t w = subtree_width(shares, threshold);
  return (cursor + w - 1) / w * w;
}

// ---------------------------------------------------------------- share writers
static void write_compact(const Ns& ns, const std::vector<Bytes>& units, std::vector<uint8_t>& sq) {
  if (units.empty()) return;
  Bytes data;
  std::vector<size_t> starts;
  for (const Bytes& u : units) {
    starts.push_back(data.size());
    put_uvarint(data, u.size());
    data.insert(data.end(), u.begin(), u.end());
  }
  size_t pos = 0, next_unit = 0;
  for (bool first = true; first || pos < data.size(); first = false) {
    uint8_t sh[kShare] = {0};
    std::memcpy(sh, ns.data(), kNs);
    sh[kNs] = first ? 1 : 0;  // share version 0, sequence start
    uint32_t header = kNs + 1;
    if (first) {
      const uint32_t L = (uint32_t)data.size();
      sh[header] = (uint8_t)(L >> 24), sh[header + 1] = (uint8_t)(L >> 16);
      sh[header + 2] = (uint8_t)(L >> 8), sh[header + 3] = (uint8_t)L;
      header += 4;
    }
    const uint32_t cap = kShare - header - 4;
    // reserved bytes: offset (within this share) of the first unit that starts in it
    while (next_unit < starts.size() && starts[next_unit] < pos) next_unit++;
    uint32_t reserved = 0;
    if (next_unit < starts.size() && starts[next_unit] < pos + cap) reserved = header + 4 + (uint32_t)(starts[next_unit] - pos);
    sh[header] = (uint8_t)(reserved >> 24), sh[header + 1] = (uint8_t)(reserved >> 16);
    sh[header + 2] = (uint8_t)(reserved >> 8), sh[header + 3] = (uint8_t)reserved;
    const size_t n = std::min<size_t>(cap, data.size() - std::min(pos, data.size()));
    if (n) std::memcpy(sh + header + 4, data.data() + pos, n);
    sq.insert(sq.end(), sh, sh + kShare);
    pos += cap;
  }
}

// Sparse shares of one blob, written in place at dst (shares * 512 bytes).
static void write_sparse(const uint8_t* ns, uint32_t share_version, const uint8_t* data, size_t len, uint8_t* dst) {
  size_t pos = 0;
  for (bool first = true; pos < len; first = false, dst += kShare) {
    std::memset(dst, 0, kShare);
    std::memcpy(dst, ns, kNs);
    dst[kNs] = (uint8_t)((share_version << 1) | (first ? 1 : 0));
    uint32_t header = kNs + 1;
    if (first) {
      const uint32_t L = (uint32_t)len;
      dst[header] = (uint8_t)(L >> 24), dst[header + 1] = (uint8_t)(L >> 16);
      dst[header + 2] = (uint8_t)(L >> 8), dst[header + 3] = (uint8_t)L;
      header += 4;
    }
    const size_t n = std::min<size_t>(kShare - header, len - pos);
    std::memcpy(dst + header, data + pos, n);
    pos += n;
  }
}

static void write_padding(const uint8_t* ns, uint32_t count, uint8_t* dst) {
  for (uint32_t i = 0; i < count; i++, dst += kShare) {
    std::memset(dst, 0, kShare);
    std::memcpy(dst, ns, kNs);
    dst[kNs] = 1;  // share version 0, sequence start; sequence length 0
  }
}

// The bytes of a layout: every segment written at its place in the k * k shares. `base` is
// the concatenated txs the BLOB segments point into.
static void expand_layout(const Layout& L, const uint8_t* base, std::vector<uint8_t>& sq) {
  sq.resize((size_t)L.k * L.k * kShare);
  for (const cel_square_segment& s : L.segs) {
    uint8_t* dst = sq.data() + (size_t)s.start * kShare;
    if (s.kind == CEL_SEG_COMPACT)
      std::memcpy(dst, L.compact.data() + (size_t)s.off * kShare, (size_t)s.count * kShare);
    else if (s.kind == CEL_SEG_BLOB)
      write_sparse(s.ns, s.share_version, base + s.off, s.len, dst);
    else
      write_padding(s.ns, s.count, dst);
  }
}

// -------------------------------------------------------------------- builder
struct Pfb {
  const uint8_t* tx;
  size_t len;
  std::vector<uint32_t> idx;
};
struct Element {
  Blob blob;
  uint32_t pfb, index, shares;
  uint32_t tx;  // index of the BlobTx among the block's txs
};

struct Builder {
  uint32_t max_size, threshold;
  uint64_t max_capacity;
  uint64_t current = 0;        // worst-case share count so far
  uint64_t tx_bytes = 0, pfb_bytes = 0;  // compact sequence lengths (counters)
  std::vector<Bytes> txs;
  std::vector<Pfb> pfbs;
  std::vector<Element> blobs;
  std::vector<Bytes> iws;  // final PFB index wrappers (after export_square)

  Builder(uint32_t m, uint32_t t) : max_size(m), threshold(t), max_capacity((uint64_t)m * m) {}

  // Builder.AppendTx
  bool append_tx(const uint8_t* tx, size_t n) {
    const uint64_t nb = tx_bytes + uvarint_len(n) + n;
    const uint64_t diff = compact_shares_for(nb) - compact_shares_for(tx_bytes);
    if (current + diff > max_capacity) return false;
    current += diff;
    tx_bytes = nb;
    txs.emplace_back(tx, tx + n);
    return true;
  }

  // Builder.AppendBlobTx: the index wrapper is counted with worst-case share indexes
  // (maxSquareSize^2), each blob with its shares plus SubTreeWidth - 1 of padding.
  bool append_blob_tx(const uint8_t* inner, size_t n, const std::vector<Blob>& bl, uint32_t tx_index) {
    const std::vector<uint32_t> worst(bl.size(), max_size * max_size);
    const size_t iw = marshal_index_wrapper(inner, n, worst).size();
    const uint64_t nb = pfb_bytes + uvarint_len(iw) + iw;
    uint64_t diff = compact_shares_for(nb) - compact_shares_for(pfb_bytes);
    for (const Blob& b : bl) {
      const uint32_t s = sparse_shares_for(b.len);
      diff += s + subtree_width(s, threshold) - 1;
    }
    if (current + diff > max_capacity) return false;
    current += diff;
    pfb_bytes = nb;
    const uint32_t pi = (uint32_t)pfbs.size();
    pfbs.push_back(Pfb{inner, n, std::vector<uint32_t>(bl.size(), 0)});
    for (uint32_t i = 0; i < bl.size(); i++) blobs.push_back(Element{bl[i], pi, i, sparse_shares_for(bl[i].len), tx_index});
    return true;
  }

  // Builder.Export, the layout only: where every share goes, the start indexes inside the
  // index wrappers, and the compact shares those wrappers fill. `base`: the concatenated txs
  // (BLOB segments carry offsets into it). The one walk of cursor / next_share_index /
  // padding; export_square writes its bytes.
  void export_layout(const uint8_t* base, Layout& L) {
    L.compact.clear();
    L.segs.clear();
    uint32_t at = 0;  // next share index
    auto add = [&](uint32_t kind, uint32_t count, const uint8_t* ns) -> cel_square_segment* {
      if (!count) return nullptr;
      cel_square_segment s;
      std::memset(&s, 0, sizeof s);
      s.kind = kind;
      s.start = at;
      s.count = count;
      if (ns) std::memcpy(s.ns, ns, kNs);
      at += count;
      L.segs.push_back(s);
      return &L.segs.back();
    };
    const Ns tail = tail_pad_ns();
    if (txs.empty() && pfbs.empty()) {  // EmptySquare: one tail padding share
      add(CEL_SEG_PAD, 1, tail.data());
      L.k = 1;
      return;
    }
    const uint32_t k = blob_min_square_size(current);
    std::stable_sort(blobs.begin(), blobs.end(),
                     [](const Element& a, const Element& b) { return a.blob.ns < b.blob.ns; });
    const uint32_t non_reserved = compact_shares_for(tx_bytes) + compact_shares_for(pfb_bytes);
    uint32_t cursor = non_reserved;
    std::vector<uint32_t> starts(blobs.size());
    for (size_t i = 0; i < blobs.size(); i++) {
      const Element& e = blobs[i];
      cursor = next_share_index(cursor, e.shares, threshold);
      pfbs[e.pfb].idx[e.index] = starts[i] = cursor;
      cursor += e.shares;
    }
    iws.clear();
    for (const Pfb& p : pfbs) iws.push_back(marshal_index_wrapper(p.tx, p.len, p.idx));
    write_compact(kTxNs, txs, L.compact);
    write_compact(kPfbNs, iws, L.compact);
    // WriteSquare: primary reserved padding up to the first blob, the blobs with namespace
    // padding (the previous blob's namespace) between them, tail padding
    const uint32_t ncompact = (uint32_t)(L.compact.size() / kShare);
    add(CEL_SEG_COMPACT, ncompact, nullptr);
    add(CEL_SEG_PAD, (blobs.empty() ? ncompact : starts[0]) - ncompact, kPrimaryPadNs.data());
    for (size_t i = 0; i < blobs.size(); i++) {
      const Element& e = blobs[i];
      if (i) add(CEL_SEG_PAD, starts[i] - at, blobs[i - 1].blob.ns.data());
      if (cel_square_segment* s = add(CEL_SEG_BLOB, e.shares, e.blob.ns.data())) {
        s->share_version = e.blob.share_version;
        s->off = (uint64_t)(e.blob.data - base);
        s->len = (uint32_t)e.blob.len;
        s->tx_index = e.tx;
      }
    }
    add(CEL_SEG_PAD, (uint32_t)((uint64_t)k * k - at), tail.data());
    L.k = k;
  }

  // Builder.Export: the layout, then its bytes.
  uint32_t export_square(const uint8_t* base, std::vector<uint8_t>& sq) {
    Layout L;
    export_layout(base, L);
    expand_layout(L, base, sq);
    return L.k;
  }

  // Builder.FindTxShareRange (after export_square): the shares [start, end) holding the
  // uvarint(len) || tx unit of normal tx `i` (i < txs.size()) or of the PFB index
  // wrapper i - txs.size() (offset by the tx shares, which precede the PFB shares).
  bool tx_range(size_t i, uint32_t& start, uint32_t& end) const {
    const bool pfb = i >= txs.size();
    const std::vector<Bytes>& units = pfb ? iws : txs;
    const size_t u = pfb ? i - txs.size() : i;
    if (u >= units.size()) return false;
    uint64_t off = 0;
    for (size_t j = 0; j < u; j++) off += uvarint_len(units[j].size()) + units[j].size();
    const uint64_t last = off + uvarint_len(units[u].size()) + units[u].size() - 1;
    auto share_of = [](uint64_t b) -> uint32_t {
      return b < kCompactFirst ? 0u : 1u + (uint32_t)((b - kCompactFirst) / kCompactCont);
    };
    const uint32_t base = pfb ? compact_shares_for(tx_bytes) : 0u;
    start = base + share_of(off);
    end = base + share_of(last) + 1;
    return true;
  }
};

}  // namespace
}  // namespace sq

bool blob::blob_tx_views(const uint8_t* tx, size_t n, std::vector<View>& out) {
  const uint8_t* inner;
  size_t inner_len;
  std::vector<sq::Blob> blobs;
  out.clear();
  if (!sq::unmarshal_blob_tx(tx, n, inner, inner_len, blobs)) return false;
  for (const sq::Blob& b : blobs) {
    View v;
    std::memcpy(v.ns, b.ns.data(), sizeof v.ns);
    v.data = b.data;
    v.len = b.len;
    v.share_version = b.share_version;
    out.push_back(v);
  }
  return true;
}

}  // namespace cel

namespace {
thread_local std::string g_square_error;
}

extern "C" {

const char* cel_square_last_error(void) { return g_square_error.c_str(); }

}  // extern "C"

namespace {

// NewBuilder(txs...) / Build's admission loop; fills included[] (0 / 1 normal / 2 blob).
cel_status build_square(cel::sq::Builder& b, const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx,
                        uint32_t greedy, uint8_t* included, std::vector<cel::sq::BlobRef>* all_blobs = nullptr) {
  using namespace cel::sq;
  size_t off = 0;
  bool seen_blob_tx = false;
  std::vector<Blob> blobs;
  for (uint32_t i = 0; i < ntx; i++) {
    const uint8_t* tx = txs + off;
    const size_t n = tx_lens[i];
    off += n;
    const uint8_t* inner;
    size_t inner_len;
    bool ok;
    const bool is_blob = unmarshal_blob_tx(tx, n, inner, inner_len, blobs);
    if (is_blob) {
      seen_blob_tx = true;
      if (all_blobs)
        for (const Blob& bl : blobs) {
          BlobRef r;
          std::memcpy(r.ns, bl.ns.data(), kNs);
          r.off = bl.len ? (uint64_t)(bl.data - txs) : 0;
          r.len = bl.len;
          r.share_version = bl.share_version;
          r.tx_index = i;
          all_blobs->push_back(r);
        }
      ok = b.append_blob_tx(inner, inner_len, blobs, i);
    } else {
      if (seen_blob_tx && !greedy) {  // square.Construct requires normal txs first
        g_square_error = "normal transaction at index " + std::to_string(i) + " can not be appended after blob tx";
        return CEL_EINVAL;
      }
      ok = b.append_tx(tx, n);
    }
    if (included) included[i] = ok ? (is_blob ? 2 : 1) : 0;
    if (!ok && !greedy) {
      g_square_error = std::string("not enough space to append ") + (seen_blob_tx ? "blob tx" : "tx") +
                       " at index " + std::to_string(i);
      return CEL_ETOOBIG;
    }
  }
  return CEL_OK;
}

bool args_ok(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
             uint32_t subtree_root_threshold) {
  return !((ntx && (!txs || !tx_lens)) || !max_square_size || !subtree_root_threshold ||
           (max_square_size & (max_square_size - 1)));
}

}  // namespace

cel_status cel::sq::square_layout(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
                                  uint32_t subtree_root_threshold, uint32_t greedy, uint8_t* included, Layout& out,
                                  std::vector<BlobRef>* all_blobs) {
  g_square_error.clear();
  if (!args_ok(txs, tx_lens, ntx, max_square_size, subtree_root_threshold)) {
    g_square_error = "invalid argument";
    return CEL_EINVAL;
  }
  Builder b(max_square_size, subtree_root_threshold);
  cel_status st = build_square(b, txs, tx_lens, ntx, greedy, included, all_blobs);
  if (st) return st;
  b.export_layout(txs, out);
  return CEL_OK;
}

extern "C" {

cel_status cel_square_layout(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
                             uint32_t subtree_root_threshold, uint32_t greedy, uint32_t* k_out, uint8_t* included,
                             cel_square_segment* segments, uint32_t cap_segments, uint32_t* n_segments,
                             uint8_t* compact_out, uint32_t cap_compact_shares, uint32_t* n_compact_shares) {
  using namespace cel::sq;
  if (!k_out || !n_segments || !n_compact_shares || (cap_segments && !segments) ||
      (cap_compact_shares && !compact_out)) {
    g_square_error = "invalid argument";
    return CEL_EINVAL;
  }
  Layout L;
  cel_status st = square_layout(txs, tx_lens, ntx, max_square_size, subtree_root_threshold, greedy, included, L, nullptr);
  if (st) return st;
  const uint32_t ncompact = (uint32_t)(L.compact.size() / kShare);
  *k_out = L.k;
  *n_segments = (uint32_t)L.segs.size();
  *n_compact_shares = ncompact;
  if (cap_segments == 0) return CEL_OK;  // size query
  if (L.segs.size() > cap_segments || ncompact > cap_compact_shares) {
    g_square_error = "output holds " + std::to_string(cap_segments) + " segments and " +
                     std::to_string(cap_compact_shares) + " compact shares, the layout needs " +
                     std::to_string(L.segs.size()) + " and " + std::to_string(ncompact);
    return CEL_EINVAL;
  }
  std::memcpy(segments, L.segs.data(), L.segs.size() * sizeof(cel_square_segment));
  if (ncompact) std::memcpy(compact_out, L.compact.data(), L.compact.size());
  return CEL_OK;
}

cel_status cel_square_construct(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
                                uint32_t subtree_root_threshold, uint32_t greedy, uint8_t* shares_out,
                                uint32_t cap_shares, uint32_t* k_out, uint8_t* included) {
  using namespace cel::sq;
  g_square_error.clear();
  if (!k_out || !args_ok(txs, tx_lens, ntx, max_square_size, subtree_root_threshold)) {
    g_square_error = "invalid argument";
    return CEL_EINVAL;
  }
  Builder b(max_square_size, subtree_root_threshold);
  cel_status st = build_square(b, txs, tx_lens, ntx, greedy, included);
  if (st) return st;
  std::vector<uint8_t> sq;
  const uint32_t k = b.export_square(txs, sq);
  *k_out = k;
  if (!shares_out) return CEL_OK;  // size query
  if ((uint64_t)k * k > cap_shares) {
    g_square_error = "output buffer holds " + std::to_string(cap_shares) + " shares, square needs " +
                     std::to_string((uint64_t)k * k);
    return CEL_EINVAL;
  }
  std::memcpy(shares_out, sq.data(), sq.size());
  return CEL_OK;
}

cel_status cel_square_tx_range(const uint8_t* txs, const uint32_t* tx_lens, uint32_t ntx, uint32_t max_square_size,
                               uint32_t subtree_root_threshold, uint32_t tx_index, uint32_t* start, uint32_t* end) {
  using namespace cel::sq;
  g_square_error.clear();
  if (!start || !end || !args_ok(txs, tx_lens, ntx, max_square_size, subtree_root_threshold)) {
    g_square_error = "invalid argument";
    return CEL_EINVAL;
  }
  if (tx_index >= ntx) {  // pkg/proof/proof.go:23-25
    g_square_error = "txIndex " + std::to_string(tx_index) + " out of bounds";
    return CEL_EINVAL;
  }
  Builder b(max_square_size, subtree_root_threshold);
  cel_status st = build_square(b, txs, tx_lens, ntx, 0, nullptr);
  if (st) return st;
  Layout L;
  b.export_layout(txs, L);
  if (!b.tx_range(tx_index, *start, *end)) {
    g_square_error = "txIndex " + std::to_string(tx_index) + " out of range";
    return CEL_EINVAL;
  }
  return CEL_OK;
}

}  // extern "C"
