// Stand-alone host check of the namespace queries' arithmetic
// (celestia-app_amd/csrc/nmt_namespace.hpp): no HIP, no device. Build it with a host compiler,
// optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/namespace_plan_check.cpp -o namespace_plan_check && ./namespace_plan_check
// For every width W = 2 .. 256 and every class of a (namespace, row) pair - the namespace inside
// the root's range or not, lt = 0 .. W leaves below it, le = lt .. W leaves at or below it:
// 1. nsq::classify against the rules spelt out below, and the node count against a walk of the
//    tree (the maximal subtrees outside the range, one more node for an absence entry);
// 2. every range inside the row: start < end <= W, and the leaf of an absence entry a leaf of
//    the row (start < W);
// 3. the offsets nsq::plan_scan gives (block sums, their scan, the add, as the kernels run them):
//    the entries in pair order, their nodes and shares tiling [0, total) without gap or overlap,
//    written into buffers of exactly the totals' size.
// It also checks that the workspace's regions (nsq::carve) follow one another without overlap.
// tests/test_namespace_plan_check.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "nmt_namespace.hpp"

using namespace cel;
using namespace cel::nsq;

static int fails = 0;
#define CHECK(c)                                                                                              \
  do {                                                                                                        \
    if (!(c)) {                                                                                               \
      if (fails < 20)                                                                                         \
        std::printf("FAIL %s:%d: %s (W = %u, lt = %u, le = %u)\n", __FILE__, __LINE__, #c, W, lt, le);        \
      fails++;                                                                                                \
    }                                                                                                         \
  } while (0)

// The number of maximal subtrees of [start, end) that do not overlap [ps, pe).
static uint32_t walk(uint32_t start, uint32_t end, uint32_t ps, uint32_t pe) {
  if (end <= ps || start >= pe) return 1;
  if (end - start == 1) return 0;
  const uint32_t half = (end - start) / 2;
  return walk(start, start + half, ps, pe) + walk(start + half, end, ps, pe);
}

struct Counts {
  uint64_t pairs, entries, nodes, leaves;
};

static Counts check_width(uint32_t W) {
  uint32_t L = 0, lt = 0, le = 0;
  while ((1u << L) < W) L++;
  std::vector<Pair> pairs;
  Counts want{0, 0, 0, 0};
  for (int inside = 0; inside < 2; inside++)
    for (lt = 0; lt <= W; lt++)
      for (le = lt; le <= W; le++) {
        const Pair p = classify(inside != 0, lt, le, W);
        pairs.push_back(p);
        const bool entry = inside && lt < W;
        CHECK((p.entry != 0) == entry);
        if (!entry) {
          CHECK(p.kind == 0 && p.start == 0 && p.end == 0);
          CHECK(entry_nodes(L, p) == 0 && entry_leaves(p) == 0);
          continue;
        }
        const bool present = le > lt;
        CHECK(p.kind == (present ? kInclusion : kAbsence));
        CHECK(p.start == lt && p.end == (present ? le : lt + 1));
        CHECK(p.start < p.end && p.end <= W && p.start < W);
        CHECK(entry_nodes(L, p) == walk(0, W, p.start, p.end) + (present ? 0 : 1));
        CHECK(entry_leaves(p) == (present ? le - lt : 0));
        want.entries++;
        want.nodes += entry_nodes(L, p);
        want.leaves += entry_leaves(p);
      }
  want.pairs = pairs.size();
  // the scan over this table taken as the pairs of want.pairs / W namespaces (the last one's rows
  // cut short: the scan does not care)
  lt = le = 0;
  std::vector<Sums> block_sums((pairs.size() + kScanBlock - 1) / kScanBlock);
  std::vector<Request> req(want.entries);  // exactly the entries: one more is a write out of bounds
  const Sums tot = plan_scan(pairs.data(), pairs.size(), W, L, block_sums.data(), req.data());
  CHECK(tot.entries == want.entries && tot.nodes == want.nodes && tot.leaves == want.leaves);
  std::vector<uint8_t> node_seen(want.nodes, 0), leaf_seen(want.leaves, 0);
  uint64_t e = 0, node_at = 0, leaf_at = 0;
  for (uint64_t p = 0; p < pairs.size(); p++) {
    if (!pairs[p].entry) continue;
    const Request& q = req[e++];
    CHECK(q.ns_idx == p / W && q.row == p % W);
    CHECK((uint32_t)q.start == pairs[p].start && (uint32_t)q.end == pairs[p].end && q.kind == pairs[p].kind);
    CHECK(q.nnodes == entry_nodes(L, pairs[p]));
    CHECK(q.node0 == node_at && q.leaf0 == leaf_at);
    for (uint64_t j = q.node0; j < q.node0 + q.nnodes && j < want.nodes; j++) node_seen[j]++;
    for (uint64_t j = q.leaf0; j < q.leaf0 + entry_leaves(pairs[p]) && j < want.leaves; j++) leaf_seen[j]++;
    node_at += q.nnodes;
    leaf_at += entry_leaves(pairs[p]);
  }
  CHECK(e == want.entries && node_at == want.nodes && leaf_at == want.leaves);
  for (uint8_t v : node_seen) CHECK(v == 1);
  for (uint8_t v : leaf_seen) CHECK(v == 1);
  return want;
}

static void check_carve(uint32_t k, uint32_t n) {
  const uint32_t W = 2 * k, lt = n, le = 0;
  std::vector<uint8_t> base(16);
  const Work w = carve(base.data(), k, n);  // the pointers are compared, never followed
  const Work z = carve(nullptr, k, n);
  CHECK(z.bytes == w.bytes && !z.head && !z.req);
  const uint8_t* b = base.data();
  CHECK(reinterpret_cast<uint8_t*>(w.head) == b);
  CHECK(reinterpret_cast<uint8_t*>(w.req) == b + kReqOff && kReqOff >= sizeof(Head) && kReqOff % 16 == 0);
  CHECK(reinterpret_cast<uint8_t*>(w.ns) >= reinterpret_cast<uint8_t*>(w.req) + w.npairs * sizeof(Request));
  CHECK(reinterpret_cast<uint8_t*>(w.pairs) >= reinterpret_cast<uint8_t*>(w.ns) + (size_t)n * 32);
  CHECK(reinterpret_cast<uint8_t*>(w.block_sums) >= reinterpret_cast<uint8_t*>(w.pairs) + w.npairs * sizeof(Pair));
  CHECK(w.bytes >= (size_t)(reinterpret_cast<uint8_t*>(w.block_sums) - b) + w.blocks * sizeof(Sums));
  CHECK((reinterpret_cast<uint8_t*>(w.pairs) - b) % 16 == 0 && (reinterpret_cast<uint8_t*>(w.ns) - b) % 16 == 0);
  CHECK(w.npairs == (uint64_t)n * W && w.blocks * kScanBlock >= w.npairs);
}

int main() {
  for (uint32_t W = 2; W <= 256; W *= 2) {
    const Counts c = check_width(W);
    std::printf("W = %3u: %6llu pairs, %6llu entries, %7llu nodes, %8llu shares\n", W, (unsigned long long)c.pairs,
                (unsigned long long)c.entries, (unsigned long long)c.nodes, (unsigned long long)c.leaves);
  }
  for (uint32_t k = 1; k <= 512; k *= 2)
    for (uint32_t n : {0u, 1u, 3u, 1024u}) check_carve(k, n);
  std::printf("namespace plan check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
