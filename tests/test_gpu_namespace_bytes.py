"""GPU: the namespace queries and the namespace verifier by namespace byte, by width and by plan
size (cel_dev_namespace_plan, cel_dev_namespace_prove, cel_namespace_rows,
cel_dev_nmt_verify_namespace_batch, cel_nmt_verify_namespace_batch, cel_dev_nmt_verify_batch).

The squares are no codewords: Q0 carries namespace_inputs.byte_ladder, whose neighbours are
decided at every one of the 29 bytes with the later bytes pointing the other way, and the other
quadrants are random. Every expected byte comes from hashlib trees (nmt_ref.Tree, ni.tree_table)
and from bytes comparisons (proof.nmt_prove_namespace, proof.verify_namespace, ni.pair_rule),
never from the device. tests/test_namespace_ladder.py checks, without a device, that the ladder
covers what these tests rely on."""
import ctypes
import hashlib

import numpy as np
import pytest

import namespace_inputs as ni
import verify_cases as vc
from test_gpu_namespace import SENTINEL, Plan
from test_gpu_namespace_verify import dev_batch, host_batch
from test_gpu_prove import Index

pytestmark = pytest.mark.gpu

P = vc._p
NS = ni.NS
KEYS = ("ns_idx", "rows", "starts", "ends", "kinds", "leaf_off", "node_off")
SEEDS = {8: 8, 32: 32}  # the ladders tests/test_namespace_ladder.py holds to their properties
_cache = {}


def _ladder(k):
    """The ladder square of width k, its part B queries and the mirror's answer over hashlib trees."""
    if k not in _cache:
        cells, nss, trans = ni.ladder_square(k, SEEDS[k])
        queries, notes = ni.ladder_queries(nss, trans)
        tables = ni.square_row_tables(cells)
        want = ni.mirror_flat(tables, cells, queries)
        for v in want.values():
            v.flags.writeable = False
        _cache[k] = dict(cells=cells, nss=nss, trans=trans, queries=queries, notes=notes, want=want,
                         roots=[t[-1].tobytes() for t in tables])
    return _cache[k]


def _free(*owners):
    """hipFree of every device buffer the owners hold (Index, Plan), now and not at collection."""
    from hipmem import DeviceBuffer
    for o in owners:
        for v in vars(o).values():
            if isinstance(v, DeviceBuffer):
                v.free()


def _plan_equals(idx, queries, want, node_shift=2):
    """Plan + prove of `queries` must give `want`, array for array and byte for byte."""
    from celestia_eds import _lib
    plan = Plan(idx, queries)
    assert plan.status == _lib.OK, plan.error
    m = plan.count.value
    assert m == len(want["rows"])
    got = plan.entries()
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert all((v[m + (1 if key.endswith("_off") else 0):] == SENTINEL).all() for key, v in plan.arr.items())
    leaves, nodes = plan.prove(node_shift=node_shift)
    assert np.array_equal(nodes, want["nodes"]), "nodes differ"
    assert np.array_equal(leaves, want["leaves"]), "shares differ"
    return plan


def _accepted_cases(k):
    """Every entry of the mirror's plan in the verifier's form, and the empty proof of every
    (query, row) without an entry against that row's hashlib root: all valid by construction."""
    sq = _ladder(k)
    if "cases" not in sq:
        want, queries, roots = sq["want"], sq["queries"], sq["roots"]
        lo, no = want["leaf_off"].tolist(), want["node_off"].tolist()
        entries = []
        for e, (i, r, s, t, kind) in enumerate(zip(want["ns_idx"].tolist(), want["rows"].tolist(), want["starts"].tolist(),
                                                   want["ends"].tolist(), want["kinds"].tolist())):
            entries.append(ni.NsCase(f"query {i} row {r}", s, t, kind, queries[i],
                                     [want["leaves"][j].tobytes() for j in range(lo[e], lo[e + 1])],
                                     [want["nodes"][j].tobytes() for j in range(no[e], no[e + 1])], roots[r], True))
        have = set(zip(want["ns_idx"].tolist(), want["rows"].tolist()))
        empties = [ni.NsCase(f"query {i} row {r}, empty", 0, 0, 0, q, [], [], roots[r], True)
                   for i, q in enumerate(queries) for r in range(2 * k) if (i, r) not in have]
        sq["cases"] = (entries, empties)
    return sq["cases"]


# ------------------------------------------------------- 1. plan and proofs, byte by byte
@pytest.mark.parametrize("k", [8, 32])
def test_plan_and_proofs_by_byte(ctx, k):
    from celestia_eds import _lib
    sq = _ladder(k)
    cells, queries, want = sq["cells"], sq["queries"], sq["want"]
    assert 0 in want["kinds"] and 1 in want["kinds"]
    idx = Index(ctx, cells)
    assert [r.tobytes() for r in idx.rr] == sq["roots"], "the index's row roots are not hashlib's"
    _plan_equals(idx, queries, want)
    if k == 8:  # the same queries over the square in host memory
        lib, h = ctx.lib, ctx.handle
        m, tl, tn = len(want["rows"]), len(want["leaves"]), len(want["nodes"])
        a = dict(ns_idx=np.full(m, SENTINEL, np.uint32), rows=np.full(m, SENTINEL, np.uint32),
                 starts=np.full(m, SENTINEL, np.int32), ends=np.full(m, SENTINEL, np.int32),
                 kinds=np.full(m, SENTINEL, np.uint8), leaf_off=np.full(m + 1, SENTINEL, np.uint64),
                 node_off=np.full(m + 1, SENTINEL, np.uint64), leaves=np.full((tl, 512), SENTINEL, np.uint8),
                 nodes=np.full((tn, 90), SENTINEL, np.uint8))
        ns = np.frombuffer(b"".join(queries), np.uint8).copy()
        cnt, cl, cn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        st = lib.cel_namespace_rows(h, P(cells), k, len(queries), P(ns), m, tl, tn,
                                    *[P(a[key]) for key in KEYS + ("leaves", "nodes")], ctypes.byref(cnt),
                                    ctypes.byref(cl), ctypes.byref(cn))
        assert st == _lib.OK, lib.cel_last_error(h).decode()
        assert (cnt.value, cl.value, cn.value) == (m, tl, tn)
        for key, v in a.items():
            assert np.array_equal(v, want[key]), key
    _free(idx)


# ---------------------------------------------------- 2. the verifier accepts, byte by byte
def test_verifier_accepts_by_byte(ctx):
    """A wrong compare shows here as a valid proof refused: sibling completeness, absence
    (leaf.min > nid), the empty proof's range test and verify_hash_node's max namespace are all
    decided at byte b of some proof, for every b; the N_b rows are one word from parity."""
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    k = 32
    sq = _ladder(k)
    entries, empties = _accepted_cases(k)
    kinds = [c.kind for c in entries]
    assert kinds.count(0) >= NS and kinds.count(1) >= NS and len(empties) >= NS
    for c in entries + empties:
        assert c.mirror() is True, c.name
    for cases in (entries, empties):
        got = dev_batch(ctx, cases)
        assert [c.name for c, v in zip(cases, got) if not v] == []
        got = host_batch(ctx, cases)
        assert [c.name for c, v in zip(cases, got) if not v] == []
    # the inclusion entries through the range verifier, which shares verify_hash_node
    idx = Index(ctx, sq["cells"])
    present = [q for q, note in zip(sq["queries"], sq["notes"]) if note[0] == "present"]
    plan = Plan(idx, present)
    assert plan.status == _lib.OK, plan.error
    e = plan.entries()
    n = plan.count.value
    assert n >= len(present) and (e["kinds"] == 0).all() and int(e["leaf_off"][-1]) == k * k
    plan.prove()
    ns = np.stack([np.frombuffer(present[i], np.uint8) for i in e["ns_idx"]])
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(int(e["leaf_off"][-1]), int(e["node_off"][-1]), n))
    st = ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(e["starts"]), P(e["ends"]), P(ns), plan.d_leaves.ptr,
                                          P(e["leaf_off"]), plan.d_nodes_ptr, P(e["node_off"]), idx.d_roots.ptr, 2 * idx.w,
                                          P(e["rows"]), d_ok.ptr, d_work.ptr, None)
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    synchronize()
    assert (d_ok.download((n,)) == 1).all()
    _free(idx, plan)


# ---------------------------------------------------- 3. the verifier rejects, byte by byte
def _reject_cases():
    """For every byte b, the neighbours x < y of a ladder transition decided at b, on a row of
    eight leaves x x y y and four parity leaves: accepted proofs and rejected ones, each with its
    verdict by construction."""
    import nmt_ref
    sq = _ladder(32)
    near = {ni.near_parity(b) for b in range(NS)}
    rng = np.random.default_rng(3)
    out = []
    add = lambda *a: out.append(ni.NsCase(*a))
    for b in range(NS):
        x, y = next((x, y) for _, tb, x, y in sq["trans"]
                    if tb == b and y not in near and (b == NS - 1 or x[b + 1] > y[b + 1]) and ni.absentees(x, y, b))
        nss = [x, x, y, y] + [ni.PARITY] * 4
        bodies = [rng.integers(0, 256, ni.SHARE, dtype=np.uint8).tobytes() for _ in range(8)]
        shares = [ns + body[NS:] if ns != ni.PARITY else body for ns, body in zip(nss, bodies)]
        tree = nmt_ref.Tree.from_shares(nss, shares)
        root, rec, pr = tree.root(), tree.leaves, tree.prove_range
        assert root[:NS] == x and root[NS:2 * NS] == y
        between = ni.absentees(x, y, b)
        above_x, below_y = between[0], between[-1]
        add(f"b{b} inclusion of x", 0, 2, 0, x, shares[0:2], pr(0, 2), root, True)
        add(f"b{b} inclusion of y", 2, 4, 0, y, shares[2:4], pr(2, 4), root, True)
        add(f"b{b} absence above x", 2, 3, 1, above_x, [], pr(2, 3) + [rec[2]], root, True)
        add(f"b{b} absence below y", 2, 3, 1, below_y, [], pr(2, 3) + [rec[2]], root, True)
        add(f"b{b} empty proof below the root", 0, 0, 0, ni.BELOW_ALL, [], [], root, True)
        # a share whose prefix byte b is the neighbour's, in a tree hashed under the claimed
        # namespaces: the root matches, the prefix test alone can object
        for at, mine, other, rng_ in ((1, x, y, (0, 2)), (2, y, x, (2, 4))):
            odd = list(shares)
            odd[at] = mine[:b] + other[b:b + 1] + shares[at][b + 1:]
            assert odd[at][:NS] != mine and odd[at][:b] == mine[:b] and odd[at][b + 1:NS] == mine[b + 1:]
            t2 = nmt_ref.Tree.from_shares(nss, odd)
            add(f"b{b} prefix byte of leaf {at}", rng_[0], rng_[1], 0, mine, odd[rng_[0]:rng_[1]],
                t2.prove_range(*rng_), t2.root(), False)
        add(f"b{b} x's proof for the absentee above it", 0, 2, 0, above_x, shares[0:2], pr(0, 2), root, False)
        add(f"b{b} absence with leaf hash min == nid", 2, 3, 1, y, [], pr(2, 3) + [rec[2]], root, False)
        add(f"b{b} empty proof at the root's min", 0, 0, 0, x, [], [], root, False)
        add(f"b{b} empty proof at the root's max", 0, 0, 0, y, [], [], root, False)
        add(f"b{b} empty proof a step above the min", 0, 0, 0, above_x, [], [], root, False)
        add(f"b{b} empty proof a step below the max", 0, 0, 0, below_y, [], [], root, False)
    return out


def test_verifier_rejects_by_byte(ctx):
    cases = _reject_cases()
    entries, empties = _accepted_cases(32)
    batch = []
    for j, c in enumerate(cases):  # an accepted proof of the ladder square after every third case
        batch.append(c)
        if j % 3 == 2:
            batch.append(entries[(7 * j) % len(entries)] if j % 2 else empties[(11 * j) % len(empties)])
    want = [c.want for c in batch]
    assert want.count(True) >= NS and want.count(False) >= NS
    for b in range(NS):
        assert sum(1 for c in cases if c.name.startswith(f"b{b} ") and not c.want) == 8
    for c in batch:
        assert c.mirror() is c.want, c.name
    got = dev_batch(ctx, batch)
    assert [c.name for c, v in zip(batch, got) if v is not c.want] == []
    assert dev_batch(ctx, batch, node_shift=1) == got
    assert host_batch(ctx, batch) == got


# ------------------------------------------------------------------------ 4. widths
def _width_queries(k, nss, trans, seed):
    """24 present and 24 absent namespaces and the two outside, by seed: among the present the
    first and the last namespace of one row and, where the layout has one, a namespace that fills
    a whole row."""
    rng = np.random.default_rng(seed)
    rows = [nss[r * k:(r + 1) * k] for r in range(k)]
    r0 = int(rng.integers(0, k))
    ends = next(rows[r % k] for r in range(r0, r0 + k) if rows[r % k][0] != rows[r % k][-1])
    full = [row[0] for row in rows if row[0] == row[-1]]
    distinct = sorted(set(nss))
    present = []
    for x in [ends[0], ends[-1]] + full[:1] + [distinct[i] for i in rng.permutation(len(distinct))]:
        if len(present) < 24 and x not in present:
            present.append(x)
    absent = [q for _, b, x, y in trans for q in ni.absentees(x, y, b)]
    absent = [absent[i] for i in sorted(rng.permutation(len(absent))[:24])]
    assert len(present) == 24 and len(absent) == 24
    return present + absent + [ni.BELOW_ALL, ni.ABOVE_LADDER], bool(full)


def _check_width(ctx, k):
    from celestia_eds import _lib
    w = 2 * k
    cells, nss, trans = ni.ladder_square(k, 1000 + k, longest=3 * k if k >= 64 else 3)
    queries, has_full = _width_queries(k, nss, trans, k)
    assert has_full or k < 64
    rows = [nss[r * k:(r + 1) * k] for r in range(k)]
    # every (query, row) pair by the counting rule; rows k .. 2k - 1 hold parity alone
    want = [(i, r) + ni.pair_rule(rows[r], q, w) for i, q in enumerate(queries) for r in range(k)
            if ni.pair_rule(rows[r], q, w)]
    kinds = [t[4] for t in want]
    assert kinds.count(0) >= 24 and kinds.count(1) >= 12
    if k >= 64:
        spans = {}
        for t in want:
            spans[t[0]] = spans.get(t[0], 0) + (t[4] == 0)
        assert max(spans.values()) >= 2  # a namespace that spans rows
    trees, nodes, leaves, leaf_off, node_off = {}, [], [], [0], [0]
    for i, r, s, e, kind in want:  # hashlib trees of the rows that have entries, no others
        if r not in trees:
            trees[r] = ni.square_row_tree(cells, r)
        nodes += trees[r].prove_range(s, e) + ([trees[r].leaves[s]] if kind else [])
        if not kind:
            leaves.append(cells[r, s:e])
        leaf_off.append(leaf_off[-1] + (0 if kind else e - s))
        node_off.append(node_off[-1] + len(trees[r].prove_range(s, e)) + kind)
    cols = list(zip(*want))
    ref = dict(ns_idx=np.array(cols[0], np.uint32), rows=np.array(cols[1], np.uint32), starts=np.array(cols[2], np.int32),
               ends=np.array(cols[3], np.int32), kinds=np.array(cols[4], np.uint8), leaf_off=np.array(leaf_off, np.uint64),
               node_off=np.array(node_off, np.uint64), leaves=np.concatenate(leaves),
               nodes=np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 90))
    idx = Index(ctx, cells)
    try:
        for r, t in trees.items():
            assert idx.rr[r].tobytes() == t.root(), f"row root {r}"
        plan = _plan_equals(idx, queries, ref)
        if k == 64:  # the same ranges through the batch prover, above W = 64 for the first time
            got_leaves, got_nodes, lo, no = idx.prove([0] * len(want), ref["rows"], ref["starts"], ref["ends"])
            by_range = b"".join(x for _, r, s, e, _ in want for x in trees[r].prove_range(s, e))
            assert got_nodes.tobytes() == by_range
            assert np.array_equal(got_leaves, np.concatenate([cells[r, s:e] for _, r, s, e, _ in want]))
        _free(plan)
    finally:
        _free(idx)


@pytest.mark.parametrize("k", [16, 64, 256])
def test_widths(ctx, k):
    """k = 16: half a wave of rows and of leaves in the find kernel; k = 64: two groups of 64
    rows per namespace; k = 256: a GF(2^16) width."""
    _check_width(ctx, k)


def test_k512(ctx):
    """The widest square the plan admits: a 512 MiB upload and an index of about 400 MB, freed
    before the test returns."""
    _check_width(ctx, 512)


# ------------------------------------------------- 5. the prefix sum past one slice per lane
def _scan_square():
    if "scan" not in _cache:
        k = 64
        cells, nss, trans = ni.ladder_square(k, 6400)
        distinct = sorted(set(nss))
        inner = [q for pos, b, x, y in trans if pos % k for q in ni.absentees(x, y, b)]  # between two leaves of a row
        base = []
        for j in range(150):
            base += [distinct[j * len(distinct) // 150], inner[j * len(inner) // 150]]
        rank = {v: i for i, v in enumerate(sorted(set(distinct) | set(base)))}
        trees = [ni.square_row_tree(cells, r) for r in range(k)]
        _cache["scan"] = dict(cells=cells, base=base, rank=rank, trees=trees,
                              ranks=np.array([rank[x] for x in nss], np.int64).reshape(k, k))
    return _cache["scan"]


@pytest.mark.parametrize("n", [514, 1030])
def test_scan_past_one_slice(ctx, n):
    """k_ns_scan gives lane t of 256 the block sums [t * per, min((t + 1) * per, blocks)), per =
    ceil(blocks / 256), a block being 256 pairs. At k = 64 (W = 128):
      n = 514:  65,792 pairs = 257 blocks, per = 2: lanes 0 .. 127 hold two blocks, lane 128 holds
                one (its slice is cut short by `blocks`), lanes 129 .. 255 get nothing (the clamp);
      n = 1030: 131,840 pairs = 515 blocks, per = 3: lanes 0 .. 170 hold three, lane 171 two.
    Every block of the reference holds an entry, so a wrong base of any slice moves an offset."""
    from celestia_eds import _lib
    k, W, L, block = 64, 128, 7, 256
    npairs = n * W
    blocks = -(-npairs // block)
    per = -(-blocks // 256)
    assert (npairs, blocks, per) == {514: (65792, 257, 2), 1030: (131840, 515, 3)}[n]
    last = (blocks - 1) // per  # the last lane that holds anything
    assert (last, blocks - last * per) == {514: (128, 1), 1030: (171, 2)}[n]
    sq = _scan_square()
    cells, ranks = sq["cells"], sq["ranks"]
    queries = [sq["base"][i % len(sq["base"])] for i in range(n)]
    q = np.array([sq["rank"][x] for x in queries], np.int64)
    # the counting rule on ranks: lt / le of every (query, row); rows 64 .. 127 hold parity alone
    lt, le, inside = (np.zeros((n, W), np.int64) for _ in range(3))
    for r in range(k):
        lt[:, r] = np.searchsorted(ranks[r], q, "left")
        le[:, r] = np.searchsorted(ranks[r], q, "right")
        inside[:, r] = (ranks[r, 0] <= q) & (q <= ranks[r, -1])
    entry = inside.astype(bool)
    pad = np.zeros(blocks * block, bool)
    pad[:npairs] = entry.reshape(-1)
    assert pad.reshape(blocks, block).any(axis=1).all() and entry.sum() >= n
    ns_idx, rows = np.nonzero(entry)
    starts = lt[entry]
    kinds = (le[entry] == starts).astype(np.int64)
    ends = np.where(kinds == 1, starts + 1, le[entry])
    pop = np.array([bin(v).count("1") for v in range(W + 1)], np.int64)
    nnodes = pop[starts] + L - pop[ends - 1] + kinds
    nleaves = np.where(kinds == 1, 0, ends - starts)
    ref = dict(ns_idx=ns_idx.astype(np.uint32), rows=rows.astype(np.uint32), starts=starts.astype(np.int32),
               ends=ends.astype(np.int32), kinds=kinds.astype(np.uint8),
               leaf_off=np.concatenate([[0], np.cumsum(nleaves)]).astype(np.uint64),
               node_off=np.concatenate([[0], np.cumsum(nnodes)]).astype(np.uint64))
    memo, nodes, leaves = {}, [], []
    for r, s, e, kind in zip(rows.tolist(), starts.tolist(), ends.tolist(), kinds.tolist()):
        if (r, s, e, kind) not in memo:
            t = sq["trees"][r]
            memo[r, s, e, kind] = (b"".join(t.prove_range(s, e) + ([t.leaves[s]] if kind else [])),
                                   b"" if kind else cells[r, s:e].tobytes())
        nodes.append(memo[r, s, e, kind][0])
        leaves.append(memo[r, s, e, kind][1])
    nodes, leaves = b"".join(nodes), b"".join(leaves)
    assert len(nodes) == 90 * int(ref["node_off"][-1]) and len(leaves) == 512 * int(ref["leaf_off"][-1])
    idx = Index(ctx, cells)
    plan = Plan(idx, queries)
    assert plan.status == _lib.OK, plan.error
    m = plan.count.value
    assert m == len(rows)
    got = plan.entries()
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), key
    assert all((v[m + (1 if key.endswith("_off") else 0):] == SENTINEL).all() for key, v in plan.arr.items())
    got_leaves, got_nodes = plan.prove()
    assert hashlib.sha256(got_nodes.tobytes()).digest() == hashlib.sha256(nodes).digest()
    assert hashlib.sha256(got_leaves.tobytes()).digest() == hashlib.sha256(leaves).digest()
    if n == 1030:
        cnt = Plan(idx, queries, count_only=True)
        assert cnt.status == _lib.OK and cnt.count.value == m and cnt.untouched()
        short = Plan(idx, queries, cap=m - 1)
        assert short.status == _lib.EINVAL and short.count.value == m and short.untouched()
        _free(cnt, short)
    _free(idx, plan)
