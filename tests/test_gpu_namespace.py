"""GPU: namespace queries on the tree index of a resident square (cel_dev_namespace_plan,
cel_dev_namespace_prove, cel_namespace_rows). Every entry, offset, node and share byte is checked
against the host mirror (proof.nmt_prove_namespace over proof.axis_trees, the path that was there
before); the outputs must stay inside the ranges the plan gives; inclusion batches go unchanged
into the device's inclusion verifier."""
import ctypes
import hashlib

import numpy as np
import pytest

import namespace_inputs as ni
import verify_cases as vc
from test_gpu_prove import Index

pytestmark = pytest.mark.gpu

P = vc._p
SENTINEL = 0x5A

# run lengths (row-major over the k x k ODS) that reach, for k = 4: a run from column 0, a run of 1
# inside a row, a run crossing a row end, a run ending at column k - 1 beside the parity half, and
# runs of exactly k covering whole rows (so the absent neighbour of the run before one of them
# falls between two rows' ranges); for k = 8 also a run covering a whole row and parts of two more
LAYOUTS = {1: [1], 2: [1, 2, 1], 4: [2, 1, 3, 2, 4, 4], 8: [3, 2, 5, 16, 1, 7, 8, 22]}
_cache = {}


def _square(oracle, ctx, k, runs=None, seed=None):
    """(ods, eds, row roots, present, absent, row trees on the host) of a square of runs."""
    from celestia_eds import proof
    from celestia_eds.rsmt2d import ExtendedDataSquare
    key = (k, seed)
    if key not in _cache:
        ods, present, absent = ni.run_ods(k, runs or LAYOUTS[k], 500 + k if seed is None else seed)
        eds, rr, cr, _ = oracle.extend_and_commit(ods)
        trees = proof.axis_trees(ExtendedDataSquare(eds, ctx=ctx), 0, 0, 2 * k)
        assert np.array_equal(trees[:, -1], rr)
        _cache[key] = (ods, eds, rr, present, absent, trees)
    return _cache[key]


def _queries(present, absent):
    return list(present) + list(absent) + [ni.BELOW_ALL, ni.ABOVE_ALL, present[0], absent[0], present[-1]]


class Plan:
    """cel_dev_namespace_plan into host arrays of `cap` entries, prefilled so that an entry the
    call did not write shows."""

    def __init__(self, idx, namespaces, cap=None, count_only=False):
        from hipmem import DeviceBuffer
        ctx = idx.ctx
        self.idx, self.n = idx, len(namespaces)
        self.ns = np.frombuffer(b"".join(namespaces) or b"\0", np.uint8).copy()
        size = ctx.lib.cel_dev_namespace_workspace_size(idx.k, self.n)
        assert size > 0
        self.d_work = DeviceBuffer(size + 64, fill=0xEE)
        self.cap = self.n * idx.w if cap is None else cap
        c = self.cap
        self.arr = dict(ns_idx=np.full(c, SENTINEL, np.uint32), rows=np.full(c, SENTINEL, np.uint32),
                        starts=np.full(c, SENTINEL, np.int32), ends=np.full(c, SENTINEL, np.int32),
                        kinds=np.full(c, SENTINEL, np.uint8), leaf_off=np.full(c + 1, SENTINEL, np.uint64),
                        node_off=np.full(c + 1, SENTINEL, np.uint64))
        self.count = ctypes.c_uint64(12345)
        ptrs = [None] * 7 if count_only else [P(self.arr[key]) for key in ("ns_idx", "rows", "starts", "ends", "kinds",
                                                                             "leaf_off", "node_off")]
        self.status = ctx.lib.cel_dev_namespace_plan(ctx.handle, idx.d_index.ptr, idx.k, self.n, P(self.ns),
                                                     0 if count_only else c, *ptrs, ctypes.byref(self.count),
                                                     self.d_work.ptr, None)
        self.error = ctx.lib.cel_last_error(ctx.handle).decode()
        # nothing behind the workspace's size is written
        assert (self.d_work.download_at(size, (64,)) == 0xEE).all()

    def entries(self):
        m = self.count.value
        return {key: v[:m + 1] if key.endswith("_off") else v[:m] for key, v in self.arr.items()}

    def untouched(self):
        return all((v == SENTINEL).all() for v in self.arr.values())

    def prove(self, node_shift=2, leaves=True, n_entries=None):
        """cel_dev_namespace_prove into 0xEE-filled buffers; d_nodes starts node_shift bytes into its
        buffer, so it is not dword aligned. Keeps the device buffers; returns (leaves, nodes)."""
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        idx, ctx = self.idx, self.idx.ctx
        e = self.entries()
        tl, tn = int(e["leaf_off"][-1]), int(e["node_off"][-1])
        self.d_leaves = DeviceBuffer(tl * 512 + 16, fill=0xEE)
        self.d_nodes = DeviceBuffer(node_shift + tn * 90 + 16, fill=0xEE)
        self.d_nodes_ptr = ctypes.c_void_p(self.d_nodes.ptr.value + node_shift)
        st = ctx.lib.cel_dev_namespace_prove(ctx.handle, idx.d_eds.ptr if leaves else None, idx.d_index.ptr, idx.k,
                                             self.count.value if n_entries is None else n_entries,
                                             self.d_leaves.ptr if leaves else None, self.d_nodes_ptr, self.d_work.ptr,
                                             None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        raw = self.d_nodes.download((self.d_nodes.nbytes,))
        assert (raw[:node_shift] == 0xEE).all() and (raw[node_shift + tn * 90:] == 0xEE).all(), "nodes outside their range"
        got = self.d_leaves.download((self.d_leaves.nbytes,))
        if leaves:
            assert (got[tl * 512:] == 0xEE).all(), "shares outside their range"
        else:
            assert (got == 0xEE).all()
        return got[:tl * 512].reshape(tl, 512), raw[node_shift:node_shift + tn * 90].reshape(tn, 90)


def _check_against_mirror(idx, trees, namespaces, node_shift=2):
    from celestia_eds import _lib
    want = ni.mirror_flat(trees, idx.cells, namespaces)
    plan = Plan(idx, namespaces)
    assert plan.status == _lib.OK, plan.error
    got = plan.entries()
    assert plan.count.value == len(want["rows"])
    for key in ("ns_idx", "rows", "starts", "ends", "kinds", "leaf_off", "node_off"):
        assert np.array_equal(got[key], want[key]), key
    m = plan.count.value  # nothing behind the entries is written
    assert all((v[m + (1 if key.endswith("_off") else 0):] == SENTINEL).all() for key, v in plan.arr.items())
    leaves, nodes = plan.prove(node_shift=node_shift)
    assert np.array_equal(nodes, want["nodes"]), "nodes differ"
    assert np.array_equal(leaves, want["leaves"]), "shares differ"
    return plan, want


# ------------------------------------------------------------- 1. parity with the mirror
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_entries_and_bytes_equal_mirror(ctx, oracle, k):
    from celestia_eds import _lib
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k)
    idx = Index(ctx, eds)
    queries = _queries(present, absent)
    plan, want = _check_against_mirror(idx, trees, queries)
    m = plan.count.value
    kinds = want["kinds"].tolist()
    if k >= 2:
        assert 0 in kinds and 1 in kinds
    # every present namespace: the union of its entries' shares is its shares of the ODS, in order
    flat = ods.reshape(-1, 512)
    leaves, _ = plan.prove(node_shift=6)
    for i, ns in enumerate(present):
        mine = [e for e in range(m) if want["ns_idx"][e] == i]
        assert mine and all(want["kinds"][e] == 0 for e in mine)
        got = np.concatenate([leaves[int(want["leaf_off"][e]):int(want["leaf_off"][e + 1])] for e in mine])
        assert np.array_equal(got, flat[(flat[:, :29] == np.frombuffer(ns, np.uint8)).all(axis=1)])
    # below all, above all: no entries; the duplicates repeat their first answers
    nq = len(queries)
    per = [[e for e in range(m) if want["ns_idx"][e] == i] for i in range(nq)]
    assert per[nq - 5] == [] and per[nq - 4] == []
    same = lambda a, b: [(want["rows"][e], want["starts"][e], want["ends"][e], want["kinds"][e]) for e in per[a]] == \
        [(want["rows"][e], want["starts"][e], want["ends"][e], want["kinds"][e]) for e in per[b]]
    assert same(nq - 3, 0) and same(nq - 2, len(present)) and same(nq - 1, len(present) - 1)
    if k == 4:
        # run 3 ends its row and run 4 begins the next: the namespace between them is in no row's range
        assert per[len(present) + 3] == [] and per[len(present) + 4] == []
        # run 1 (one share) is followed by run 2 in the same row: an absence entry there
        assert [want["kinds"][e] for e in per[len(present) + 1]] == [1]
    # count only
    cnt = Plan(idx, queries, count_only=True)
    assert cnt.status == _lib.OK and cnt.count.value == m and cnt.untouched()
    # cap one below the count
    if m:
        short = Plan(idx, queries, cap=m - 1)
        assert short.status == _lib.EINVAL and short.count.value == m and short.untouched()
        assert str(m - 1) in short.error and str(m) in short.error
    # nodes alone; fewer entries than the plan holds
    _, nodes = plan.prove(leaves=False)
    assert np.array_equal(nodes, want["nodes"])
    # no namespaces
    none = Plan(idx, [])
    assert none.status == _lib.OK and none.count.value == 0 and none.arr["leaf_off"][0] == 0 and none.arr["node_off"][0] == 0


def test_k32_seeded_runs(ctx, oracle):
    k = 32
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k, runs=ni.seeded_runs(k, 32, 3 * k), seed=3200)
    idx = Index(ctx, eds)
    _check_against_mirror(idx, trees, _queries(present, absent))
    # one namespace, and five: a workgroup holds four pairs and four entries
    _check_against_mirror(idx, trees, [present[3]], node_shift=4)
    _check_against_mirror(idx, trees, present[1:4] + absent[2:4])


# ------------------------------------------------------- 2. into the inclusion verifier
@pytest.mark.parametrize("k", [4, 32])
def test_inclusion_batch_feeds_device_verifier(ctx, oracle, k):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    runs = None if k == 4 else ni.seeded_runs(k, 32, 3 * k)
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k, runs=runs, seed=None if k == 4 else 3200)
    idx = Index(ctx, eds)
    plan = Plan(idx, present)
    assert plan.status == _lib.OK
    e = plan.entries()
    n = plan.count.value
    assert n >= len(present) and (e["kinds"] == 0).all()
    plan.prove()
    # byte for byte what cel_dev_prove_batch gives for the same ranges
    leaves, nodes, leaf_off, node_off = idx.prove([0] * n, e["rows"], e["starts"], e["ends"])
    assert np.array_equal(leaf_off, e["leaf_off"]) and np.array_equal(node_off, e["node_off"])
    assert np.array_equal(plan.d_leaves.download((len(leaves), 512)), leaves)
    assert np.array_equal(plan.d_nodes.download_at(2, (len(nodes), 90)), nodes)
    ns = np.stack([np.frombuffer(present[i], np.uint8) for i in e["ns_idx"]])
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(int(e["leaf_off"][-1]), int(e["node_off"][-1]), n))
    st = ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(e["starts"]), P(e["ends"]), P(ns), plan.d_leaves.ptr,
                                          P(e["leaf_off"]), plan.d_nodes_ptr, P(e["node_off"]), idx.d_roots.ptr, 2 * idx.w,
                                          P(e["rows"]), d_ok.ptr, d_work.ptr, None)
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    synchronize()
    assert (d_ok.download((n,)) == 1).all()


# ------------------------------------------------------------------------ 3. block 408
def test_block408_namespaces(ctx, oracle, block408_ods):
    from celestia_eds import _lib, proof
    ods = np.ascontiguousarray(block408_ods)
    eds, rr, cr, _ = oracle.extend_and_commit(ods)
    flat = ods.reshape(-1, 512)
    present = sorted({bytes(x) for x in flat[:, :29]} - {ni.PARITY})
    assert len(present) >= 2
    idx = Index(ctx, eds)
    plan = Plan(idx, present)
    assert plan.status == _lib.OK, plan.error
    e = plan.entries()
    leaves, nodes = plan.prove()
    for i, ns in enumerate(present):
        mine = [j for j in range(plan.count.value) if e["ns_idx"][j] == i]
        assert mine
        got = []
        for j in mine:
            assert e["kinds"][j] == 0
            p = proof.NMTProof(Start=int(e["starts"][j]), End=int(e["ends"][j]),
                               Nodes=[nodes[t].tobytes() for t in range(int(e["node_off"][j]), int(e["node_off"][j + 1]))])
            shares = [leaves[t].tobytes() for t in range(int(e["leaf_off"][j]), int(e["leaf_off"][j + 1]))]
            assert p.VerifyNamespace(ns, shares, rr[int(e["rows"][j])].tobytes())
            got += shares
        assert got == [x.tobytes() for x in flat[(flat[:, :29] == np.frombuffer(ns, np.uint8)).all(axis=1)]]


# ------------------------------------------------------------------------ 4. k = 128
def test_k128_batch_of_256(ctx, oracle):
    from celestia_eds import _lib
    k = 128
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k, runs=ni.seeded_runs(k, 128, 96), seed=12800)
    assert len(present) >= 128
    queries = present[:128] + absent[:128]
    idx = Index(ctx, eds)
    plan = Plan(idx, queries)
    assert plan.status == _lib.OK, plan.error
    leaves, nodes = plan.prove()
    want = ni.mirror_flat(trees, eds, queries)
    got = plan.entries()
    for key in ("ns_idx", "rows", "starts", "ends", "kinds", "leaf_off", "node_off"):
        assert np.array_equal(got[key], want[key]), key
    assert 1 in want["kinds"] and 0 in want["kinds"]
    assert hashlib.sha256(nodes.tobytes()).digest() == hashlib.sha256(want["nodes"].tobytes()).digest()
    assert hashlib.sha256(leaves.tobytes()).digest() == hashlib.sha256(want["leaves"].tobytes()).digest()


# ---------------------------------------------------------------- 5. an unordered square
def test_unordered_square_stays_in_bounds(ctx):
    """Arbitrary cells: no order among the leaves, roots that are no ranges. The counts are counts,
    so every entry lies inside its row and the outputs inside their ranges; the host entry point
    refuses the square."""
    from celestia_eds import _lib
    k, w = 8, 16
    rng = np.random.default_rng(77)
    cells = rng.integers(0, 256, (w, w, 512), dtype=np.uint8)
    vals = rng.integers(1, 12, (w, w))
    for r in range(w):
        for c in range(w):
            cells[r, c, :29] = np.frombuffer(ni.ns_value(int(vals[r, c])), np.uint8)
    cells[3, :, :29] = 0xFF                                       # a row of parity leaves alone
    cells[5, :, :29] = np.frombuffer(ni.ns_value(4), np.uint8)    # a row of one namespace
    idx = Index(ctx, cells)
    queries = [ni.ns_value(v) for v in range(0, 14)]
    plan = Plan(idx, queries)
    assert plan.status == _lib.OK, plan.error
    e = plan.entries()
    m = plan.count.value
    assert m > 0
    assert (e["starts"] >= 0).all() and (e["starts"] < w).all() and (e["ends"] > e["starts"]).all() and (e["ends"] <= w).all()
    assert (e["rows"] < w).all() and (e["ns_idx"] < len(queries)).all() and (e["kinds"] <= 1).all()
    assert (np.diff(e["leaf_off"].astype(np.int64)) == np.where(e["kinds"] == 0, e["ends"] - e["starts"], 0)).all()
    plan.prove()  # asserts the fill around the outputs
    # the counting rule itself, on any cells; a leaf's namespace is its share's inside the ODS
    # quadrant and the parity namespace elsewhere (the wrapper's rule)
    assert (e["rows"] < k).all()
    for j in range(m):
        q = queries[int(e["ns_idx"][j])]
        row = [cells[int(e["rows"][j]), c, :29].tobytes() if c < k else ni.PARITY for c in range(w)]
        lt, le = sum(x < q for x in row), sum(x <= q for x in row)
        assert (int(e["starts"][j]), int(e["ends"][j]), int(e["kinds"][j])) == ((lt, le, 0) if le > lt else (lt, lt + 1, 1))
    cnt = ctypes.c_uint64()
    tl, tn = ctypes.c_uint64(), ctypes.c_uint64()
    ns = np.frombuffer(b"".join(queries), np.uint8).copy()
    st = ctx.lib.cel_namespace_rows(ctx.handle, P(cells), k, len(queries), P(ns), 0, 0, 0, *([None] * 9),
                                    ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn))
    assert st == _lib.EORDER


# --------------------------------------------------------------------- 6. the host entry
def test_namespace_rows_host_entry(ctx, oracle):
    from celestia_eds import _lib
    k = 4
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k)
    queries = _queries(present, absent)
    want = ni.mirror_flat(trees, eds, queries)
    ns = np.frombuffer(b"".join(queries), np.uint8).copy()
    cnt, tl, tn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib, h = ctx.lib, ctx.handle
    tail = (ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn))
    assert lib.cel_namespace_rows(h, P(eds), k, len(queries), P(ns), 0, 0, 0, *([None] * 9), *tail) == _lib.OK
    m = len(want["rows"])
    assert (cnt.value, tl.value, tn.value) == (m, len(want["leaves"]), len(want["nodes"]))

    def call(cap, leaf_cap, node_cap):
        a = dict(ns_idx=np.full(m, SENTINEL, np.uint32), rows=np.full(m, SENTINEL, np.uint32),
                 starts=np.full(m, SENTINEL, np.int32), ends=np.full(m, SENTINEL, np.int32),
                 kinds=np.full(m, SENTINEL, np.uint8), leaf_off=np.full(m + 1, SENTINEL, np.uint64),
                 node_off=np.full(m + 1, SENTINEL, np.uint64), leaves=np.full((tl.value, 512), SENTINEL, np.uint8),
                 nodes=np.full((tn.value, 90), SENTINEL, np.uint8))
        st = lib.cel_namespace_rows(h, P(eds), k, len(queries), P(ns), cap, leaf_cap, node_cap,
                                    *[P(a[key]) for key in ("ns_idx", "rows", "starts", "ends", "kinds", "leaf_off",
                                                            "node_off", "leaves", "nodes")], *tail)
        return st, a

    st, a = call(m, tl.value, tn.value)
    assert st == _lib.OK, lib.cel_last_error(h).decode()
    for key, v in a.items():
        assert np.array_equal(v, want[key]), key
    for caps in ((m - 1, tl.value, tn.value), (m, tl.value - 1, tn.value), (m, tl.value, tn.value - 1)):
        st, a = call(*caps)
        assert st == _lib.EINVAL and all((v == SENTINEL).all() for v in a.values())
        assert cnt.value == m
    parity = np.full(29, 0xFF, np.uint8)
    assert lib.cel_namespace_rows(h, P(eds), k, 1, P(parity), 0, 0, 0, *([None] * 9), *tail) == _lib.EINVAL
    assert "parity" in lib.cel_last_error(h).decode()
    assert lib.cel_namespace_rows(h, None, k, 1, P(ns), 0, 0, 0, *([None] * 9), *tail) == _lib.EINVAL
    assert lib.cel_namespace_rows(h, P(eds), 3, 1, P(ns), 0, 0, 0, *([None] * 9), *tail) == _lib.EINVAL
    assert lib.cel_namespace_rows(h, P(eds), k, 0, None, 0, 0, 0, *([None] * 9), *tail) == _lib.OK and cnt.value == 0


# --------------------------------------------------------------------- 7. call errors
def test_plan_and_prove_call_errors(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer
    k = 2
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k)
    idx = Index(ctx, eds)
    lib, h = ctx.lib, ctx.handle
    d_work = DeviceBuffer(lib.cel_dev_namespace_workspace_size(k, 2))
    ns = np.frombuffer(present[0] + absent[0], np.uint8).copy()
    cnt = ctypes.c_uint64()
    arrs = [np.zeros(9, np.uint32), np.zeros(9, np.uint32), np.zeros(9, np.int32), np.zeros(9, np.int32),
            np.zeros(9, np.uint8), np.zeros(9, np.uint64), np.zeros(9, np.uint64)]

    def plan(handle=h, d_index=idx.d_index.ptr, k=k, n=2, ns=ns, cap=8, arrays=arrs, count=cnt, work=d_work.ptr):
        ptrs = [None if a is None else P(a) for a in arrays]
        return lib.cel_dev_namespace_plan(handle, d_index, k, n, None if ns is None else P(ns), cap, *ptrs,
                                          None if count is None else ctypes.byref(count), work, None)

    assert plan() == _lib.OK and cnt.value >= 1
    assert plan(handle=None) == _lib.EINVAL
    for kw in (dict(d_index=None), dict(ns=None), dict(count=None), dict(work=None), dict(arrays=arrs[:3] + [None] + arrs[4:]),
               dict(arrays=[None] * 7)):  # cap > 0 without arrays
        assert plan(**kw) == _lib.EINVAL, kw
        assert lib.cel_last_error(h).decode() == "nil argument"
    assert plan(work=ctypes.c_void_p(d_work.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in lib.cel_last_error(h).decode()
    assert plan(k=3) == _lib.EINVAL and plan(k=1024) == _lib.EINVAL
    bad = ns.copy()
    bad[29:] = 0xFF
    assert plan(ns=bad) == _lib.EINVAL and "namespace 1 is the parity namespace" in lib.cel_last_error(h).decode()
    assert plan(n=0, ns=None) == _lib.OK and cnt.value == 0
    assert plan(cap=0, arrays=[None] * 7) == _lib.OK and cnt.value >= 1

    assert plan() == _lib.OK
    m = cnt.value
    d_leaves, d_nodes = DeviceBuffer(1 << 16, fill=0xEE), DeviceBuffer(1 << 16, fill=0xEE)

    def prove(handle=h, d_eds=idx.d_eds.ptr, d_index=idx.d_index.ptr, k=k, m=m, leaves=d_leaves.ptr, nodes=d_nodes.ptr,
              work=d_work.ptr):
        return lib.cel_dev_namespace_prove(handle, d_eds, d_index, k, m, leaves, nodes, work, None)

    assert prove() == _lib.OK
    assert prove(handle=None) == _lib.EINVAL
    for kw in (dict(d_index=None), dict(nodes=None), dict(work=None), dict(d_eds=None)):
        assert prove(**kw) == _lib.EINVAL, kw
    assert prove(d_eds=None, leaves=None) == _lib.OK
    assert prove(leaves=ctypes.c_void_p(d_leaves.ptr.value + 8)) == _lib.EINVAL
    assert prove(nodes=ctypes.c_void_p(d_nodes.ptr.value + 1)) == _lib.EINVAL
    assert prove(k=3) == _lib.EINVAL and prove(m=0) == _lib.OK
