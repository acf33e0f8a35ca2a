"""GPU: namespace queries over the batch tree index of many resident squares
(cel_dev_namespace_plan_squares, cel_dev_namespace_prove_squares, cel_namespace_rows_squares,
rsmt2d.SharesByNamespaceBatch). A query is a (square, namespace) pair. The reference is the
single-square path on each square's own index (Plan of test_gpu_namespace, itself checked against
the host mirror there): every entry, offset, node and share byte of the batch equals the
per-square plan and prove output, put in (query, row) order."""
import ctypes

import numpy as np
import pytest

import namespace_inputs as ni
import verify_cases as vc
from test_gpu_index_batch import BatchIndex
from test_gpu_namespace import LAYOUTS, SENTINEL, Plan
from test_gpu_prove import Index

pytestmark = pytest.mark.gpu

P = vc._p
KEYS = ("query_idx", "rows", "starts", "ends", "kinds", "leaf_off", "node_off")


def _relabel(ods, old, new):
    """Every share of namespace `old` gets namespace `new` (which keeps the order)."""
    flat = ods.reshape(-1, 512)
    hit = (flat[:, :29] == np.frombuffer(old, np.uint8)).all(axis=1)
    assert hit.any()
    flat[hit, :29] = np.frombuffer(new, np.uint8)


def _three_squares(oracle, k, runs=None, seed=0):
    """Three squares of runs: the layout, the layout reversed (the same namespaces elsewhere), and
    the layout with its second namespace moved up by one: namespace 4 is in squares 0 and 1 and
    absent from square 2, namespace 5 is in square 2 alone. [(cells, present, absent)]."""
    runs = runs or LAYOUTS[k]
    out = []
    for i, r in enumerate((runs, runs[::-1], runs)):
        ods, present, absent = ni.run_ods(k, list(r), 800 + 10 * k + seed + i)
        if i == 2:
            _relabel(ods, present[1], absent[1])
            present, absent = [absent[1] if j == 1 else p for j, p in enumerate(present)], \
                              [present[1] if j == 1 else a for j, a in enumerate(absent)]
        out.append((oracle.extend_and_commit(ods)[0], present, absent))
    return out


class PlanSquares:
    """cel_dev_namespace_plan_squares into host arrays of `cap` entries, prefilled so that an entry
    the call did not write shows; then cel_dev_namespace_prove_squares into guarded buffers."""

    def __init__(self, batch, queries, cap=None, count_only=False):
        from hipmem import DeviceBuffer
        ctx = batch.ctx
        self.batch, self.n = batch, len(queries)
        self.sq = np.array([q for q, _ in queries] or [0], np.uint32)
        self.ns = np.frombuffer(b"".join(ns for _, ns in queries) or b"\0", np.uint8).copy()
        size = ctx.lib.cel_dev_namespace_squares_workspace_size(batch.k, self.n)
        assert size > 0
        self.d_work = DeviceBuffer(size + 64, fill=0xEE)
        self.cap = self.n * batch.w if cap is None else cap
        c = self.cap
        self.arr = dict(query_idx=np.full(c, SENTINEL, np.uint32), rows=np.full(c, SENTINEL, np.uint32),
                        starts=np.full(c, SENTINEL, np.int32), ends=np.full(c, SENTINEL, np.int32),
                        kinds=np.full(c, SENTINEL, np.uint8), leaf_off=np.full(c + 1, SENTINEL, np.uint64),
                        node_off=np.full(c + 1, SENTINEL, np.uint64))
        self.count = ctypes.c_uint64(12345)
        ptrs = [None] * 7 if count_only else [P(self.arr[key]) for key in KEYS]
        self.status = ctx.lib.cel_dev_namespace_plan_squares(ctx.handle, batch.d_index.ptr, batch.k, batch.n, self.n,
                                                             P(self.sq), P(self.ns), 0 if count_only else c, *ptrs,
                                                             ctypes.byref(self.count), self.d_work.ptr, None)
        self.error = ctx.lib.cel_last_error(ctx.handle).decode()
        assert (self.d_work.download_at(size, (64,)) == 0xEE).all(), "the plan outside its workspace"

    def entries(self):
        m = self.count.value
        return {key: v[:m + 1] if key.endswith("_off") else v[:m] for key, v in self.arr.items()}

    def untouched(self):
        return all((v == SENTINEL).all() for v in self.arr.values())

    def prove(self, node_shift=2, leaves=True):
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        batch, ctx = self.batch, self.batch.ctx
        e = self.entries()
        tl, tn = int(e["leaf_off"][-1]), int(e["node_off"][-1])
        self.d_leaves = DeviceBuffer(tl * 512 + 16, fill=0xEE)
        self.d_nodes = DeviceBuffer(node_shift + tn * 90 + 16, fill=0xEE)
        self.d_nodes_ptr = ctypes.c_void_p(self.d_nodes.ptr.value + node_shift)
        st = ctx.lib.cel_dev_namespace_prove_squares(ctx.handle, batch.d_eds.ptr if leaves else None, batch.d_index.ptr,
                                                     batch.k, batch.n, self.count.value,
                                                     self.d_leaves.ptr if leaves else None, self.d_nodes_ptr,
                                                     self.d_work.ptr, None)
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


def _expected(singles, queries):
    """The per-square Plan and prove output of each square's queries, in (query, row) order."""
    from celestia_eds import _lib
    by_query = [[] for _ in queries]
    for sq in sorted({q for q, _ in queries}):
        ids = [i for i, (q, _) in enumerate(queries) if q == sq]
        plan = Plan(singles[sq], [queries[i][1] for i in ids])
        assert plan.status == _lib.OK, plan.error
        leaves, nodes = plan.prove()
        e = plan.entries()
        for j in range(plan.count.value):
            by_query[ids[int(e["ns_idx"][j])]].append(
                (int(e["rows"][j]), int(e["starts"][j]), int(e["ends"][j]), int(e["kinds"][j]),
                 leaves[int(e["leaf_off"][j]):int(e["leaf_off"][j + 1])], nodes[int(e["node_off"][j]):int(e["node_off"][j + 1])]))
    flat = [(i,) + ent for i, ents in enumerate(by_query) for ent in ents]
    out = dict(query_idx=np.array([f[0] for f in flat], np.uint32), rows=np.array([f[1] for f in flat], np.uint32),
               starts=np.array([f[2] for f in flat], np.int32), ends=np.array([f[3] for f in flat], np.int32),
               kinds=np.array([f[4] for f in flat], np.uint8))
    out["leaf_off"] = np.cumsum([0] + [len(f[5]) for f in flat]).astype(np.uint64)
    out["node_off"] = np.cumsum([0] + [len(f[6]) for f in flat]).astype(np.uint64)
    out["leaves"] = np.concatenate([f[5] for f in flat] + [np.zeros((0, 512), np.uint8)])
    out["nodes"] = np.concatenate([f[6] for f in flat] + [np.zeros((0, 90), np.uint8)])
    return out


def _check(batch, singles, queries, node_shift=2):
    from celestia_eds import _lib
    want = _expected(singles, queries)
    plan = PlanSquares(batch, queries)
    assert plan.status == _lib.OK, plan.error
    got = plan.entries()
    m = plan.count.value
    assert m == len(want["rows"])
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert all((v[m + (1 if key.endswith("_off") else 0):] == SENTINEL).all() for key, v in plan.arr.items())
    leaves, nodes = plan.prove(node_shift=node_shift)
    assert np.array_equal(nodes, want["nodes"]), "nodes differ"
    assert np.array_equal(leaves, want["leaves"]), "shares differ"
    return plan, want


def _mixed_queries(squares, seed):
    """Present and absent namespaces of every square asked of every square, the namespaces below
    and above all, duplicates; shuffled."""
    names = sorted({ns for _, present, absent in squares for ns in present + absent} | {ni.BELOW_ALL, ni.ABOVE_ALL})
    queries = [(sq, ns) for ns in names for sq in range(len(squares))]
    queries += [queries[0], queries[5], queries[0], (2, squares[2][1][1]), (0, squares[2][1][1])]
    return [queries[i] for i in np.random.default_rng(seed).permutation(len(queries))]


# ------------------------------------------------------------ 5. parity with the single plans
@pytest.mark.parametrize("k", [2, 4, 8])
def test_entries_and_bytes_equal_single_plans(ctx, oracle, k):
    from celestia_eds import _lib
    squares = _three_squares(oracle, k)
    batch = BatchIndex(ctx, [s[0] for s in squares], flags=_lib.FLAG_ORDER_CHECK)
    assert batch.status == [_lib.OK] * 3
    singles = [Index(ctx, s[0]) for s in squares]
    queries = _mixed_queries(squares, k)
    plan, want = _check(batch, singles, queries)
    assert 0 in want["kinds"] and 1 in want["kinds"]
    # the namespace that squares 0 and 1 hold and square 2 lacks, and the one square 2 holds alone
    moved_from, moved_to = squares[0][1][1], squares[2][1][1]
    kinds_of = lambda q: {int(want["kinds"][e]) for e in range(len(want["rows"])) if queries[int(want["query_idx"][e])] == q}
    assert kinds_of((0, moved_from)) == {0} and kinds_of((1, moved_from)) == {0} and kinds_of((2, moved_from)) == {1}
    assert kinds_of((2, moved_to)) == {0} and kinds_of((0, moved_to)) == {1}
    m = plan.count.value
    # count only, and a cap one below the count
    count = PlanSquares(batch, queries, count_only=True)
    assert count.status == _lib.OK and count.count.value == m and count.untouched()
    short = PlanSquares(batch, queries, cap=m - 1)
    assert short.status == _lib.EINVAL and short.count.value == m and short.untouched()
    assert short.error == f"cap {m - 1} is below the {m} entries of the plan"
    # one query, and five: a workgroup holds four waves
    _check(batch, singles, [(2, moved_to)], node_shift=4)
    _check(batch, singles, queries[:5])
    # nodes alone
    _, nodes = plan.prove(leaves=False, node_shift=6)
    assert np.array_equal(nodes, want["nodes"])
    # all queries on one square: the single plan's entries
    only = [(1, ns) for _, ns in queries[:9]]
    plan1, _ = _check(batch, singles, only)
    single = Plan(singles[1], [ns for _, ns in only])
    for a, b in zip(KEYS, ("ns_idx",) + KEYS[1:]):
        assert np.array_equal(plan1.entries()[a], single.entries()[b])
    none = PlanSquares(batch, [])
    assert none.status == _lib.OK and none.count.value == 0 and none.arr["leaf_off"][0] == 0 and none.arr["node_off"][0] == 0


def test_k32_seeded_runs(ctx, oracle):
    from celestia_eds import _lib
    k = 32
    squares = _three_squares(oracle, k, runs=ni.seeded_runs(k, 32, 3 * k), seed=3200)
    batch = BatchIndex(ctx, [s[0] for s in squares], flags=_lib.FLAG_ORDER_CHECK)
    assert batch.status == [_lib.OK] * 3
    singles = [Index(ctx, s[0]) for s in squares]
    rng = np.random.default_rng(32)
    queries = []
    for sq, (_, present, absent) in enumerate(squares):
        queries += [(sq, present[i]) for i in rng.integers(0, len(present), 6)] + \
                   [(sq, absent[i]) for i in rng.integers(0, len(absent), 4)] + [(sq, ni.BELOW_ALL), (sq, ni.ABOVE_ALL)]
    queries += [(2, squares[2][1][1]), (0, squares[2][1][1]), (1, squares[0][1][1])]
    queries = [queries[i] for i in rng.permutation(len(queries))]
    _, want = _check(batch, singles, queries)
    assert 0 in want["kinds"] and 1 in want["kinds"]


def test_inclusion_batch_feeds_device_verifier(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    k = 4
    squares = _three_squares(oracle, k)
    batch = BatchIndex(ctx, [s[0] for s in squares])
    queries = [(sq, ns) for sq, (_, present, _) in enumerate(squares) for ns in present]
    plan = PlanSquares(batch, queries)
    assert plan.status == _lib.OK
    e = plan.entries()
    n = plan.count.value
    assert n >= len(queries) and (e["kinds"] == 0).all()
    plan.prove()
    sq = np.array([queries[int(q)][0] for q in e["query_idx"]], np.uint32)
    ns = np.stack([np.frombuffer(queries[int(q)][1], np.uint8) for q in e["query_idx"]])
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(int(e["leaf_off"][-1]), int(e["node_off"][-1]), n))
    for square_of, verdict in ((sq, 1), ((sq + 1) % 3, 0)):
        root_idx = (square_of * batch.w + e["rows"]).astype(np.uint32)  # the row roots lie first: [n][2k]
        st = ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(e["starts"]), P(e["ends"]), P(ns), plan.d_leaves.ptr,
                                              P(e["leaf_off"]), plan.d_nodes_ptr, P(e["node_off"]), batch.d_roots.ptr,
                                              2 * 3 * batch.w, P(root_idx), d_ok.ptr, d_work.ptr, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        assert (d_ok.download((n,)) == verdict).all()


def test_unordered_squares_stay_in_bounds(ctx):
    """Two squares of arbitrary cells: no order among the leaves, roots that are no ranges. Every
    entry lies inside its row and the outputs inside the plan's ranges (the guards of PlanSquares),
    and the batch still equals the per-square plans."""
    from celestia_eds import _lib
    k, w = 8, 16
    cells = []
    for seed in (77, 78):
        rng = np.random.default_rng(seed)
        c = rng.integers(0, 256, (w, w, 512), dtype=np.uint8)
        vals = rng.integers(1, 12, (w, w))
        for r in range(w):
            for col in range(w):
                c[r, col, :29] = np.frombuffer(ni.ns_value(int(vals[r, col])), np.uint8)
        c[3 + seed % 2, :, :29] = 0xFF
        c[5, :, :29] = np.frombuffer(ni.ns_value(4 + seed % 2), np.uint8)
        cells.append(c)
    batch = BatchIndex(ctx, cells, flags=_lib.FLAG_ORDER_CHECK)
    assert batch.status == [_lib.EORDER] * 2
    queries = [(sq, ni.ns_value(v)) for v in range(0, 14) for sq in (1, 0)]
    plan, want = _check(batch, [Index(ctx, c) for c in cells], queries)
    e = plan.entries()
    assert plan.count.value > 0
    assert (e["starts"] >= 0).all() and (e["starts"] < w).all() and (e["ends"] > e["starts"]).all() and (e["ends"] <= w).all()
    assert (e["rows"] < k).all() and (e["query_idx"] < len(queries)).all() and (e["kinds"] <= 1).all()
    assert (np.diff(e["leaf_off"].astype(np.int64)) == np.where(e["kinds"] == 0, e["ends"] - e["starts"], 0)).all()


# ------------------------------------------------------------------------- 6. errors
def test_plan_and_prove_call_errors(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    k = 2
    squares = _three_squares(oracle, k)
    batch = BatchIndex(ctx, [s[0] for s in squares])
    lib, h = ctx.lib, ctx.handle
    err = lambda: lib.cel_last_error(h).decode()
    d_work = DeviceBuffer(lib.cel_dev_namespace_squares_workspace_size(k, 2), fill=0xEE)
    ns = np.frombuffer(squares[0][1][0] + squares[1][2][0], np.uint8).copy()
    cnt = ctypes.c_uint64()
    arrs = [np.full(9, SENTINEL, np.uint32), np.full(9, SENTINEL, np.uint32), np.full(9, SENTINEL, np.int32),
            np.full(9, SENTINEL, np.int32), np.full(9, SENTINEL, np.uint8), np.full(9, SENTINEL, np.uint64),
            np.full(9, SENTINEL, np.uint64)]
    u32 = lambda *v: np.array(v, np.uint32)

    def plan(handle=h, d_index=batch.d_index.ptr, k=k, n_squares=3, n=2, sq=u32(0, 1), ns=ns, cap=8, arrays=arrs, count=cnt,
             work=d_work.ptr):
        ptrs = [None if a is None else P(a) for a in arrays]
        return lib.cel_dev_namespace_plan_squares(handle, d_index, k, n_squares, n, None if sq is None else P(sq),
                                                  None if ns is None else P(ns), cap, *ptrs,
                                                  None if count is None else ctypes.byref(count), work, None)

    def untouched():
        synchronize()
        return all((a == SENTINEL).all() for a in arrs) and (d_work.download((d_work.nbytes,)) == 0xEE).all()

    assert plan(handle=None) == _lib.EINVAL
    assert plan(sq=u32(0, 3)) == _lib.EINVAL and err() == "query 1: square 3 of 3"
    assert plan(n_squares=0) == _lib.EINVAL and err() == "query 0: square 0 of 0"
    assert plan(n_squares=65536) == _lib.EINVAL and "more than one call takes" in err()
    for kw in (dict(d_index=None), dict(ns=None), dict(sq=None), dict(count=None), dict(work=None),
               dict(arrays=arrs[:3] + [None] + arrs[4:]), dict(arrays=[None] * 7)):
        assert plan(**kw) == _lib.EINVAL and err() == "nil argument", kw
    assert plan(work=ctypes.c_void_p(d_work.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert plan(d_index=ctypes.c_void_p(batch.d_index.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    for bad_k in (0, 3, 1024):
        assert plan(k=bad_k) == _lib.EINVAL and "power of two" in err()
    bad = ns.copy()
    bad[29:] = 0xFF
    assert plan(ns=bad) == _lib.EINVAL and "namespace 1 is the parity namespace" in err()
    assert untouched(), "a rejected plan wrote its outputs"
    assert plan(n=0, ns=None, sq=None) == _lib.OK and cnt.value == 0
    assert plan(n=0, n_squares=0, ns=None, sq=None, d_index=None) == _lib.OK
    assert plan(cap=0, arrays=[None] * 7) == _lib.OK and cnt.value >= 1
    assert plan() == _lib.OK and cnt.value >= 1
    m = cnt.value
    d_leaves, d_nodes = DeviceBuffer(1 << 16, fill=0xEE), DeviceBuffer(1 << 16, fill=0xEE)

    def prove(handle=h, d_eds=batch.d_eds.ptr, d_index=batch.d_index.ptr, k=k, n_squares=3, m=m, leaves=d_leaves.ptr,
              nodes=d_nodes.ptr, work=d_work.ptr):
        return lib.cel_dev_namespace_prove_squares(handle, d_eds, d_index, k, n_squares, m, leaves, nodes, work, None)

    def outputs_untouched():
        synchronize()
        return (d_leaves.download((d_leaves.nbytes,)) == 0xEE).all() and (d_nodes.download((d_nodes.nbytes,)) == 0xEE).all()

    assert prove(handle=None) == _lib.EINVAL
    for kw in (dict(d_index=None), dict(nodes=None), dict(work=None), dict(d_eds=None)):
        assert prove(**kw) == _lib.EINVAL and err() == "nil argument", kw
    assert prove(leaves=ctypes.c_void_p(d_leaves.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert prove(nodes=ctypes.c_void_p(d_nodes.ptr.value + 1)) == _lib.EINVAL and "2-byte aligned" in err()
    assert prove(d_index=ctypes.c_void_p(batch.d_index.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert prove(work=ctypes.c_void_p(d_work.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert prove(k=3) == _lib.EINVAL and prove(n_squares=65536) == _lib.EINVAL
    assert prove(m=0) == _lib.OK and prove(n_squares=0) == _lib.OK
    # a plan of one sort is nothing to the prove call of the other sort
    assert lib.cel_dev_namespace_prove(h, batch.d_eds.ptr, batch.d_index.ptr, k, m, d_leaves.ptr, d_nodes.ptr, d_work.ptr,
                                       None) == _lib.OK
    single_work = DeviceBuffer(lib.cel_dev_namespace_workspace_size(k, 2), fill=0xEE)
    one = ctypes.c_uint64()
    assert lib.cel_dev_namespace_plan(h, batch.d_index.ptr, k, 2, P(ns), 0, *([None] * 7), ctypes.byref(one),
                                      single_work.ptr, None) == _lib.OK and one.value >= 1
    assert prove(work=single_work.ptr, m=one.value) == _lib.OK
    assert outputs_untouched(), "a prove call ran a plan of the other sort"
    assert prove() == _lib.OK
    assert not outputs_untouched()


# ------------------------------------------------------------------------- 7. Python
def test_shares_by_namespace_batch(ctx, oracle):
    from celestia_eds import _lib
    from celestia_eds._lib import CelError
    from celestia_eds.rsmt2d import ExtendedDataSquare, SharesByNamespaceBatch
    ks = [2, 8, 2, 4]
    odss = [ni.run_ods(k, LAYOUTS[k], 90 + i) for i, k in enumerate(ks)]
    squares = [ExtendedDataSquare(oracle.extend_and_commit(o[0])[0], ctx=ctx) for o in odss]
    queries = [(sq, ns) for sq in (3, 0, 1, 2, 1) for ns in odss[sq][1][:3] + odss[sq][2][:2] + [ni.BELOW_ALL, ni.ABOVE_ALL]]
    got = SharesByNamespaceBatch(squares, queries, ctx=ctx)
    assert len(got) == len(queries) and any(got)
    flat = lambda rows: [(r, p.Start, p.End, p.Nodes, p.LeafHash, s) for r, p, s in rows]
    for (sq, ns), g in zip(queries, got):
        assert flat(g) == flat(squares[sq].SharesByNamespace(ns))
    assert SharesByNamespaceBatch(squares, [], ctx=ctx) == []
    with pytest.raises(CelError) as e:
        SharesByNamespaceBatch(squares, [(0, ni.PARITY)], ctx=ctx)
    assert e.value.status == _lib.EINVAL
    with pytest.raises(CelError):
        SharesByNamespaceBatch(squares, [(4, odss[0][1][0])], ctx=ctx)
