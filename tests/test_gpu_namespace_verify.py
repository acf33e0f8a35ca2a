"""GPU: nmt Proof.VerifyNamespace in batches (cel_nmt_verify_namespace_batch,
cel_dev_nmt_verify_namespace_batch, proof.VerifyNamespaceBatch). The producer's device outputs go
in unchanged; accepted proofs and every rejection, each by a named construction with its verdict
stated (namespace_inputs.proof_cases), must get that verdict and the host mirror's; malformed
proofs are verdict 0 and leave their neighbours alone."""
import ctypes

import numpy as np
import pytest

import namespace_inputs as ni
import verify_cases as vc
from test_gpu_namespace import LAYOUTS, Plan, _queries, _square
from test_gpu_prove import Index

pytestmark = pytest.mark.gpu

P = vc._p


def _flatten(cases):
    buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return dict(
        n=len(cases),
        starts=np.array([c.start for c in cases], np.int32), ends=np.array([c.end for c in cases], np.int32),
        kinds=np.array([c.kind for c in cases], np.uint8),
        ns=buf(c.ns for c in cases), leaves=buf(x for c in cases for x in c.leaves),
        leaf_off=np.cumsum([0] + [len(c.leaves) for c in cases]).astype(np.uint64),
        nodes=buf(x for c in cases for x in c.nodes),
        node_off=np.cumsum([0] + [len(c.nodes) for c in cases]).astype(np.uint64),
        roots=buf(c.root for c in cases), root_idx=np.arange(len(cases), dtype=np.uint32))


def _dev_call(ctx, f, d_leaves, d_nodes, d_roots, nroots, d_ok, d_work):
    return ctx.lib.cel_dev_nmt_verify_namespace_batch(
        ctx.handle, f["n"], P(f["starts"]), P(f["ends"]), P(f["kinds"]), P(f["ns"]), d_leaves, P(f["leaf_off"]), d_nodes,
        P(f["node_off"]), d_roots, nroots, P(f["root_idx"]), d_ok, d_work, None)


def dev_batch(ctx, cases, node_shift=2):
    """The device form over device buffers; the packed nodes start node_shift bytes into their
    buffer and the roots 90 bytes into theirs, so neither is dword aligned throughout."""
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    f = _flatten(cases)
    d_leaves = DeviceBuffer(f["leaves"].nbytes)
    d_leaves.upload(f["leaves"])
    d_nodes = DeviceBuffer(f["nodes"].nbytes + node_shift)
    d_nodes.upload_at(node_shift, f["nodes"])
    d_roots = DeviceBuffer(f["roots"].nbytes + 90)
    d_roots.upload_at(90, f["roots"])
    d_ok = DeviceBuffer(f["n"] + 16, fill=0xEE)
    tl, tn = int(f["leaf_off"][-1]), int(f["node_off"][-1])
    size = ctx.lib.cel_dev_nmt_verify_namespace_workspace_size(tl, tn, f["n"])
    d_work = DeviceBuffer(size + 64, fill=0xEE)
    st = _dev_call(ctx, f, d_leaves.ptr, ctypes.c_void_p(d_nodes.ptr.value + node_shift),
                   ctypes.c_void_p(d_roots.ptr.value + 90), f["n"], d_ok.ptr, d_work.ptr)
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    synchronize()
    assert (d_work.download_at(size, (64,)) == 0xEE).all(), "workspace overrun"
    ok = d_ok.download((f["n"] + 16,))
    assert (ok[f["n"]:] == 0xEE).all() and set(ok[:f["n"]].tolist()) <= {0, 1}
    return [bool(v) for v in ok[:f["n"]]]


def host_batch(ctx, cases):
    from celestia_eds import _lib
    f = _flatten(cases)
    ok = np.full(f["n"], 0xEE, np.uint8)
    st = ctx.lib.cel_nmt_verify_namespace_batch(ctx.handle, f["n"], P(f["starts"]), P(f["ends"]), P(f["kinds"]), P(f["ns"]),
                                                P(f["leaves"]), P(f["leaf_off"]), P(f["nodes"]), P(f["node_off"]),
                                                P(f["roots"]), f["n"], P(f["root_idx"]), P(ok))
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    assert set(ok.tolist()) <= {0, 1}
    return [bool(v) for v in ok]


# ------------------------------------------------------------- 1. producer into verifier
@pytest.mark.parametrize("k", [1, 4, 8, 32])
def test_producer_feeds_namespace_verifier(ctx, oracle, k):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    runs = LAYOUTS.get(k) or ni.seeded_runs(k, 32, 3 * k)
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k, runs=runs, seed=None if k in LAYOUTS else 3200)
    idx = Index(ctx, eds)
    queries = _queries(present, absent)
    plan = Plan(idx, queries)
    assert plan.status == _lib.OK
    e = plan.entries()
    n = plan.count.value
    plan.prove()
    if k > 1:
        assert 0 in e["kinds"] and 1 in e["kinds"]
    ns = np.stack([np.frombuffer(queries[i], np.uint8) for i in e["ns_idx"]])
    tl, tn = int(e["leaf_off"][-1]), int(e["node_off"][-1])
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_namespace_workspace_size(tl, tn, n))
    f = dict(n=n, starts=e["starts"], ends=e["ends"], kinds=e["kinds"], ns=ns, leaf_off=e["leaf_off"],
             node_off=e["node_off"], root_idx=e["rows"])

    def verify():
        st = _dev_call(ctx, f, plan.d_leaves.ptr, plan.d_nodes_ptr, idx.d_roots.ptr, 2 * idx.w, d_ok.ptr, d_work.ptr)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        return d_ok.download((n,))

    assert (verify() == 1).all(), "a produced proof does not verify"
    if tl:
        # one byte of one share flipped on the device: that proof alone fails
        victim = next(i for i in range(n) if e["kinds"][i] == 0 and i >= n // 3)
        at = int(e["leaf_off"][victim]) * 512 + 300
        byte = plan.d_leaves.download_at(at, (1,))
        plan.d_leaves.upload_at(at, byte ^ 0x20)
        want = np.ones(n, np.uint8)
        want[victim] = 0
        assert np.array_equal(verify(), want)


# ------------------------------------------------------------------- 2. the named cases
def test_mixed_batch_of_named_cases(ctx):
    cases = ni.proof_cases()
    names = [c.name for c in cases]
    for need in ("one leaf short at the right end", "one leaf short at the left end", "a share with another prefix",
                 "absence with leaf hash min == nid", "absence with leaf hash min < nid", "absence with a leaf", "kind 2",
                 "a node bit flipped", "the root bit flipped", "empty proof inside the root's range"):
        assert need in names
    rng = np.random.default_rng(2)
    order = [cases[i] for i in rng.permutation(len(cases))] + cases  # each twice, at two places
    got = dev_batch(ctx, order)
    for c, v in zip(order, got):
        assert v is c.want, c.name
        assert c.mirror() is c.want, c.name
    assert host_batch(ctx, order) == got
    assert dev_batch(ctx, order, node_shift=1) == got


def test_wider_rows_against_the_mirror(ctx):
    """Every namespace value on rows of 2 .. 64 leaves: the producer mirror's proofs, each also
    with a range one leaf off and with its namespace one off; verdict = the mirror's."""
    from celestia_eds import proof
    cases = []
    for w in (2, 4, 8, 16, 32, 64):
        rng = np.random.default_rng(w)
        vals = [1 + int(v) for v in rng.integers(0, 3, w // 2).cumsum()]
        nss, shares, tree = ni.row_tree(vals, 900 + w)
        table, root = ni.tree_table(tree.leaves), tree.root()
        for v in range(0, max(vals) + 2):
            nid = ni.small_ns(v)
            p = proof.nmt_prove_namespace(table, w, nid)
            if p is None:
                cases.append(ni.NsCase(f"w{w} v{v} empty", 0, 0, 0, nid, [], [], root, True))
                continue
            absent = p.IsOfAbsence()
            nodes = p.Nodes + ([p.LeafHash] if absent else [])
            leaves = [] if absent else shares[p.Start:p.End]
            cases.append(ni.NsCase(f"w{w} v{v}", p.Start, p.End, int(absent), nid, leaves, nodes, root, True))
            cases.append(ni.NsCase(f"w{w} v{v} as {v + 1}", p.Start, p.End, int(absent), ni.small_ns(v + 1), leaves, nodes,
                                   root, None))
            if not absent and p.End - p.Start > 1:
                cases.append(ni.NsCase(f"w{w} v{v} short", p.Start, p.End - 1, 0, nid, leaves[:-1],
                                       tree.prove_range(p.Start, p.End - 1), root, False))
    got = dev_batch(ctx, cases)
    for c, v in zip(cases, got):
        assert v is c.mirror(), c.name
        if c.want is not None:
            assert v is c.want, c.name
    assert sum(got) >= 40 and got.count(False) >= 40


# --------------------------------------------------------------- 3. malformed structure
def test_malformed_proofs_are_verdict_zero(ctx):
    good = [c for c in ni.proof_cases() if c.want]
    bad = ni.malformed_cases()
    assert [c.name for c in bad][:4] == ["start < 0", "end < start", "a leaf too many", "a leaf too few"]
    batch = []
    for b in bad:  # every malformed proof between two good ones
        batch += [good[len(batch) % len(good)], b]
    batch.append(good[0])
    got = dev_batch(ctx, batch)
    assert got == [c.want for c in batch]
    assert all(c.mirror() is c.want for c in batch)
    assert host_batch(ctx, batch) == got


def test_call_errors(ctx):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer
    cases = [c for c in ni.proof_cases() if c.want][:3]
    f = _flatten(cases)
    ok = np.zeros(3, np.uint8)
    lib, h = ctx.lib, ctx.handle

    def host(**kw):
        g = dict(f, **kw)
        return lib.cel_nmt_verify_namespace_batch(h, g["n"], P(g["starts"]), P(g["ends"]),
                                                  None if g["kinds"] is None else P(g["kinds"]), P(g["ns"]), P(g["leaves"]),
                                                  P(g["leaf_off"]), P(g["nodes"]), P(g["node_off"]), P(g["roots"]),
                                                  g.get("nroots", g["n"]), P(g["root_idx"]), P(ok))

    assert host() == _lib.OK and ok.tolist() == [1, 1, 1]
    down = f["leaf_off"].copy()
    down[2] = down[1] - 1
    assert host(leaf_off=down) == _lib.EINVAL and "leaf offsets" in lib.cel_last_error(h).decode()
    down = f["node_off"].copy()
    down[1] = down[2] + 1
    assert host(node_off=down) == _lib.EINVAL and "node offsets" in lib.cel_last_error(h).decode()
    assert host(root_idx=np.array([0, 3, 2], np.uint32)) == _lib.EINVAL and "root index 3" in lib.cel_last_error(h).decode()
    assert host(nroots=2) == _lib.EINVAL
    assert host(kinds=None) == _lib.EINVAL and lib.cel_last_error(h).decode() == "nil argument"
    assert host(n=0) == _lib.OK
    d = DeviceBuffer(1 << 16)
    bad_off = f["leaf_off"].copy()
    bad_off[2] = bad_off[1] - 1
    g = dict(f, leaf_off=bad_off)
    assert _dev_call(ctx, g, d.ptr, d.ptr, d.ptr, 3, d.ptr, d.ptr) == _lib.EINVAL
    g = dict(f, root_idx=np.array([0, 1, 3], np.uint32))
    assert _dev_call(ctx, g, d.ptr, d.ptr, d.ptr, 3, d.ptr, d.ptr) == _lib.EINVAL
    assert _dev_call(ctx, f, ctypes.c_void_p(d.ptr.value + 8), d.ptr, d.ptr, 3, d.ptr, d.ptr) == _lib.EINVAL
    assert _dev_call(ctx, f, None, d.ptr, d.ptr, 3, d.ptr, d.ptr) == _lib.EINVAL


# ------------------------------------------------------------------- 4. Python, end to end
def test_python_end_to_end_k4(ctx, oracle):
    from celestia_eds import CelError, _lib, proof
    from celestia_eds.rsmt2d import ExtendedDataSquare
    k = 4
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, k)
    sq = ExtendedDataSquare(eds, ctx=ctx)
    roots = sq.RowRoots()
    assert roots == [r.tobytes() for r in rr]
    flat = ods.reshape(-1, 512)
    queries = _queries(present, absent)
    per_ns = proof.TreeIndex(eds, ctx=ctx).namespace_rows(queries)
    assert len(per_ns) == len(queries)
    proofs, nss, leaves, rts = [], [], [], []
    for ns, rows in zip(queries, per_ns):
        assert rows == sq.SharesByNamespace(ns)  # the host entry gives the same
        for row, p, shares in rows:
            want = proof.nmt_prove_namespace(trees[row], 2 * k, ns)
            assert p == want
            assert p.VerifyNamespace(ns, shares, roots[row])
            proofs.append(p)
            nss.append(ns)
            leaves.append(shares)
            rts.append(roots[row])
        if ns in present:
            got = [s for _, _, sh in rows for s in sh]
            assert got == [x.tobytes() for x in flat[(flat[:, :29] == np.frombuffer(ns, np.uint8)).all(axis=1)]]
        elif ns in absent:
            assert all(p.IsOfAbsence() and not sh for _, p, sh in rows)
    assert any(p.IsOfAbsence() for p in proofs) and any(not p.IsOfAbsence() for p in proofs)
    n = len(proofs)
    # tampered copies ride along: a short range, a foreign namespace, a node of the wrong size
    inc = next(i for i, p in enumerate(proofs) if not p.IsOfAbsence() and p.End - p.Start >= 2)
    short = proof.NMTProof(Start=proofs[inc].Start, End=proofs[inc].End - 1,
                           Nodes=proof.nmt_prove_range(trees[[r for r in range(2 * k) if roots[r] == rts[inc]][0]],
                                                       proofs[inc].Start, proofs[inc].End - 1))
    proofs += [short, proofs[0], proof.NMTProof(Start=0, End=1, Nodes=[b"x" * 89])]
    nss += [nss[inc], absent[-1], nss[0]]
    leaves += [leaves[inc][:-1], leaves[0], leaves[0][:1]]
    rts += [rts[inc], rts[0], rts[0]]
    got = proof.VerifyNamespaceBatch(proofs, nss, leaves, rts, ctx=ctx)
    assert got == [True] * n + [False, False, False]
    assert got == [p.VerifyNamespace(a, b, c) for p, a, b, c in zip(proofs, nss, leaves, rts)]
    assert short.VerifyInclusion(nss[inc], leaves[inc][:-1], rts[inc])
    assert proof.VerifyNamespaceBatch([], [], [], [], ctx=ctx) == []
    with pytest.raises(CelError) as ei:
        sq.SharesByNamespace(ni.PARITY)
    assert ei.value.status == _lib.EINVAL
    assert sq.SharesByNamespace(ni.BELOW_ALL) == []
