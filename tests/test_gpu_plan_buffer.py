"""GPU: the ctx's one page-locked plan buffer under its rule (csrc/api_common.hpp: plan_stage,
plan_uploaded) across the entry points that share it. On one fresh ctx, with no host
synchronisation in between, two rounds of cel_dev_tree_index_build, cel_dev_prove_batch,
cel_dev_nmt_verify_batch (on the prover's device output), cel_dev_nmt_verify_namespace_batch and
cel_dev_create_commitments are enqueued: each call refills the buffer the call before it uploaded
from, and round two's tables are larger than round one's, so the buffer has to grow while an
upload out of the old one may still be queued. After one synchronisation every verdict must be the
host mirror's (celestia_eds/proof.py, tests/nmt_ref.py) and every commitment
cel_create_commitments' on the same blobs."""
import ctypes

import numpy as np
import pytest

import commitment_ref as cref
import namespace_inputs as ni
import nmt_ref
import verify_cases as vc
from test_gpu_namespace import _queries, _square

pytestmark = pytest.mark.gpu

P = vc._p
K = 4
W = 2 * K
ROW, COL = 0, 1


def _buf(parts):
    return np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()


def _range_requests(n):
    """n requests (axis, tree, start, end): three ranges of several leaves, then single leaves of
    both axes. (Round.__init__ verifies every third under a range one leaf to the right and every
    seventh under another namespace.)"""
    reqs = [(ROW, 2, 0, K), (COL, W - 1, 1, 3), (ROW, W - 1, 2, W)]  # each inside one namespace
    cells = [(axis, t, p, p + 1) for axis in (ROW, COL) for t in range(W) for p in range(W)]
    return (reqs + cells * (n // len(cells) + 1))[:n]


def _namespace_cases(trees, eds, rr, queries, n):
    """n proofs as the namespace verifier takes them: the mirror's proofs of every (query, row)
    of the square, and each of them once more under the next query's namespace."""
    from celestia_eds import proof
    base = []
    for q, ns in enumerate(queries):
        for row in range(W):
            p = proof.nmt_prove_namespace(trees[row], W, ns)
            if p is None:
                continue
            absent = p.IsOfAbsence()
            nodes = list(p.Nodes) + ([p.LeafHash] if absent else [])
            leaves = [] if absent else [eds[row, c].tobytes() for c in range(p.Start, p.End)]
            root = rr[row].tobytes()
            base.append(ni.NsCase(f"q{q} row{row}", p.Start, p.End, int(absent), ns, leaves, nodes, root, True))
            base.append(ni.NsCase(f"q{q} row{row} as the next", p.Start, p.End, int(absent),
                                  queries[(q + 1) % len(queries)], leaves, nodes, root, None))
    assert len(base) >= 3
    return (base * (n // len(base) + 1))[:n]


class Round:
    """The inputs of one round on the device, its outputs prefilled, and what the host expects."""

    def __init__(self, c, sq, n_proofs, n_ns, blobs):
        from celestia_eds import inclusion, proof
        from hipmem import DeviceBuffer
        ods, eds, rr, present, absent, trees, col_trees = sq
        lib = c.lib
        self.c = c
        # the prover's requests and the verifier's view of them
        reqs = _range_requests(n_proofs)
        self.n = n = len(reqs)
        self.axes = np.array([r[0] for r in reqs], np.uint8)
        self.index = np.array([r[1] for r in reqs], np.uint32)
        self.starts = np.array([r[2] for r in reqs], np.int32)
        self.ends = np.array([r[3] for r in reqs], np.int32)
        self.leaf_off, self.node_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        assert lib.cel_prove_offsets(K, n, P(self.starts), P(self.ends), P(self.leaf_off), P(self.node_off)) == 0
        tl, tn = int(self.leaf_off[-1]), int(self.node_off[-1])
        self.v_starts, self.v_ends = self.starts.copy(), self.ends.copy()
        nss, self.want = [], []
        for i, (axis, t, s, e) in enumerate(reqs):
            cell = eds[t, s] if axis == ROW else eds[s, t]
            ns = cell[:29].tobytes() if t < K and s < K else ni.PARITY
            if i % 3 == 2:
                self.v_starts[i] += 1
                self.v_ends[i] += 1
            if i % 7 == 6:
                ns = ni.ABOVE_ALL
            nss.append(ns)
            tree = trees[t] if axis == ROW else col_trees[t]
            leaves = [(eds[t, p] if axis == ROW else eds[p, t]).tobytes() for p in range(s, e)]
            self.want.append(nmt_ref.mirror_verify(int(self.v_starts[i]), int(self.v_ends[i]), ns, leaves,
                                                   proof.nmt_prove_range(tree, s, e), tree[-1].tobytes()))
        self.ns = _buf(nss)
        self.root_idx = np.where(self.axes == COL, W + self.index, self.index).astype(np.uint32)
        self.d_leaves = DeviceBuffer(tl * 512)
        self.d_nodes = DeviceBuffer(tn * 90 + 2)
        self.d_req = DeviceBuffer(lib.cel_dev_prove_workspace_size(n))
        self.d_ok = DeviceBuffer(n, fill=0xEE)
        self.d_vwork = DeviceBuffer(lib.cel_dev_nmt_verify_workspace_size(tl, tn, n))
        # the namespace verifier's batch, from the host
        self.cases = cases = _namespace_cases(trees, eds, rr, _queries(present, absent), n_ns)
        self.m = m = len(cases)
        self.q_starts = np.array([x.start for x in cases], np.int32)
        self.q_ends = np.array([x.end for x in cases], np.int32)
        self.q_kinds = np.array([x.kind for x in cases], np.uint8)
        self.q_ns = _buf(x.ns for x in cases)
        self.q_leaf_off = np.cumsum([0] + [len(x.leaves) for x in cases]).astype(np.uint64)
        self.q_node_off = np.cumsum([0] + [len(x.nodes) for x in cases]).astype(np.uint64)
        self.q_root_idx = np.arange(m, dtype=np.uint32)
        q_leaves, q_nodes = _buf(y for x in cases for y in x.leaves), _buf(y for x in cases for y in x.nodes)
        q_roots = _buf(x.root for x in cases)
        self.dq_leaves, self.dq_nodes, self.dq_roots = (DeviceBuffer(a.nbytes) for a in (q_leaves, q_nodes, q_roots))
        self.dq_leaves.upload(q_leaves)
        self.dq_nodes.upload(q_nodes)
        self.dq_roots.upload(q_roots)
        self.dq_ok = DeviceBuffer(m, fill=0xEE)
        self.dq_work = DeviceBuffer(lib.cel_dev_nmt_verify_namespace_workspace_size(
            int(self.q_leaf_off[-1]), int(self.q_node_off[-1]), m))
        self.q_want = [x.mirror() for x in cases]
        # the blobs
        self.blobs = blobs
        data, self.b_off, self.b_ns, _ = inclusion._pack_blobs(blobs)
        self.d_data = DeviceBuffer(len(data))
        self.d_data.upload(data)
        self.d_com = DeviceBuffer(32 * len(blobs), fill=0xEE)
        shares = sum(cref.sparse_shares_needed(len(d)) for _, d in blobs)
        self.d_cwork = DeviceBuffer(lib.cel_dev_commitments_workspace_size(shares, len(blobs)))

    def enqueue(self, d_eds, d_index, d_roots):
        """The five calls on the ctx's stream; nothing here waits for the device."""
        c, lib, h = self.c, self.c.lib, self.c.handle
        d_cr = ctypes.c_void_p(d_roots.ptr.value + W * 90)
        c.check(lib.cel_dev_tree_index_build(h, d_eds.ptr, K, d_index.ptr, d_roots.ptr, d_cr, None, None, 0, None))
        d_nodes = ctypes.c_void_p(self.d_nodes.ptr.value + 2)  # 2-byte aligned and no more
        c.check(lib.cel_dev_prove_batch(h, d_eds.ptr, d_index.ptr, K, self.n, P(self.axes), P(self.index),
                                        P(self.starts), P(self.ends), self.d_leaves.ptr, d_nodes, self.d_req.ptr, None))
        c.check(lib.cel_dev_nmt_verify_batch(h, self.n, P(self.v_starts), P(self.v_ends), P(self.ns), self.d_leaves.ptr,
                                             P(self.leaf_off), d_nodes, P(self.node_off), d_roots.ptr, 2 * W,
                                             P(self.root_idx), self.d_ok.ptr, self.d_vwork.ptr, None))
        c.check(lib.cel_dev_nmt_verify_namespace_batch(h, self.m, P(self.q_starts), P(self.q_ends), P(self.q_kinds),
                                                       P(self.q_ns), self.dq_leaves.ptr, P(self.q_leaf_off),
                                                       self.dq_nodes.ptr, P(self.q_node_off), self.dq_roots.ptr, self.m,
                                                       P(self.q_root_idx), self.dq_ok.ptr, self.dq_work.ptr, None))
        c.check(lib.cel_dev_create_commitments(h, self.d_data.ptr, P(self.b_off), len(self.blobs), P(self.b_ns), None, 64,
                                               self.d_com.ptr, self.d_cwork.ptr, None))

    def check(self, name):
        from celestia_eds import inclusion
        ok = self.d_ok.download((self.n,)).tolist()
        assert ok == [int(v) for v in self.want], f"{name}: inclusion verdicts"
        q_ok = self.dq_ok.download((self.m,)).tolist()
        assert q_ok == [int(v) for v in self.q_want], f"{name}: namespace verdicts"
        for x, v in zip(self.cases, self.q_want):
            assert x.want is None or v is x.want, x.name
        com = self.d_com.download((len(self.blobs), 32))
        assert [r.tobytes() for r in com] == inclusion.CreateCommitments(self.blobs, ctx=self.c), f"{name}: commitments"
        # both verdicts occur, so a table read from the wrong place cannot pass by being constant
        assert 0 in ok and 1 in ok and 0 in q_ok and 1 in q_ok


def test_entry_points_share_the_plan_buffer(ctx, oracle):
    import celestia_eds
    from celestia_eds import proof
    from celestia_eds.rsmt2d import ExtendedDataSquare
    from hipmem import DeviceBuffer, synchronize
    ods, eds, rr, present, absent, trees = _square(oracle, ctx, K)
    col_trees = proof.axis_trees(ExtendedDataSquare(eds, ctx=ctx), COL, 0, W)
    sq = (ods, eds, rr, present, absent, trees, col_trees)
    rng = np.random.default_rng(44)
    blobs = [(cref.random_namespace(rng), cref.random_bytes(rng, int(rng.integers(1, 3000)))) for _ in range(42)]
    c = celestia_eds.Context(ctx.device)  # fresh: its plan buffer starts empty
    try:
        small = Round(c, sq, 3, 3, blobs[:2])
        large = Round(c, sq, 300, 300, blobs[2:])
        d_eds = DeviceBuffer(eds.nbytes)
        d_eds.upload(eds)
        d_index = DeviceBuffer(c.lib.cel_dev_tree_index_size(K))
        d_roots = DeviceBuffer(2 * W * 90)
        synchronize()
        small.enqueue(d_eds, d_index, d_roots)
        large.enqueue(d_eds, d_index, d_roots)
        synchronize()
        small.check("round one")
        large.check("round two")
    finally:
        c.close()
