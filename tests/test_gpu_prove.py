"""GPU: NMT proofs built in batches from the tree index of a resident square
(cel_dev_tree_index_build, cel_dev_prove_batch, cel_prove_samples, proof.TreeIndex,
proof.NewShareInclusionProofsBatch, ExtendedDataSquare.SampleProofs). The index's roots and DAH
are checked against the oracle; every proof byte against the path that was there before
(proof.axis_trees: every node downloaded, then proof.nmt_prove_range per proof); the producer's
device outputs go unchanged into the device verifier; samples go into the repair."""
import ctypes

import numpy as np
import pytest

import verify_cases as vc
from eds_inputs import random_ods

pytestmark = pytest.mark.gpu

PARITY = b"\xff" * 29
ROW, COL = 0, 1
P = vc._p
_parent_cache = {}


def _square(oracle, k, seed=None):
    return oracle.extend_and_commit(random_ods(k, 100 + k if seed is None else seed))


def _parent(ctx, key, cells):
    """The path before the index: every node of all 4k trees on the host, [axis][tree][4k-1][90]."""
    from celestia_eds import proof
    from celestia_eds.rsmt2d import ExtendedDataSquare
    if key not in _parent_cache:
        sq = ExtendedDataSquare(cells, ctx=ctx)
        _parent_cache[key] = [proof.axis_trees(sq, axis, 0, cells.shape[0]) for axis in (ROW, COL)]
    return _parent_cache[key]


class Index:
    """The tree index of `cells` in device buffers; the two root arrays share one buffer, rows
    first, so it is also the verifier's root table."""

    def __init__(self, ctx, cells, flags=0, want_dah=True):
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        self.ctx, self.cells = ctx, cells
        self.w = cells.shape[0]
        self.k = self.w // 2
        w = self.w
        self.d_eds = DeviceBuffer(cells.nbytes)
        self.d_eds.upload(cells)
        size = ctx.lib.cel_dev_tree_index_size(self.k)
        self.d_index = DeviceBuffer(size + 64, fill=0xEE)
        self.d_roots = DeviceBuffer(2 * w * 90)
        self.d_rr = self.d_roots.ptr
        self.d_cr = ctypes.c_void_p(self.d_roots.ptr.value + w * 90)
        self.d_dah = DeviceBuffer(32, fill=0xEE)
        status = ctypes.c_int32(0x7F7F7F7F)
        st = ctx.lib.cel_dev_tree_index_build(ctx.handle, self.d_eds.ptr, self.k, self.d_index.ptr, self.d_rr, self.d_cr,
                                              self.d_dah.ptr if want_dah else None, ctypes.byref(status), flags, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        self.status = status.value
        roots = self.d_roots.download((2, w, 90))
        self.rr, self.cr = roots[0], roots[1]
        self.dah = self.d_dah.download((32,)).tobytes()
        # nothing behind the index's size is written
        assert (self.d_index.download_at(size, (64,)) == 0xEE).all()

    def prove(self, axes, index, starts, ends, leaves=True, node_shift=2):
        """cel_dev_prove_batch; d_nodes starts node_shift bytes into its buffer, so it is not
        dword aligned. Returns (leaves, nodes, leaf_off, node_off) and keeps the device buffers."""
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        ctx = self.ctx
        axes, index = np.ascontiguousarray(axes, np.uint8), np.ascontiguousarray(index, np.uint32)
        starts, ends = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(ends, np.int32)
        n = len(axes)
        leaf_off, node_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        assert ctx.lib.cel_prove_offsets(self.k, n, P(starts), P(ends), P(leaf_off), P(node_off)) == _lib.OK
        tl, tn = int(leaf_off[-1]), int(node_off[-1])
        self.d_leaves = DeviceBuffer(tl * 512 + 16, fill=0xEE)
        self.d_nodes = DeviceBuffer(node_shift + tn * 90 + 16, fill=0xEE)
        self.d_nodes_ptr = ctypes.c_void_p(self.d_nodes.ptr.value + node_shift)
        d_work = DeviceBuffer(ctx.lib.cel_dev_prove_workspace_size(n))
        st = ctx.lib.cel_dev_prove_batch(ctx.handle, self.d_eds.ptr if leaves else None, self.d_index.ptr, self.k, n,
                                         P(axes), P(index), P(starts), P(ends), self.d_leaves.ptr if leaves else None,
                                         self.d_nodes_ptr, d_work.ptr, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        raw = self.d_nodes.download((self.d_nodes.nbytes,))
        assert (raw[:node_shift] == 0xEE).all() and (raw[node_shift + tn * 90:] == 0xEE).all(), "nodes outside their range"
        got_leaves = self.d_leaves.download((self.d_leaves.nbytes,))
        if leaves:
            assert (got_leaves[tl * 512:] == 0xEE).all(), "shares outside their range"
        else:
            assert (got_leaves == 0xEE).all()
        return got_leaves[:tl * 512].reshape(tl, 512), raw[node_shift:node_shift + tn * 90].reshape(tn, 90), leaf_off, node_off


def _all_samples(w):
    """Every single-leaf request on both axes: (axis, tree, start, end), 2 w^2 of them."""
    return [(axis, t, p, p + 1) for axis in (ROW, COL) for t in range(w) for p in range(w)]


def _seeded_ranges(w, seed, count=300):
    k = w // 2
    rng = np.random.default_rng(seed)
    out = [(ROW, 0, 0, w), (COL, w - 1, 0, w),                  # no nodes, twice in a row
           (ROW, 1, 0, 1), (COL, 1, 0, 1), (ROW, w - 1, w - 1, w), (COL, 0, w - 1, w),
           (ROW, k - 1, k - 1, k + 1), (COL, k, k - 1, k + 1), (ROW, 0, 1, w - 1) if w > 2 else (ROW, 0, 0, 2),
           (COL, 0, 0, k), (COL, w - 1, k, w), (COL, k - 1, 0, w - 1)]  # multi-leaf column ranges
    while len(out) < count:
        s = int(rng.integers(0, w))
        e = int(rng.integers(s + 1, w + 1))
        if len(out) % 3 == 0:  # straddle k
            s, e = int(rng.integers(0, k)), int(rng.integers(k + 1, w + 1))
        out.append((int(rng.integers(0, 2)), int(rng.integers(0, w)), s, e))
    assert sum(1 for a, _, s, e in out if a == COL and e - s > 1) >= count // 15
    assert sum(1 for _, _, s, e in out if s < k < e) >= count // 15
    return out


def _expected(trees, cells, reqs):
    from celestia_eds import proof
    nodes, leaves = [], []
    for axis, t, s, e in reqs:
        nodes += proof.nmt_prove_range(trees[axis][t], s, e)
        leaves += [cells[t, p] if axis == ROW else cells[p, t] for p in range(s, e)]
    nodes = np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 90)
    return np.stack(leaves), nodes


def _check_parity(idx, trees, reqs):
    """The batch over reqs equals the parent path byte for byte."""
    axes, index, starts, ends = zip(*reqs)
    leaves, nodes, leaf_off, node_off = idx.prove(axes, index, starts, ends)
    want_leaves, want_nodes = _expected(trees, idx.cells, reqs)
    assert leaf_off[-1] == len(want_leaves) and node_off[-1] == len(want_nodes)
    assert np.array_equal(nodes, want_nodes), "proof nodes differ"
    assert np.array_equal(leaves, want_leaves), "shares differ"
    return leaves, nodes, leaf_off, node_off


# ------------------------------------------------------------------ 1. index roots
@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_index_roots_and_status(ctx, oracle, k):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    eds, rr, cr, dah = _square(oracle, k)
    for flags in (0, _lib.FLAG_ORDER_CHECK):
        idx = Index(ctx, eds, flags=flags)
        assert np.array_equal(idx.rr, rr) and np.array_equal(idx.cr, cr), "roots differ"
        assert idx.dah == dah and idx.status == _lib.OK
    idx = Index(ctx, eds, want_dah=False)  # no DAH wanted: roots and status all the same
    assert np.array_equal(idx.rr, rr) and np.array_equal(idx.cr, cr) and idx.status == _lib.OK
    if k == 1:
        return
    # two Q0 shares swapped: the status of cel_dev_commit_only on the same cells
    bad = eds.copy()
    bad[0, 0], bad[0, 1] = eds[0, 1], eds[0, 0]
    assert bad[0, 0, :29].tobytes() > bad[0, 1, :29].tobytes()
    w = 2 * k
    d_eds = DeviceBuffer(bad.nbytes)
    d_eds.upload(bad)
    d_rr, d_cr, d_dah, d_st = DeviceBuffer(w * 90), DeviceBuffer(w * 90), DeviceBuffer(32), DeviceBuffer(4, fill=0x7F)
    d_work = DeviceBuffer(ctx.lib.cel_dev_workspace_size(k, 1))
    for flags in (0, _lib.FLAG_ORDER_CHECK):
        ctx.check(ctx.lib.cel_dev_commit_only(ctx.handle, d_eds.ptr, 1, k, d_rr.ptr, d_cr.ptr, d_dah.ptr, d_st.ptr,
                                              d_work.ptr, None, flags))
        synchronize()
        want = int(d_st.download((1,), np.int32)[0])
        assert want == (_lib.EORDER if flags else _lib.OK)
        idx = Index(ctx, bad, flags=flags)
        assert idx.status == want
        assert np.array_equal(idx.rr, d_rr.download((w, 90))) and np.array_equal(idx.cr, d_cr.download((w, 90)))
        assert idx.dah == d_dah.download((32,)).tobytes()


# ------------------------------------------------- 2. byte parity with the parent path
@pytest.mark.parametrize("k", [2, 8, 32])
def test_proofs_equal_parent_path(ctx, oracle, k):
    eds, rr, cr, _ = _square(oracle, k)
    w = 2 * k
    trees = _parent(ctx, ("eds", k), eds)
    idx = Index(ctx, eds)
    ranges = _seeded_ranges(w, k)
    reqs = _all_samples(w) + ranges
    assert len(reqs) == 2 * 4 * k * k + 300
    _, _, _, node_off = _check_parity(idx, trees, reqs)
    lg = w.bit_length() - 1
    assert np.diff(node_off)[:2 * w * w].tolist() == [lg] * (2 * w * w)          # a sample: log2(2k) nodes
    assert np.diff(node_off)[2 * w * w:2 * w * w + 2].tolist() == [0, 0]          # [0, 2k): none
    # one proof, and 257: a workgroup holds four proofs, so the last one is partial
    _check_parity(idx, trees, [ranges[7]])
    _check_parity(idx, trees, [(ROW, 0, 0, w)])
    order = np.random.default_rng(k).permutation(len(reqs))[:257]
    _check_parity(idx, trees, [reqs[i] for i in order])
    # nodes alone: no shares written, the square not read
    axes, index, starts, ends = zip(*ranges)
    _, nodes, _, _ = idx.prove(axes, index, starts, ends, leaves=False, node_shift=6)
    assert np.array_equal(nodes, _expected(trees, eds, ranges)[1])


# ------------------------------------------ 3. producer into verifier, device resident
@pytest.mark.parametrize("k", [8, 32])
def test_prover_feeds_device_verifier(ctx, oracle, k):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    eds, rr, cr, _ = _square(oracle, k)
    w = 2 * k
    idx = Index(ctx, eds)
    rng = np.random.default_rng(30 + k)
    reqs = _all_samples(w)
    for _ in range(200):  # multi-leaf ranges inside the parity half of a tree: one namespace
        axis, t = int(rng.integers(0, 2)), int(rng.integers(0, w))
        lo = 0 if t >= k else k  # trees k .. 2k-1 are parity throughout
        s = int(rng.integers(lo, w - 1))
        reqs.append((axis, t, s, int(rng.integers(s + 2, w + 1))))
    reqs = [reqs[i] for i in rng.permutation(len(reqs))]
    axes, index, starts, ends = (np.array(x) for x in zip(*reqs))
    leaves, nodes, leaf_off, node_off = idx.prove(axes, index, starts, ends)
    n = len(reqs)
    # the wrapper's namespace rule, from the host copy of the square
    ns = np.full((n, 29), 0xFF, np.uint8)
    for i, (axis, t, s, e) in enumerate(reqs):
        r, c = (t, s) if axis == ROW else (s, t)
        if e - s == 1 and r < k and c < k:
            ns[i] = eds[r, c, :29]
    root_idx = np.where(axes == ROW, index, w + index).astype(np.uint32)
    st32, en32 = starts.astype(np.int32), ends.astype(np.int32)
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(int(leaf_off[-1]), int(node_off[-1]), n))

    def verify():
        st = ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(st32), P(en32), P(ns), idx.d_leaves.ptr, P(leaf_off),
                                              idx.d_nodes_ptr, P(node_off), idx.d_roots.ptr, 2 * w, P(root_idx),
                                              d_ok.ptr, d_work.ptr, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        return d_ok.download((n,))

    assert (verify() == 1).all(), "a produced proof does not verify"
    # one byte of one share flipped on the device: that proof alone fails
    victim = next(i for i, (_, _, s, e) in enumerate(reqs) if e - s >= 3 and i > n // 2)
    at = (int(leaf_off[victim]) + 1) * 512 + 300
    byte = idx.d_leaves.download_at(at, (1,))
    idx.d_leaves.upload_at(at, byte ^ 0x20)
    want = np.ones(n, np.uint8)
    want[victim] = 0
    assert np.array_equal(verify(), want)


# --------------------------------------------------------------- 4. samples to repair
@pytest.mark.parametrize("k", [8, 32])
def test_sample_proofs_to_repair(ctx, oracle, k):
    from celestia_eds import proof
    from celestia_eds.rsmt2d import ExtendedDataSquare, RepairFromSamples
    eds, rr, cr, _ = oracle.extend_and_commit(random_ods(k, 7))
    w = 2 * k
    present = (np.random.default_rng(7).random((w, w)) < 0.55).astype(np.uint8)
    coords = [(int(r), int(c), i % 2) for i, (r, c) in enumerate(zip(*np.nonzero(present)))]
    samples = ExtendedDataSquare(eds, ctx=ctx).SampleProofs(coords)
    assert [s[:3] for s in samples] == coords
    trees = _parent(ctx, ("seed7", k), eds)
    for r, c, axis, share, nodes in samples[::7]:  # the host entry's bytes: the parent path's
        t, leaf = (r, c) if axis == ROW else (c, r)
        assert share == eds[r, c].tobytes() and nodes == proof.nmt_prove_range(trees[axis][t], leaf, leaf + 1)
    out, ok = RepairFromSamples(k, samples, [r.tobytes() for r in rr], [c.tobytes() for c in cr], ctx=ctx)
    assert all(ok) and len(ok) == int(present.sum())
    assert np.array_equal(out.cells, eds)
    assert out.RowRoots() == [r.tobytes() for r in rr] and out.ColRoots() == [c.tobytes() for c in cr]
    assert ExtendedDataSquare(eds, ctx=ctx).SampleProofs([]) == []


# ------------------------------------------------------------ 5. a non-codeword square
def test_non_codeword_square(ctx, oracle):
    """Random cells outside Q0 (no codeword), and shares inside Q0 that carry the parity
    namespace themselves: the index is the parent path's trees node for node, 6 zero bytes
    behind each, and so are the proofs."""
    k, w = 8, 16
    ods = random_ods(k, 7000 + k)
    h = k // 2
    ods[h:, :, :29] = 0xFF
    ods[:, h:, :29] = 0xFF
    cells = oracle.extend_and_commit(ods)[0].copy()
    noise = np.random.default_rng(5).integers(0, 256, cells.shape, dtype=np.uint8)
    cells[k:], cells[:, k:] = noise[k:], noise[:, k:]
    trees = _parent(ctx, ("noise", k), cells)
    idx = Index(ctx, cells)
    assert [r.tobytes() for r in idx.rr] == [t[-1].tobytes() for t in trees[ROW]]
    assert [c.tobytes() for c in idx.cr] == [t[-1].tobytes() for t in trees[COL]]
    records = w * w + 2 * w * (w - 1)
    rec = idx.d_index.download((records, 96))
    assert not rec[:, 90:].any()
    leaves = rec[:w * w, :90].reshape(w, w, 90)
    assert np.array_equal(leaves, trees[ROW][:, :w]) and np.array_equal(leaves.transpose(1, 0, 2), trees[COL][:, :w])
    at, off = w * w, w
    for l in range(1, w.bit_length()):
        m = w >> l
        level = rec[at:at + 2 * w * m, :90].reshape(2, w, m, 90)
        assert np.array_equal(level[ROW], trees[ROW][:, off:off + m]), f"row level {l}"
        assert np.array_equal(level[COL], trees[COL][:, off:off + m]), f"column level {l}"
        at, off = at + 2 * w * m, off + m
    assert at == records
    _check_parity(idx, trees, _all_samples(w) + _seeded_ranges(w, 99))


# ------------------------------------------------------------------ 6. ShareProof batch
def test_share_proofs_batch(ctx, oracle):
    from celestia_eds import da, proof
    from celestia_eds.rsmt2d import ExtendedDataSquare
    k, run = 8, 13
    ods = random_ods(k, 61)
    flat = ods.reshape(-1, 512)
    for i in range(k * k):  # runs of 13 shares of one namespace, ascending row-major: every run crosses a row end
        flat[i, :29] = np.frombuffer(bytes(19) + bytes([1 + i // run]) * 10, np.uint8)
    eds, rr, cr, dah = oracle.extend_and_commit(ods)
    sq = ExtendedDataSquare(eds, rr, cr, ctx=ctx)
    assert da.NewDataAvailabilityHeader(sq).Hash() == dah
    rng = np.random.default_rng(6)
    requests = []
    while len(requests) < 20:
        b = int(rng.integers(0, k * k // run))
        s = int(rng.integers(b * run, (b + 1) * run - 1))
        e = int(rng.integers(s + 1, (b + 1) * run + 1))
        if s // k < (e - 1) // k:
            requests.append((flat[s, :29].tobytes(), s, e))
    got = proof.NewShareInclusionProofsBatch(sq, requests)
    assert len(got) == 20
    for p, (ns, s, e) in zip(got, requests):
        assert p == proof.NewShareInclusionProofFromEDS(sq, ns, s, e)
        assert p.Data == [flat[i].tobytes() for i in range(s, e)]
        p.Validate(dah)
    assert proof.NewShareInclusionProofsBatch(sq, []) == []
    with pytest.raises(proof.CelError):
        proof.NewShareInclusionProofsBatch(sq, [(requests[0][0], 3, k * k + 1)])


def test_tree_index_python(ctx, oracle):
    """proof.TreeIndex: roots, DAH, ranges and samples through the package's own device buffers."""
    from celestia_eds import proof
    k = 8
    eds, rr, cr, dah = _square(oracle, k)
    trees = _parent(ctx, ("eds", k), eds)
    ti = proof.TreeIndex(eds, ctx=ctx)
    assert ti.row_roots == [r.tobytes() for r in rr] and ti.col_roots == [c.tobytes() for c in cr] and ti.dah == dah
    reqs = _seeded_ranges(2 * k, 8, count=40)
    axes, index, starts, ends = zip(*reqs)
    proofs, shares = ti.prove_ranges(axes, index, starts, ends, shares=True)
    for (axis, t, s, e), p, sh in zip(reqs, proofs, shares):
        assert (p.Start, p.End, p.Nodes) == (s, e, proof.nmt_prove_range(trees[axis][t], s, e))
        assert sh == [(eds[t, j] if axis == ROW else eds[j, t]).tobytes() for j in range(s, e)]
    assert ti.prove_ranges(axes, index, starts, ends) == proofs
    got = ti.prove_samples([(3, 9, ROW), (3, 9, COL), (15, 0, COL)])
    assert got[0] == (3, 9, ROW, eds[3, 9].tobytes(), proof.nmt_prove_range(trees[ROW][3], 9, 10))
    assert got[1] == (3, 9, COL, eds[3, 9].tobytes(), proof.nmt_prove_range(trees[COL][9], 3, 4))
    assert got[2] == (15, 0, COL, eds[15, 0].tobytes(), proof.nmt_prove_range(trees[COL][0], 15, 16))
    with pytest.raises(proof.CelError):
        ti.prove_samples([(16, 0, ROW)])
    with pytest.raises(proof.CelError, match="proof 1: range"):
        ti.prove_ranges([0, 0], [0, 0], [0, 5], [1, 5])


# --------------------------------------------------------------------- 7. call errors
def test_prove_call_errors(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer
    k, w = 2, 4
    eds = _square(oracle, k)[0]
    idx = Index(ctx, eds)
    lib, h = ctx.lib, ctx.handle
    d_leaves, d_nodes, d_work = DeviceBuffer(4096, fill=0xEE), DeviceBuffer(4096, fill=0xEE), DeviceBuffer(4096)
    u8 = lambda *v: np.array(v, np.uint8)
    u32 = lambda *v: np.array(v, np.uint32)
    i32 = lambda *v: np.array(v, np.int32)

    def prove(d_eds=idx.d_eds.ptr, d_index=idx.d_index.ptr, k=k, n=1, axes=u8(0), index=u32(1), starts=i32(1),
              ends=i32(3), leaves=d_leaves.ptr, nodes=d_nodes.ptr, work=d_work.ptr, handle=h):
        a = [x if x is None else P(x) for x in (axes, index, starts, ends)]
        return lib.cel_dev_prove_batch(handle, d_eds, d_index, k, n, *a, leaves, nodes, work, None)

    assert prove() == _lib.OK
    assert prove(handle=None) == _lib.EINVAL
    for nil in ("d_index", "axes", "index", "starts", "ends", "nodes", "work"):
        assert prove(**{nil: None}) == _lib.EINVAL, nil
        assert lib.cel_last_error(h).decode() == "nil argument"
    assert prove(d_eds=None) == _lib.EINVAL                    # shares wanted, no square
    assert prove(d_eds=None, leaves=None) == _lib.OK           # nodes only
    assert prove(leaves=ctypes.c_void_p(d_leaves.ptr.value + 8)) == _lib.EINVAL
    assert "16-byte aligned" in lib.cel_last_error(h).decode()
    assert prove(nodes=ctypes.c_void_p(d_nodes.ptr.value + 1)) == _lib.EINVAL
    assert prove(axes=u8(2)) == _lib.EINVAL and "proof 0: axis 2" in lib.cel_last_error(h).decode()
    assert prove(index=u32(w)) == _lib.EINVAL and "proof 0: tree 4" in lib.cel_last_error(h).decode()
    assert prove(ends=i32(w + 1)) == _lib.EINVAL and "proof 0: range [1, 5)" in lib.cel_last_error(h).decode()
    assert prove(starts=i32(-1)) == _lib.EINVAL and prove(starts=i32(3)) == _lib.EINVAL
    assert prove(n=2, axes=u8(0, 0), index=u32(0, 0), starts=i32(0, 2), ends=i32(1, 2)) == _lib.EINVAL
    assert "proof 1: range [2, 2)" in lib.cel_last_error(h).decode()
    assert prove(k=3) == _lib.ENOTPOW2 and prove(k=4096) == _lib.ETOOBIG
    assert prove(n=0) == _lib.OK and prove(n=0, axes=None, index=None, starts=None, ends=None, nodes=None) == _lib.OK

    rr, cr = DeviceBuffer(w * 90), DeviceBuffer(w * 90)

    def build(d_eds=idx.d_eds.ptr, k=k, d_index=idx.d_index.ptr, d_rr=rr.ptr, d_cr=cr.ptr, handle=h):
        return lib.cel_dev_tree_index_build(handle, d_eds, k, d_index, d_rr, d_cr, None, None, 0, None)

    assert build() == _lib.OK
    assert build(handle=None) == _lib.EINVAL
    for nil in ("d_eds", "d_index", "d_rr", "d_cr"):
        assert build(**{nil: None}) == _lib.EINVAL, nil
    assert build(k=3) == _lib.ENOTPOW2 and build(k=4096) == _lib.ETOOBIG
    assert lib.cel_dev_tree_index_size(3) == 0 and lib.cel_dev_tree_index_size(4096) == 0

    # the host entries
    shares, nodes, off = np.zeros((2, 512), np.uint8), np.zeros((8, 90), np.uint8), np.full(3, 7, np.uint64)

    def samples(rows=u32(0, 3), cols=u32(1, 2), axes=u8(0, 1), n=2, k=k, cells=eds, out=nodes):
        return lib.cel_prove_samples(h, None if cells is None else P(cells), k, n, P(rows), P(cols), P(axes), P(shares),
                                     None if out is None else P(out), P(off))

    assert samples() == _lib.OK and off.tolist() == [0, 2, 4]
    assert np.array_equal(shares[0], eds[0, 1]) and np.array_equal(shares[1], eds[3, 2])
    assert samples(rows=u32(0, w)) == _lib.EINVAL and "sample 1: cell (4, 2)" in lib.cel_last_error(h).decode()
    assert samples(cols=u32(2 ** 31, 0)) == _lib.EINVAL and samples(axes=u8(0, 2)) == _lib.EINVAL
    assert samples(cells=None) == _lib.EINVAL and samples(out=None) == _lib.EINVAL
    assert samples(k=3) == _lib.ENOTPOW2 and samples(k=4096) == _lib.ETOOBIG
    assert samples(n=0) == _lib.OK and off[0] == 0

    def ranges(ends=i32(2, 4), n=2, k=k, cells=eds):
        return lib.cel_prove_ranges(h, None if cells is None else P(cells), k, n, P(u8(0, 1)), P(u32(0, 3)), P(i32(0, 1)),
                                    P(ends), None, P(nodes))

    assert ranges() == _lib.OK
    assert ranges(ends=i32(2, w + 1)) == _lib.EINVAL and "proof 1: range [1, 5)" in lib.cel_last_error(h).decode()
    assert ranges(cells=None) == _lib.EINVAL and ranges(k=3) == _lib.ENOTPOW2 and ranges(n=0) == _lib.OK
