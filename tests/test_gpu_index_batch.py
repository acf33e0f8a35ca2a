"""GPU: the tree index and NMT proofs of many resident squares at once
(cel_dev_tree_index_build_batch, cel_dev_prove_squares, cel_prove_samples_squares,
proof.TreeIndexBatch, rsmt2d.SampleProofsBatch). The batch index is n single-square indexes back
to back, so the single-square calls are the reference throughout: every square's records and leaf
digests equal the single build's bytes, every slice serves the single-square calls unchanged, and
every proof byte equals what cel_dev_prove_batch gives on that square, scattered to the request
order. Roots and DAH are checked against the oracle; the device outputs go unchanged into the
device verifier."""
import ctypes

import numpy as np
import pytest

import verify_cases as vc
from eds_inputs import random_ods
from test_gpu_prove import COL, ROW, Index, _all_samples, _seeded_ranges

pytestmark = pytest.mark.gpu

P = vc._p
UNSET = 0x7F7F7F7F
_squares_cache = {}


def _squares(oracle, k, n, seed0=0):
    """n distinct squares of width k with the oracle's roots and DAH: [(eds, rr, cr, dah)]."""
    key = (k, n, seed0)
    if key not in _squares_cache:
        _squares_cache[key] = [oracle.extend_and_commit(random_ods(k, 9000 + 100 * k + seed0 + i)) for i in range(n)]
    return _squares_cache[key]


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


class Slice:
    """Square i of a batch index as the single-square calls take it: Index's prove and the
    namespace tests' Plan work on it as they do on an Index."""

    prove = Index.prove

    def __init__(self, batch, i):
        self.ctx, self.cells, self.w, self.k = batch.ctx, batch.cells[i], batch.w, batch.k
        self.d_eds = _At(ctypes.c_void_p(batch.d_eds.ptr.value + i * batch.cells[i].nbytes))
        self.d_index = _At(ctypes.c_void_p(batch.d_index.ptr.value + i * batch.size))


class BatchIndex:
    """The batch index of `cells` (n squares of one width) in device buffers. The roots share one
    buffer, all row roots [n][2k][90] then all column roots, so it is also the verifier's root
    table: root (square, axis, tree) is number axis * n * 2k + square * 2k + tree."""

    def __init__(self, ctx, cells, flags=0, want_dah=True, want_status=True):
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        self.ctx, self.cells = ctx, [np.ascontiguousarray(c) for c in cells]
        self.n, self.w = len(cells), cells[0].shape[0]
        self.k = self.w // 2
        n, w, lib = self.n, self.w, ctx.lib
        self.d_eds = DeviceBuffer(n * cells[0].nbytes)
        self.d_eds.upload(np.stack(self.cells))
        self.size = lib.cel_dev_tree_index_size(self.k)
        assert lib.cel_dev_tree_index_batch_size(self.k, n) == n * self.size and self.size % 16 == 0
        self.d_index = DeviceBuffer(n * self.size + 64, fill=0xEE)
        self.d_roots = DeviceBuffer(2 * n * w * 90)
        self.d_cr = ctypes.c_void_p(self.d_roots.ptr.value + n * w * 90)
        self.d_dah = DeviceBuffer(n * 32, fill=0xEE)
        status = np.full(n, UNSET, np.int32)
        st = lib.cel_dev_tree_index_build_batch(ctx.handle, self.d_eds.ptr, n, self.k, self.d_index.ptr, self.d_roots.ptr,
                                                self.d_cr, self.d_dah.ptr if want_dah else None,
                                                P(status) if want_status else None, flags, None)
        assert st == _lib.OK, lib.cel_last_error(ctx.handle).decode()
        synchronize()
        self.status = status.tolist()
        roots = self.d_roots.download((2, n, w, 90))
        self.rr, self.cr = roots[0], roots[1]
        self.dah = [d.tobytes() for d in self.d_dah.download((n, 32))]
        # 64 guard bytes behind the batch index stay untouched
        assert (self.d_index.download_at(n * self.size, (64,)) == 0xEE).all()
        self.tail = 2 * w * 32 + 48
        self.record_bytes = self.size - self.tail

    def records(self, i):
        return self.d_index.download_at(i * self.size, (self.record_bytes,))

    def leafd(self, i):
        return self.d_index.download_at(i * self.size + self.record_bytes, (2 * self.w * 32,))

    def tail_dah(self, i):
        return self.d_index.download_at(i * self.size + self.record_bytes + 2 * self.w * 32, (32,)).tobytes()

    def prove(self, squares, axes, index, starts, ends, leaves=True, node_shift=2):
        """cel_dev_prove_squares into 0xEE-filled buffers; d_nodes starts node_shift bytes into
        its buffer. Returns (leaves, nodes, leaf_off, node_off) and keeps the device buffers."""
        from celestia_eds import _lib
        from hipmem import DeviceBuffer, synchronize
        ctx = self.ctx
        squares = np.ascontiguousarray(squares, np.uint32)
        axes, index = np.ascontiguousarray(axes, np.uint8), np.ascontiguousarray(index, np.uint32)
        starts, ends = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(ends, np.int32)
        n = len(axes)
        leaf_off, node_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        assert ctx.lib.cel_prove_offsets(self.k, n, P(starts), P(ends), P(leaf_off), P(node_off)) == _lib.OK
        tl, tn = int(leaf_off[-1]), int(node_off[-1])
        self.d_leaves = DeviceBuffer(tl * 512 + 16, fill=0xEE)
        self.d_nodes = DeviceBuffer(node_shift + tn * 90 + 16, fill=0xEE)
        self.d_nodes_ptr = ctypes.c_void_p(self.d_nodes.ptr.value + node_shift)
        d_work = DeviceBuffer(ctx.lib.cel_dev_prove_squares_workspace_size(n) + 64, fill=0xEE)
        st = ctx.lib.cel_dev_prove_squares(ctx.handle, self.d_eds.ptr if leaves else None, self.d_index.ptr, self.k, self.n,
                                           n, P(squares), P(axes), P(index), P(starts), P(ends),
                                           self.d_leaves.ptr if leaves else None, self.d_nodes_ptr, d_work.ptr, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        assert (d_work.download_at(d_work.nbytes - 64, (64,)) == 0xEE).all(), "the request table outside its workspace"
        raw = self.d_nodes.download((self.d_nodes.nbytes,))
        assert (raw[:node_shift] == 0xEE).all() and (raw[node_shift + tn * 90:] == 0xEE).all(), "nodes outside their range"
        got = self.d_leaves.download((self.d_leaves.nbytes,))
        if leaves:
            assert (got[tl * 512:] == 0xEE).all(), "shares outside their range"
        else:
            assert (got == 0xEE).all(), "shares written without d_leaves"
        return got[:tl * 512].reshape(tl, 512), raw[node_shift:node_shift + tn * 90].reshape(tn, 90), leaf_off, node_off


def _single(ctx, cells, cache={}):
    """The single-square Index of a square, one per square and test session."""
    key = cells.tobytes()[:4096] + bytes(str(cells.shape), "ascii")
    if key not in cache:
        cache[key] = Index(ctx, cells)
    return cache[key]


def _index_bytes(idx):
    size = idx.ctx.lib.cel_dev_tree_index_size(idx.k)
    tail = 2 * idx.w * 32 + 48
    return idx.d_index.download((size - tail,)), idx.d_index.download_at(size - tail, (2 * idx.w * 32,))


def _check_square(batch, i, ref):
    """Slice i of the batch index equals the single build of the same cells; roots and DAH the oracle's."""
    eds, rr, cr, dah = ref
    assert np.array_equal(batch.rr[i], rr) and np.array_equal(batch.cr[i], cr), f"square {i}: roots differ"
    assert batch.dah[i] == dah, f"square {i}: DAH differs"
    records, leafd = _index_bytes(_single(batch.ctx, eds))
    assert np.array_equal(batch.records(i), records), f"square {i}: records differ from the single build"
    assert np.array_equal(batch.leafd(i), leafd), f"square {i}: leaf digests differ from the single build"


# ------------------------------------------------------------------------- 1. the build
@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_build_equals_single_builds(ctx, oracle, k):
    from celestia_eds import _lib
    refs = _squares(oracle, k, 3)
    cells = [r[0] for r in refs]
    for flags in (0, _lib.FLAG_ORDER_CHECK):
        batch = BatchIndex(ctx, cells, flags=flags)
        assert batch.status == [_lib.OK] * 3
        for i in range(3):
            _check_square(batch, i, refs[i])
    one = BatchIndex(ctx, cells[2:])  # n = 1
    assert one.status == [_lib.OK]
    _check_square(one, 0, refs[2])
    # no DAH wanted: it goes to each slice's tail; roots and status all the same
    quiet = BatchIndex(ctx, cells, flags=_lib.FLAG_ORDER_CHECK, want_dah=False)
    assert quiet.status == [_lib.OK] * 3 and all(d == b"\xee" * 32 for d in quiet.dah)
    for i in range(3):
        assert np.array_equal(quiet.rr[i], refs[i][1]) and np.array_equal(quiet.cr[i], refs[i][2])
        assert quiet.tail_dah(i) == refs[i][3]
    nostat = BatchIndex(ctx, cells, want_status=False)
    assert nostat.status == [UNSET] * 3 and [d for d in nostat.dah] == [r[3] for r in refs]
    if k == 1:
        return  # one Q0 share: nothing to swap
    # two Q0 shares of the middle square swapped: its status alone, and the others' bytes unchanged
    bad = cells[1].copy()
    bad[0, 0], bad[0, 1] = cells[1][0, 1], cells[1][0, 0]
    assert bad[0, 0, :29].tobytes() > bad[0, 1, :29].tobytes()
    for flags, want in ((0, [0, 0, 0]), (_lib.FLAG_ORDER_CHECK, [0, _lib.EORDER, 0])):
        for want_dah in (True, False):
            batch = BatchIndex(ctx, [cells[0], bad, cells[2]], flags=flags, want_dah=want_dah)
            assert batch.status == want
            for i in (0, 2):
                if want_dah:
                    _check_square(batch, i, refs[i])
                else:
                    assert np.array_equal(batch.rr[i], refs[i][1]) and batch.tail_dah(i) == refs[i][3]
            single = Index(ctx, bad, flags=flags)
            assert single.status == want[1]
            assert np.array_equal(batch.rr[1], single.rr) and np.array_equal(batch.cr[1], single.cr)
            records, leafd = _index_bytes(single)
            assert np.array_equal(batch.records(1), records) and np.array_equal(batch.leafd(1), leafd)


def test_build_of_67_squares(ctx, oracle):
    """Many squares, an odd count: every square's roots and DAH, three squares' records."""
    from celestia_eds import _lib
    k, n = 8, 67
    refs = _squares(oracle, k, n, seed0=500)
    batch = BatchIndex(ctx, [r[0] for r in refs], flags=_lib.FLAG_ORDER_CHECK)
    assert batch.status == [_lib.OK] * n
    for i in range(n):
        assert np.array_equal(batch.rr[i], refs[i][1]) and np.array_equal(batch.cr[i], refs[i][2]), i
        assert batch.dah[i] == refs[i][3], i
    for i in (0, 33, 66):
        _check_square(batch, i, refs[i])


# ------------------------------------------------- 2. a slice is a single-square index
def test_slices_serve_single_square_calls(ctx, oracle):
    import namespace_inputs as ni
    from celestia_eds import _lib
    from test_gpu_namespace import LAYOUTS, Plan
    k = 8
    odss = [ni.run_ods(k, LAYOUTS[k], 700 + i) for i in range(3)]
    cells = [oracle.extend_and_commit(o[0])[0] for o in odss]
    batch = BatchIndex(ctx, cells)
    view, single = Slice(batch, 1), Index(ctx, cells[1])
    reqs = _seeded_ranges(2 * k, 21) + _all_samples(2 * k)[::5]
    axes, index, starts, ends = zip(*reqs)
    got, want = view.prove(axes, index, starts, ends), single.prove(axes, index, starts, ends)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    queries = odss[1][1] + odss[1][2] + [ni.BELOW_ALL, ni.ABOVE_ALL]
    pa, pb = Plan(view, queries), Plan(single, queries)
    assert pa.status == pb.status == _lib.OK and pa.count.value == pb.count.value > 0
    for key, v in pa.arr.items():
        assert np.array_equal(v, pb.arr[key]), key
    for a, b in zip(pa.prove(), pb.prove()):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------- 3. proofs
def _requests(k, n, seed):
    """Each square's seeded ranges (and every single-leaf sample for k <= 8), shuffled across
    squares: [(square, axis, tree, start, end)]."""
    w = 2 * k
    reqs = []
    for sq in range(n):
        mine = _seeded_ranges(w, 31 * k + sq) + (_all_samples(w) if k <= 8 else [])
        reqs += [(sq,) + r for r in mine]
    order = np.random.default_rng(seed).permutation(len(reqs))
    return [reqs[i] for i in order]


def _expected(ctx, batch, reqs):
    """The single-square call on each square's requests, scattered to the request order."""
    n = len(reqs)
    leaves, nodes = [None] * n, [None] * n
    for sq in sorted({r[0] for r in reqs}):
        ids = [i for i, r in enumerate(reqs) if r[0] == sq]
        axes, index, starts, ends = zip(*[reqs[i][1:] for i in ids])
        lv, nd, lo, no = _single(ctx, batch.cells[sq]).prove(axes, index, starts, ends)
        for j, i in enumerate(ids):
            leaves[i] = lv[int(lo[j]):int(lo[j + 1])]
            nodes[i] = nd[int(no[j]):int(no[j + 1])]
    return np.concatenate(leaves), np.concatenate(nodes + [np.zeros((0, 90), np.uint8)])


def _check_requests(ctx, batch, reqs, **kw):
    sq, axes, index, starts, ends = zip(*reqs)
    leaves, nodes, leaf_off, node_off = batch.prove(sq, axes, index, starts, ends, **kw)
    want_leaves, want_nodes = _expected(ctx, batch, reqs)
    assert node_off[-1] == len(want_nodes) and leaf_off[-1] == len(want_leaves)
    assert np.array_equal(nodes, want_nodes), "proof nodes differ"
    if kw.get("leaves", True):
        assert np.array_equal(leaves, want_leaves), "shares differ"


@pytest.mark.parametrize("k", [2, 8, 32])
def test_proofs_equal_single_square_calls(ctx, oracle, k):
    refs = _squares(oracle, k, 3)
    batch = BatchIndex(ctx, [r[0] for r in refs])
    reqs = _requests(k, 3, seed=k)
    assert len({r[0] for r in reqs[:8]}) > 1  # shuffled across squares
    _check_requests(ctx, batch, reqs)                      # d_nodes 2 mod 4
    _check_requests(ctx, batch, reqs[:1])
    _check_requests(ctx, batch, reqs[:257], node_shift=6)  # a workgroup holds four proofs: the last is partial
    _check_requests(ctx, batch, reqs[:300], leaves=False)  # nodes alone: the share buffer untouched
    # all requests on one square: byte for byte cel_dev_prove_batch on that slice
    mine = [r for r in reqs if r[0] == 2][:400]
    sq, axes, index, starts, ends = zip(*mine)
    got = batch.prove(sq, axes, index, starts, ends)
    want = Slice(batch, 2).prove(axes, index, starts, ends)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ----------------------------------------------------------- 4. into the device verifier
def test_proofs_feed_device_verifier(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    k, n_sq = 8, 3
    w = 2 * k
    refs = _squares(oracle, k, n_sq)
    batch = BatchIndex(ctx, [r[0] for r in refs])
    rng = np.random.default_rng(44)
    reqs = [(sq,) + r for sq in range(n_sq) for r in _all_samples(w)]
    for _ in range(150):  # multi-leaf ranges inside the parity half of a tree: one namespace
        sq, axis, t = int(rng.integers(0, n_sq)), int(rng.integers(0, 2)), int(rng.integers(0, w))
        s = int(rng.integers(0 if t >= k else k, w - 1))
        reqs.append((sq, axis, t, s, int(rng.integers(s + 2, w + 1))))
    reqs = [reqs[i] for i in rng.permutation(len(reqs))]
    sq, axes, index, starts, ends = (np.array(x) for x in zip(*reqs))
    leaves, nodes, leaf_off, node_off = batch.prove(sq, axes, index, starts, ends)
    n = len(reqs)
    ns = np.full((n, 29), 0xFF, np.uint8)
    for i, (q, axis, t, s, e) in enumerate(reqs):
        r, c = (t, s) if axis == ROW else (s, t)
        if e - s == 1 and r < k and c < k:
            ns[i] = refs[q][0][r, c, :29]
    st32, en32 = starts.astype(np.int32), ends.astype(np.int32)
    d_ok = DeviceBuffer(n, fill=0xEE)
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(int(leaf_off[-1]), int(node_off[-1]), n))

    def verify(square_of):
        root_idx = (axes * n_sq * w + square_of * w + index).astype(np.uint32)
        st = ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(st32), P(en32), P(ns), batch.d_leaves.ptr, P(leaf_off),
                                              batch.d_nodes_ptr, P(node_off), batch.d_roots.ptr, 2 * n_sq * w, P(root_idx),
                                              d_ok.ptr, d_work.ptr, None)
        assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
        synchronize()
        return d_ok.download((n,))

    assert (verify(sq) == 1).all(), "a produced proof does not verify against its square's root"
    assert (verify((sq + 1) % n_sq) == 0).all(), "a proof verifies against another square's root"


# ------------------------------------------------------------------------- 6. errors
def test_build_and_prove_call_errors(ctx, oracle):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    k, n = 2, 2
    w = 2 * k
    refs = _squares(oracle, k, 3)[:n]
    batch = BatchIndex(ctx, [r[0] for r in refs])
    lib, h = ctx.lib, ctx.handle
    err = lambda: lib.cel_last_error(h).decode()
    d_index = DeviceBuffer(n * batch.size + 64, fill=0xEE)
    d_roots = DeviceBuffer(2 * n * w * 90, fill=0xEE)
    d_cr = ctypes.c_void_p(d_roots.ptr.value + n * w * 90)

    def build(handle=h, d_eds=batch.d_eds.ptr, n=n, k=k, d_index=d_index.ptr, d_rr=d_roots.ptr, d_cr=d_cr):
        return lib.cel_dev_tree_index_build_batch(handle, d_eds, n, k, d_index, d_rr, d_cr, None, None, 0, None)

    assert build(handle=None) == _lib.EINVAL
    for kw in (dict(d_eds=None), dict(d_index=None), dict(d_rr=None), dict(d_cr=None)):
        assert build(**kw) == _lib.EINVAL and err() == "nil argument", kw
    assert build(d_index=ctypes.c_void_p(d_index.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert build(d_rr=ctypes.c_void_p(d_roots.ptr.value + 1)) == _lib.EINVAL and "2-byte aligned" in err()
    for bad_k in (0, 3, 1024):
        assert build(k=bad_k) == _lib.EINVAL and "power of two" in err()
    assert build(n=65536) == _lib.EINVAL and "more than one call takes" in err()
    assert build(n=0, d_eds=None, d_index=None) == _lib.OK
    synchronize()
    assert (d_index.download((d_index.nbytes,)) == 0xEE).all() and (d_roots.download((d_roots.nbytes,)) == 0xEE).all()

    u8 = lambda *v: np.array(v, np.uint8)
    u32 = lambda *v: np.array(v, np.uint32)
    i32 = lambda *v: np.array(v, np.int32)
    d_leaves, d_nodes = DeviceBuffer(1 << 14, fill=0xEE), DeviceBuffer(1 << 14, fill=0xEE)
    d_work = DeviceBuffer(lib.cel_dev_prove_squares_workspace_size(2), fill=0xEE)

    def prove(handle=h, d_eds=batch.d_eds.ptr, d_index=batch.d_index.ptr, k=k, n_squares=n, n=2, squares=u32(1, 0),
              axes=u8(0, 1), index=u32(1, 2), starts=i32(1, 0), ends=i32(3, 4), leaves=d_leaves.ptr, nodes=d_nodes.ptr,
              work=d_work.ptr):
        ptr = lambda a: None if a is None else P(a)
        return lib.cel_dev_prove_squares(handle, d_eds, d_index, k, n_squares, n, ptr(squares), ptr(axes), ptr(index),
                                         ptr(starts), ptr(ends), leaves, nodes, work, None)

    def untouched():
        synchronize()
        return all((b.download((b.nbytes,)) == 0xEE).all() for b in (d_leaves, d_nodes, d_work))

    assert prove(handle=None) == _lib.EINVAL
    assert prove(squares=u32(1, 2)) == _lib.EINVAL and err() == "proof 1: square 2 of 2"
    assert prove(n_squares=0) == _lib.EINVAL and err() == "proof 0: square 1 of 0"
    for kw in (dict(d_index=None), dict(squares=None), dict(axes=None), dict(index=None), dict(starts=None),
               dict(ends=None), dict(nodes=None), dict(work=None), dict(d_eds=None)):
        assert prove(**kw) == _lib.EINVAL and err() == "nil argument", kw
    assert prove(leaves=ctypes.c_void_p(d_leaves.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert prove(work=ctypes.c_void_p(d_work.ptr.value + 8)) == _lib.EINVAL and "16-byte aligned" in err()
    assert prove(nodes=ctypes.c_void_p(d_nodes.ptr.value + 1)) == _lib.EINVAL and "2-byte aligned" in err()
    for bad_k in (0, 3, 1024):
        assert prove(k=bad_k) == _lib.EINVAL and "power of two" in err()
    assert prove(n_squares=65536) == _lib.EINVAL and "more than one call takes" in err()
    assert prove(axes=u8(0, 2)) == _lib.EINVAL and err() == "proof 1: axis 2"
    assert prove(index=u32(1, w)) == _lib.EINVAL and err() == f"proof 1: tree {w} of {w}"
    for s, e in ((-1, 2), (2, 2), (3, 1), (0, w + 1)):
        assert prove(starts=i32(1, s), ends=i32(3, e)) == _lib.EINVAL
        assert err() == f"proof 1: range [{s}, {e}) is not a range of {w} leaves"
    assert untouched(), "a rejected call wrote to the device"
    assert prove(n=0, squares=None, axes=None, index=None, starts=None, ends=None) == _lib.OK
    assert prove(n=0, n_squares=0, d_index=None, d_eds=None) == _lib.OK and untouched()
    assert prove() == _lib.OK
    assert prove(d_eds=None, leaves=None) == _lib.OK
    synchronize()

    # the host-memory form
    eds = np.stack([r[0] for r in refs])
    shares, nodes, off = np.full((2, 512), 0x5A, np.uint8), np.full((4, 90), 0x5A, np.uint8), np.full(3, 0x5A, np.uint64)

    def samples(squares=u32(1, 0), rows=u32(0, 3), cols=u32(1, 2), axes=u8(0, 1), n=2, k=k, n_squares=n, cells=eds):
        return lib.cel_prove_samples_squares(h, None if cells is None else P(cells), n_squares, k, n, P(squares), P(rows),
                                             P(cols), P(axes), P(shares), P(nodes), P(off))

    assert samples(squares=u32(1, 2)) == _lib.EINVAL and err() == "sample 1: square 2 of 2"
    assert samples(rows=u32(0, w)) == _lib.EINVAL and "outside the square" in err()
    assert samples(axes=u8(0, 2)) == _lib.EINVAL and samples(k=3) == _lib.EINVAL and samples(cells=None) == _lib.EINVAL
    assert (shares == 0x5A).all() and (nodes == 0x5A).all() and (off == 0x5A).all()
    assert samples() == _lib.OK, err()
    assert off.tolist() == [0, 2, 4] and shares[0].tobytes() == refs[1][0][0, 1].tobytes()
    assert shares[1].tobytes() == refs[0][0][3, 2].tobytes()
    assert samples(n=0) == _lib.OK and off[0] == 0


# ------------------------------------------------------------------------- 7. Python
def test_tree_index_batch_python(ctx, oracle):
    import namespace_inputs as ni
    from celestia_eds import _lib, proof
    from celestia_eds._lib import CelError
    from test_gpu_namespace import LAYOUTS
    widths = [2, 8, 2, 4]
    odss = [ni.run_ods(k, LAYOUTS[k], 40 + i) for i, k in enumerate(widths)]
    refs = [oracle.extend_and_commit(o[0]) for o in odss]
    cells = [r[0] for r in refs]
    batch = proof.TreeIndexBatch(cells, ctx=ctx, order_check=True)
    singles = [proof.TreeIndex(c, ctx=ctx) for c in cells]
    assert batch.status == [_lib.OK] * 4
    for i, (eds, rr, cr, dah) in enumerate(refs):
        assert batch.row_roots[i] == [r.tobytes() for r in rr] and batch.col_roots[i] == [c.tobytes() for c in cr]
        assert batch.dah[i] == dah
    rng = np.random.default_rng(4)
    samples = [(sq, int(rng.integers(0, 2 * widths[sq])), int(rng.integers(0, 2 * widths[sq])), int(rng.integers(0, 2)))
               for sq in rng.integers(0, 4, 60)]
    samples = [(int(sq), r, c, a) for sq, r, c, a in samples]
    assert {s[0] for s in samples} == {0, 1, 2, 3}
    got = batch.prove_samples(samples)
    for (sq, r, c, a), g in zip(samples, got):
        assert g == singles[sq].prove_samples([(r, c, a)])[0]
    queries = [(sq, ns) for sq in (3, 1, 0, 2, 1) for ns in odss[sq][1][:3] + odss[sq][2][:2] + [ni.BELOW_ALL, ni.ABOVE_ALL]]
    rows = batch.namespace_rows(queries)
    assert any(rows) and len(rows) == len(queries)
    for (sq, ns), g in zip(queries, rows):
        want = singles[sq].namespace_rows([ns])[0]
        assert [(r, p.Start, p.End, p.Nodes, p.LeafHash, s) for r, p, s in g] == \
               [(r, p.Start, p.End, p.Nodes, p.LeafHash, s) for r, p, s in want]
    assert batch.prove_samples([]) == [] and batch.namespace_rows([]) == []
    with pytest.raises(CelError):
        batch.prove_samples([(4, 0, 0, 0)])
    with pytest.raises(CelError):
        batch.prove_samples([(1, 16, 0, 0)])
    # an unordered square keeps its status; the others are served, it is not
    bad = cells[1].copy()
    bad[0, 0], bad[0, 3] = cells[1][0, 3].copy(), cells[1][0, 0].copy()  # the first run is three shares long
    assert bad[0, 0, :29].tobytes() > bad[0, 1, :29].tobytes()
    mixed = proof.TreeIndexBatch([cells[0], bad, cells[3]], ctx=ctx, order_check=True)
    assert mixed.status == [_lib.OK, _lib.EORDER, _lib.OK]
    assert mixed.prove_samples([(2, 1, 1, 0)]) == [singles[3].prove_samples([(1, 1, 0)])[0]]
    with pytest.raises(CelError) as e:
        mixed.prove_samples([(0, 0, 0, 0), (1, 0, 0, 0)])
    assert e.value.status == _lib.EORDER
    with pytest.raises(CelError):
        mixed.namespace_rows([(1, odss[1][1][0])])


def test_sample_proofs_batch_to_repair(ctx, oracle):
    from celestia_eds.rsmt2d import ExtendedDataSquare, RepairFromSamples, SampleProofsBatch
    ks = [4, 8, 4]
    refs = [oracle.extend_and_commit(random_ods(k, 60 + i)) for i, k in enumerate(ks)]
    squares = [ExtendedDataSquare(r[0], ctx=ctx) for r in refs]
    k, w = 8, 16
    present = (np.random.default_rng(8).random((w, w)) < 0.6).astype(np.uint8)
    coords = [(1, int(r), int(c), i % 2) for i, (r, c) in enumerate(zip(*np.nonzero(present)))]
    others = [(0, 1, 2, 0), (2, 7, 0, 1), (0, 0, 0, 1)]
    samples = coords[:20] + others + coords[20:]
    got = SampleProofsBatch(squares, samples, ctx=ctx)
    assert [g[:4] for g in got] == samples
    for g in got[20:23]:  # each is what the square's own SampleProofs gives
        assert g[1:] == squares[g[0]].SampleProofs([g[1:4]])[0]
    mine = [g[1:] for g in got if g[0] == 1]
    assert mine[:5] == squares[1].SampleProofs([s[1:] for s in coords[:5]])
    eds, rr, cr, _ = refs[1]
    out, ok = RepairFromSamples(k, mine, [r.tobytes() for r in rr], [c.tobytes() for c in cr], ctx=ctx)
    assert all(ok) and len(ok) == int(present.sum())
    assert np.array_equal(out.cells, eds)
    assert SampleProofsBatch(squares, [], ctx=ctx) == []
