"""GPU: blobs out of a resident square (cel_dev_blobs_plan / cel_dev_blobs_emit, TreeIndex.blobs,
celestia_eds.blob, ExtendedDataSquare.Blobs). The checker is the host parser
blob.parse_sparse_shares (pinned in test_blob_parse.py) and the existing CreateCommitments.

The edge lengths at k = 16 leave out the 70,000-byte blob: EDGE_LENGTHS need 327 shares and a
16 x 16 square has 256. That blob runs at k = 32 and in the scan-boundary test."""
import ctypes

import numpy as np
import pytest

import block_inputs as B
import blob_cases as C
import commitment_ref
from celestia_eds import _lib, blob, block, inclusion, proof
from celestia_eds.rsmt2d import ExtendedDataSquare

pytestmark = pytest.mark.gpu

TAIL = C.padding(B.TAIL_PAD_NS)[0]


def square(ods, k, fill=0):
    """A (2k, 2k, 512) square with Q0 = ods ([k*k][512]) and `fill` everywhere else."""
    eds = np.full((2 * k, 2 * k, B.SHARE), fill, np.uint8)
    eds[:k, :k] = np.asarray(ods, np.uint8).reshape(k, k, B.SHARE)
    return eds


def tail_filled(k, pieces):
    """A k*k ODS of tail padding with the shares of pieces[i][1] written from pieces[i][0] on."""
    ods = np.tile(TAIL, (k * k, 1))
    for at, sh in pieces:
        ods[at:at + len(sh)] = sh
    return ods


def mirror(ods, ranges):
    """Per range [(ns, data, ODS index, shares)] or the error kind."""
    out = []
    for a, b in ranges:
        try:
            out.append([(g.namespace, g.data, g.index + a, g.shares) for g in blob.parse_sparse_shares(ods[a:b])])
        except blob.BlobParseError as e:
            out.append(e.kind)
    return out


def check_against_mirror(ctx, ods, k, ranges):
    index = proof.TreeIndex(square(ods, k), ctx=ctx)
    want = mirror(ods, ranges)
    recs, status, data, com = index.blobs_flat(ranges)
    assert [int(s) for s in status] == [w if isinstance(w, int) else 0 for w in want]
    flat = [(r, b) for r, w in enumerate(want) if not isinstance(w, int) for b in w]
    assert len(recs) == len(flat)
    at = 0
    for rec, (r, (ns, d, start, shares)) in zip(recs, flat):
        assert (rec.range, rec.start, rec.shares, rec.share_version, rec.len) == (r, start, shares, 0, len(d))
        assert bytes(rec.ns) == ns + bytes(3)
        assert rec.data_off == at and at % 16 == 0
        assert data[at:at + len(d)].tobytes() == d
        at += (len(d) + 15) // 16 * 16
        assert not data[rec.data_off + len(d):at].any(), "the bytes up to the next multiple of 16 are zero"
    assert len(data) == at
    if flat:
        assert [c.tobytes() for c in com] == inclusion.CreateCommitments([(ns, d) for _, (ns, d, _, _) in flat], ctx=ctx)
    return index, want


@pytest.fixture(scope="module")
def b408(ctx):
    txs = B.block408_txs()
    b = block.block_extend(ctx, txs, want_eds=True)
    from celestia_eds import square as sq
    carried = [(ns, data) for tx in txs if sq.is_blob_tx(tx) for ns, data, _ in commitment_ref.blob_tx_blobs(tx)]
    want_com = [c for _, c in inclusion.BlobTxCommitments(txs, ctx=ctx)]
    assert len(want_com) == len(carried) > 0
    return b, proof.TreeIndex(b.eds, ctx=ctx), carried, want_com


def test_block408_blob_service(ctx, b408):
    b, index, carried, want_com = b408
    namespaces = sorted({ns for ns, _ in carried})
    got = blob.GetAll(index, namespaces)
    assert sorted((g.namespace, g.data, g.commitment) for g in got) == \
        sorted((ns, d, c) for (ns, d), c in zip(carried, want_com))
    by_com = {g.commitment: g for g in got}
    for (ns, d), c in zip(carried, want_com):
        g = blob.Get(index, ns, c)
        assert (g.namespace, g.data, g.index) == (ns, d, by_com[c].index)
        assert blob.Included(index, ns, c)
        flipped = bytes([c[0] ^ 1]) + c[1:]
        assert not blob.Included(index, ns, flipped)
        with pytest.raises(blob.BlobNotFound):
            blob.Get(index, ns, flipped)
    # the proofs of every blob's shares, row by row, against the block's row roots
    proofs, nss, leaves, roots = [], [], [], []
    for g in got:
        for row, p in blob.GetProof(index, g):
            proofs.append(p)
            nss.append(g.namespace)
            leaves.append([b.eds[row, c].tobytes() for c in range(p.Start, p.End)])
            roots.append(b.row_roots[row].tobytes())
        n = blob.sparse_shares_needed(len(g.data))
        assert sum(p.End - p.Start for _, p in blob.GetProof(index, g)) == n == g.shares
    assert all(proof.VerifyInclusionBatch(proofs, nss, leaves, roots, ctx=ctx)) and proofs
    with pytest.raises(_lib.CelError) as e:
        blob.GetAll(index, [proof.PFB_NAMESPACE])
    assert e.value.status == _lib.EINVAL


def test_host_memory_form_equals_the_device_form(ctx, b408):
    b, index, carried, _ = b408
    absent = bytes(19) + b"\x07" * 10
    namespaces = sorted({ns for ns, _ in carried}) + [absent]
    eds = ExtendedDataSquare(b.eds, b.row_roots, b.col_roots, ctx=ctx)
    host = eds.Blobs(namespaces)
    ranges = blob.ods_ranges(index.k, len(namespaces), index.namespace_flat(namespaces))
    assert host == index.blobs(ranges) and host[-1] == [] and sum(len(h) for h in host) == len(carried)
    assert blob.GetAll(eds, namespaces) == blob.GetAll(index, namespaces)


@pytest.mark.parametrize("k", [16, 32])
def test_edge_lengths(ctx, k):
    lengths = B.EDGE_LENGTHS if k == 32 else [n for n in B.EDGE_LENGTHS if n != 70000]
    raw, segs = B.blob_layout(lengths, k, 100 + k)
    ods = B.expand(raw, k, segs, None)
    _, want = check_against_mirror(ctx, ods, k, [(0, k * k)])
    assert [len(d) for _, d, _, _ in want[0]] == lengths


def test_scan_boundaries(ctx):
    k = 32
    rng = np.random.default_rng(7)
    # more blobs than a scan block of 256: every share a blob
    lengths = [int(n) for n in rng.integers(1, B.FIRST + 1, k * k)]
    raw, segs = B.blob_layout(lengths, k, 8)
    _, want = check_against_mirror(ctx, B.expand(raw, k, segs, None), k, [(0, k * k)])
    assert len(want[0]) == k * k
    # one blob of 146 shares from share 200 on: across position 256 and four row ends
    lengths = [int(n) for n in rng.integers(1, B.FIRST + 1, 200)] + [70000] + [300] * 50
    raw, segs = B.blob_layout(lengths, k, 9)
    assert segs[200].start == 200 and segs[200].count == 146
    ods = B.expand(raw, k, segs, None)
    check_against_mirror(ctx, ods, k, [(0, k * k)])
    check_against_mirror(ctx, ods, k, [(190, 400), (200, 346)])  # the scan block boundary moves with the range


@pytest.mark.parametrize("k", [1, 2])
def test_smallest_squares(ctx, k):
    sh, _ = C.blob_shares([300] if k == 1 else [300, 900], 30 + k)
    ods = tail_filled(k, [(0, sh)])
    _, want = check_against_mirror(ctx, ods, k, [(0, k * k)])
    assert len(want[0]) == k


def test_range_geometry(ctx):
    k = 8
    raw, segs = B.blob_layout([100, 2000, 478, 5000, 30, 479, 960], k, 41)
    ods = B.expand(raw, k, segs, None)
    starts = [s.start for s in segs if s.kind == B.SEG_BLOB]
    inside = starts[1] + 2  # a continuation of the second blob
    ranges = [(0, k * k),
              (starts[1], starts[4]),        # starts and ends in the middle of rows
              (starts[3], starts[3] + 11),   # the whole of one blob, across a row end
              (starts[1], starts[4]),        # repeated
              (starts[2], k * k),            # overlaps the others
              (5, 5),                        # empty
              (inside, starts[3]),           # begins with a continuation
              (starts[3], starts[3] + 4)]    # ends inside a blob
    _, want = check_against_mirror(ctx, ods, k, ranges)
    assert want[6] == blob.ENOSTART and want[7] == blob.ESHORT and want[5] == [] and want[1] == want[3]
    assert len(want[2]) == 1 and len(want[2][0][1]) == 5000
    index = proof.TreeIndex(square(ods, k), ctx=ctx)
    assert index.blobs([]) == []
    recs, status, data, com = index.blobs_flat([])
    assert (len(recs), len(status), len(data)) == (0, 0, 0)
    assert index.blobs([(3, 3), (0, 0)]) == [[], []]  # only empty ranges


def test_only_q0_is_read(ctx):
    k = 8
    raw, segs = B.blob_layout([1443, 700, 3000, 5], k, 43)
    ods = B.expand(raw, k, segs, None)
    ranges = [(0, k * k), (4, 13)]  # the second one: the blobs of 700 and 3000 bytes
    outs = []
    for fill in (0, 0xA5):
        index = proof.TreeIndex(square(ods, k, fill), ctx=ctx)
        recs, status, data, com = index.blobs_flat(ranges)
        outs.append(([bytes(r) for r in recs], status.tobytes(), data.tobytes(), com.tobytes()))
    assert outs[0] == outs[1] and len(outs[0][0]) == 6


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_malformed_cells(ctx, case):
    k = 4
    sh = case.shares()
    ods = tail_filled(k, [(3, sh)])
    _, want = check_against_mirror(ctx, ods, k, [(3, 3 + len(sh))])
    assert want[0] == (case.error or [(ns, d, i + 3, n) for ns, d, i, n in case.want()])


def test_bad_ranges_leave_the_good_ones_alone(ctx):
    k = 8
    good, _ = C.blob_shares([1000, 40, 478], 50)
    pieces, ranges, at = [], [], 0
    for sh in (good, C.CASES[8].shares(), good, C.CASES[0].shares(), C.CASES[10].shares(), good):
        pieces.append((at, sh))
        ranges.append((at, at + len(sh)))
        at += len(sh) + 1
    ods = tail_filled(k, pieces)
    _, want = check_against_mirror(ctx, ods, k, ranges)
    assert want[1] == blob.ESHORT and want[3] == blob.ENOSTART and want[4] == blob.EVERSION
    assert want[0] == [(ns, d, i, n) for ns, d, i, n in want[0]] and len(want[0]) == len(want[2]) == len(want[5]) == 3
    # the length of 0xFFFFFFFF adds nothing to the total: the same ranges without it
    index = proof.TreeIndex(square(ods, k), ctx=ctx)
    got = index.blobs(ranges, commitments=False)
    assert [g.kind if isinstance(g, blob.BlobParseError) else [(b.namespace, b.data, b.index, b.shares) for b in g]
            for g in got] == want and got[0][0].commitment is None
    total = lambda rs: len(index.blobs_flat(rs, commitments=False)[2])
    assert total(ranges) == total([r for i, r in enumerate(ranges) if i != 1]) == 3 * (1008 + 48 + 480)


def _plan(index, starts, ends, cap, recs, status=None):
    c = index.ctx
    n = len(starts)
    s, e = np.array(starts or [0], np.uint32), np.array(ends or [0], np.uint32)
    total = int(sum(b - a for a, b in zip(starts, ends)))
    import torch
    d_work = torch.empty((max(c.lib.cel_dev_blobs_workspace_size(total, n), 16),), dtype=torch.uint8, device=index._dev)
    cnt, tb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    st = c.lib.cel_dev_blobs_plan(c.handle, index._ptr(index.d_eds), index.k, n, s.ctypes.data_as(ctypes.c_void_p),
                                  e.ctypes.data_as(ctypes.c_void_p), cap, recs,
                                  status.ctypes.data_as(ctypes.c_void_p) if status is not None else None,
                                  ctypes.byref(cnt), ctypes.byref(tb), index._ptr(d_work), index._stream_ptr())
    return st, cnt.value, tb.value, d_work


def test_abi_conventions(ctx):
    import torch
    k = 8
    lengths = [100, 2000, 478]
    raw, segs = B.blob_layout(lengths, k, 60)
    index = proof.TreeIndex(square(B.expand(raw, k, segs, None), k), ctx=ctx)
    c, lib = index.ctx, index.ctx.lib
    nbytes = sum((n + 15) // 16 * 16 for n in lengths)
    # count only
    st, cnt, tb, _ = _plan(index, [0], [k * k], 0, None)
    assert (st, cnt, tb) == (_lib.OK, 3, nbytes)
    # a short cap: CEL_EINVAL with both numbers, the counts still set
    recs = (blob.BlobRec * 2)()
    status = np.full(1, 77, np.uint32)
    st, cnt, tb, _ = _plan(index, [0], [k * k], 2, recs, status)
    assert (st, cnt, tb) == (_lib.EINVAL, 3, nbytes) and status[0] == 0
    msg = lib.cel_last_error(c.handle).decode()
    assert "2" in msg.split() and "3" in msg.split(), msg
    # n_ranges = 0; bad ranges and widths
    assert _plan(index, [], [], 0, None)[:3] == (_lib.OK, 0, 0)
    assert _plan(index, [5], [4], 0, None)[0] == _lib.EINVAL
    assert _plan(index, [0], [k * k + 1], 0, None)[0] == _lib.EINVAL
    s = np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cnt, tb = ctypes.c_uint64(), ctypes.c_uint64()
    d_work = torch.empty((1 << 16,), dtype=torch.uint8, device=index._dev)
    plan = lambda kk, eds, work, nb=ctypes.byref(cnt): lib.cel_dev_blobs_plan(
        c.handle, eds, kk, 1, p(s), p(s), 0, None, None, nb, ctypes.byref(tb), work, index._stream_ptr())
    assert plan(3, index._ptr(index.d_eds), index._ptr(d_work)) == _lib.EINVAL
    assert plan(1024, index._ptr(index.d_eds), index._ptr(d_work)) == _lib.EINVAL
    assert plan(k, None, index._ptr(d_work)) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), None) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), index._ptr(d_work), None) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), ctypes.c_void_p(d_work.data_ptr() + 4)) == _lib.EINVAL
    assert lib.cel_dev_blobs_workspace_size(1 << 31, 1) == 0 and lib.cel_dev_blobs_workspace_size(0, 0) > 0
    # the emit call: a NULL d_commitments gives the bytes alone; it runs over no more blobs than
    # the plan holds, whatever it is passed
    recs = (blob.BlobRec * 3)()
    st, cnt, tb, d_work = _plan(index, [0], [k * k], 3, recs)
    assert st == _lib.OK
    d_data = torch.full((nbytes + 64,), 0xCC, dtype=torch.uint8, device=index._dev)
    emit = lambda n, data, work: lib.cel_dev_blobs_emit(c.handle, index._ptr(index.d_eds), k, n, data, None, 64, work,
                                                        None, index._stream_ptr())
    assert emit(1000, index._ptr(d_data), index._ptr(d_work)) == _lib.OK
    index._stream.synchronize()
    got = d_data.cpu().numpy()
    assert (got[nbytes:] == 0xCC).all(), "nothing is written past the plan's bytes"
    for r, n in zip(recs, lengths):
        assert r.len == n and got[r.data_off:r.data_off + n].tobytes() == raw[:n]
        raw = raw[n:]
    # the first blob alone
    d_data.fill_(0xCC)
    assert emit(1, index._ptr(d_data), index._ptr(d_work)) == _lib.OK
    index._stream.synchronize()
    assert (d_data.cpu().numpy()[112:] == 0xCC).all()
    # a workspace that holds no plan of this context, a nil and a misaligned buffer
    other = torch.empty((1 << 16,), dtype=torch.uint8, device=index._dev)
    assert emit(3, index._ptr(d_data), index._ptr(other)) == _lib.EINVAL
    assert emit(3, None, index._ptr(d_work)) == _lib.EINVAL
    assert emit(3, ctypes.c_void_p(d_data.data_ptr() + 8), index._ptr(d_work)) == _lib.EINVAL
    assert emit(0, None, None) == _lib.OK
