"""GPU: the block path from txs (cel_block_extend, cel_dev_square_build, celestia_eds.block),
bit-exact against the three-call path it replaces: cel_blob_tx_commitments,
cel_square_construct (the host byte builder) and cel_extend_shares."""
import ctypes

import numpy as np
import pytest

import block_inputs as B
from square_inputs import block408_txs, random_block

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Result:
    pass


def block_extend(ctx, txs, max_square_size=128, greedy=0, eds="none", cap=None, flags=1, txs_at=None):
    """cel_block_extend through the raw ABI. eds: "none" | "full" | "parity" (FLAG_PARITY_ONLY,
    buffer pre-filled with 0x5A); cap: commitment capacity (None = exactly the blob count, 0 =
    skip). Outputs are sized for max_square_size and pre-filled, so what is written shows.
    txs_at: a pointer to a copy of the concatenated txs that the call reads instead."""
    import celestia_eds._lib as L
    l = ctx.lib
    buf, lens, ntx, _ = B.pack(txs)
    if txs_at is not None:
        buf = txs_at
    r = Result()
    k, n = ctypes.c_uint32(), ctypes.c_uint32()
    inc = (ctypes.c_uint8 * max(ntx, 1))()
    if cap is None:
        assert l.cel_blob_tx_commitments(ctx.handle, buf, lens, ntx, 64, None, None, 0, ctypes.byref(n)) == 0
        cap = n.value
    rr = np.full((2 * max_square_size, 90), 0xC3, np.uint8)
    cr = np.full((2 * max_square_size, 90), 0xC3, np.uint8)
    dah = np.zeros(32, np.uint8)
    com = np.zeros((max(cap, 1), 32), np.uint8)
    txi = np.zeros(max(cap, 1), np.uint32)
    eds_buf, eds_cap = None, 0
    if eds != "none":
        _, _, kk, _, _, _ = B.layout(txs, max_square_size, 64, greedy)
        eds_buf = np.full((2 * kk, 2 * kk, 512), 0x5A, np.uint8)
        eds_cap = eds_buf.nbytes
        if eds == "parity":
            flags |= L.FLAG_PARITY_ONLY
    r.status = l.cel_block_extend(ctx.handle, buf, lens, ntx, max_square_size, 64, greedy, ctypes.byref(k), inc,
                                  _p(rr), _p(cr), _p(dah), _p(eds_buf) if eds_buf is not None else None, eds_cap,
                                  _p(com) if cap else None, _p(txi) if cap else None, cap, ctypes.byref(n), flags)
    r.error = l.cel_last_error(ctx.handle).decode() if r.status else ""
    r.k, r.included = k.value, [int(inc[i]) for i in range(ntx)]
    r.row_roots, r.col_roots, r.dah, r.eds = rr, cr, dah.tobytes(), eds_buf
    r.commitments = [(int(txi[i]), com[i].tobytes()) for i in range(min(cap, n.value))]
    r.n_commit = n.value
    return r


def three_calls(ctx, txs, max_square_size=128, greedy=0, commitments=True):
    """The path cel_block_extend replaces, on the kept txs' square."""
    from celestia_eds import da, inclusion
    st, err, k, included, shares = B.construct(txs, max_square_size, 64, greedy)
    r = Result()
    r.status, r.error, r.k, r.included, r.shares = st, err, k, included, shares
    if st == 0:
        e = da._extend(shares, ctx=ctx)
        r.row_roots, r.col_roots, r.dah, r.eds = e._row_roots, e._col_roots, e._dah, e.cells
        r.commitments = inclusion.BlobTxCommitments(txs, ctx=ctx) if commitments else None
    return r


def assert_same(got, want, commitments=True):
    assert (got.status, got.error, got.k, got.included) == (want.status, want.error, want.k, want.included)
    if want.status:
        return
    k = want.k
    assert np.array_equal(got.row_roots[:2 * k], want.row_roots) and np.array_equal(got.col_roots[:2 * k], want.col_roots)
    assert (got.row_roots[2 * k:] == 0xC3).all() and (got.col_roots[2 * k:] == 0xC3).all()  # 2k roots written, no more
    assert got.dah == want.dah
    if got.eds is not None:
        assert np.array_equal(got.eds[:k, :k].reshape(k * k, 512), want.shares), "Q0 differs from the host square"
        assert np.array_equal(got.eds, want.eds.reshape(got.eds.shape))
    if commitments:
        assert got.commitments == want.commitments


def test_block408(ctx, golden):
    txs = block408_txs()
    got = block_extend(ctx, txs, eds="full")
    want = three_calls(ctx, txs)
    assert got.status == 0 and got.k == 32
    assert got.dah.hex() == golden["block408"]["data_hash"].lower()
    assert_same(got, want)
    assert len(got.commitments) == 1


@pytest.fixture(scope="module")
def edge():
    return B.edge_block()


def test_share_edges(ctx, edge):
    txs, segs = edge
    blobs = [s for s in segs if s.kind == B.SEG_BLOB]
    assert {s.off % 4 for s in blobs} == {0, 1, 2, 3}
    assert sorted(s.len for s in blobs) == sorted(B.EDGE_LENGTHS)
    blob_ns = {bytes(s.ns)[:B.NS] for s in blobs}
    assert any(s.kind == B.SEG_PAD and bytes(s.ns)[:B.NS] in blob_ns for s in segs)
    got = block_extend(ctx, txs, eds="full")
    want = three_calls(ctx, txs)
    assert got.status == 0 and got.k == 32
    assert_same(got, want)


KINDS = [b for b in B.layout_blocks() if b[0] != "block408"]


@pytest.mark.parametrize("name,txs,max_square_size,k", KINDS, ids=[b[0] for b in KINDS])
@pytest.mark.parametrize("greedy", [0, 1])
def test_layout_kinds(ctx, name, txs, max_square_size, k, greedy):
    import celestia_eds._lib as L
    got = block_extend(ctx, txs, max_square_size, greedy, eds="full")
    want = three_calls(ctx, txs, max_square_size, greedy)
    if k is not None:
        assert got.status == 0 and got.k == k
    if name == "dropping":
        if greedy:
            assert got.status == 0 and got.included == [1] * 4 + [2] * 8 + [0] * 22
            # the kept txs alone give the same roots through the three calls
            kept = three_calls(ctx, [t for t, s in zip(txs, got.included) if s], max_square_size, 0, False)
            assert kept.status == 0 and kept.dah == got.dah
            assert np.array_equal(kept.row_roots, got.row_roots[:2 * got.k])
        else:
            assert (got.status, got.error) == (L.ETOOBIG, "not enough space to append blob tx at index 12")
    if name == "misordered" and not greedy:
        assert (got.status, got.error) == (L.EINVAL, "normal transaction at index 2 can not be appended after blob tx")
    # the commitments cover every blob of every blob tx, kept or not
    assert_same(got, want)


def test_stale_scratch(ctx):
    """ctx scratch is reused: a smaller block after a larger one must not see its bytes."""
    import celestia_eds
    blocks = [random_block(1, 3, 4, max_blob=60000), random_block(3, 5, 0), []]
    fresh = []
    for txs in blocks:
        c = celestia_eds.Context(ctx.device)
        fresh.append(block_extend(c, txs, eds="full"))
        c.close()
    assert [f.k for f in fresh] == [32, 4, 1]
    c = celestia_eds.Context(ctx.device)
    for txs, f in zip(blocks, fresh):
        got = block_extend(c, txs, eds="full")
        assert got.status == 0 and got.dah == f.dah and np.array_equal(got.eds, f.eds)
        assert np.array_equal(got.row_roots, f.row_roots) and np.array_equal(got.col_roots, f.col_roots)
        assert_same(got, three_calls(ctx, txs))
    c.close()


def test_device_entry(ctx, edge):
    """cel_dev_square_build: tx bytes at an odd offset of a device buffer, the last blob ending
    on the buffer's last byte; exactly Q0 of the EDS buffer is written."""
    from hipmem import DeviceBuffer, synchronize
    rng = np.random.default_rng(5)
    # the edge block with one more blob tx whose only blob is the tx's (and the buffer's) end:
    # a BlobTx ending in its blob field (field order is free in protobuf)
    from square_inputs import blob_msg, field_bytes
    ns_id = bytes(18) + b"\xff" * 10  # sorts last: also the square's last blob
    data = rng.integers(0, 256, 1001, np.uint8).tobytes()
    last = field_bytes(1, rng.integers(0, 256, 190, np.uint8).tobytes()) + field_bytes(3, b"BLOB") + \
        field_bytes(2, blob_msg(ns_id, data))
    txs = edge[0] + [last]
    st, _, k, _, segs, compact = B.layout(txs)
    assert st == 0 and k == 32
    raw = b"".join(txs)
    blobs = [s for s in segs if s.kind == B.SEG_BLOB]
    assert max(s.off + s.len for s in blobs) == len(raw) and blobs[-1].off + blobs[-1].len == len(raw)
    shares = B.construct(txs)[4]
    odd = 3
    d_txs = DeviceBuffer(odd + len(raw))
    d_txs.upload(np.frombuffer(bytes(odd) + raw, np.uint8))
    d_eds = DeviceBuffer(4 * k * k * 512, fill=0xA5)
    arr = (B.Segment * len(segs))(*segs)
    ctx.check(ctx.lib.cel_dev_square_build(ctx.handle, ctypes.c_void_p(d_txs.ptr.value + odd), arr, len(segs),
                                           _p(compact), len(compact), k, d_eds.ptr, None))
    synchronize()
    eds = d_eds.download((2 * k, 2 * k, 512))
    assert np.array_equal(eds[:k, :k].reshape(k * k, 512), shares)
    assert (eds[:k, k:] == 0xA5).all() and (eds[k:] == 0xA5).all()
    # a layout that does not cover the square, or reads past the compact shares, is refused
    import celestia_eds._lib as L
    assert ctx.lib.cel_dev_square_build(ctx.handle, ctypes.c_void_p(d_txs.ptr.value + odd), arr, len(segs) - 1,
                                        _p(compact), len(compact), k, d_eds.ptr, None) == L.EINVAL
    assert ctx.lib.cel_dev_square_build(ctx.handle, ctypes.c_void_p(d_txs.ptr.value + odd), arr, len(segs),
                                        _p(compact), len(compact) - 1, k, d_eds.ptr, None) == L.EINVAL


def test_gf16_path(ctx, oracle):
    """k = 256: the GF(2^16) extension runs in place over the device-built Q0."""
    import celestia_eds._lib as L
    txs = B.mib_block()
    small = block_extend(ctx, txs, 128, cap=0)
    assert (small.status, small.error) == (L.ETOOBIG, "not enough space to append blob tx at index 7")
    got = block_extend(ctx, txs, 256)
    want = three_calls(ctx, txs, 256)
    assert got.status == 0 and got.k == 256 and len(got.commitments) == 9
    assert_same(got, want)
    _, _, _, dah = oracle.extend_and_commit(want.shares.reshape(256, 256, 512))
    assert got.dah == dah


def test_parity_only_and_no_eds(ctx, edge):
    txs = edge[0]
    full = block_extend(ctx, txs, eds="full", cap=0)
    par = block_extend(ctx, txs, eds="parity", cap=0)
    none = block_extend(ctx, txs, eds="none", cap=0)
    k = full.k
    for r in (par, none):
        assert r.status == 0 and r.dah == full.dah
        assert np.array_equal(r.row_roots, full.row_roots) and np.array_equal(r.col_roots, full.col_roots)
    assert (par.eds[:k, :k] == 0x5A).all(), "PARITY_ONLY wrote Q0"
    assert np.array_equal(par.eds[:k, k:], full.eds[:k, k:]) and np.array_equal(par.eds[k:], full.eds[k:])
    # an EDS buffer below 2k*2k*512 bytes is refused
    import celestia_eds._lib as L
    buf, lens, ntx, _ = B.pack(txs)
    kk, n = ctypes.c_uint32(), ctypes.c_uint32()
    small = np.zeros(4 * k * k * 512 - 1, np.uint8)
    out = np.zeros((256, 90), np.uint8)
    dah = np.zeros(32, np.uint8)
    assert ctx.lib.cel_block_extend(ctx.handle, buf, lens, ntx, 128, 64, 0, ctypes.byref(kk), None, _p(out), _p(out),
                                    _p(dah), _p(small), small.nbytes, None, None, 0, ctypes.byref(n), 0) == L.EINVAL


def test_commitment_errors(ctx):
    from celestia_eds import CelError, inclusion
    txs = B.version1_block()
    with pytest.raises(CelError) as e:
        inclusion.BlobTxCommitments(txs, ctx=ctx)
    got = block_extend(ctx, txs, cap=1)
    assert (got.status, got.error) == (e.value.status, str(e.value))
    assert got.error == "unsupported share version 1"
    # without commitments the square is still built, the version in the info byte
    got = block_extend(ctx, txs, eds="full", cap=0)
    want = three_calls(ctx, txs, commitments=False)
    assert got.status == 0 and got.n_commit == 1
    assert_same(got, want, commitments=False)
    info = got.eds[:got.k, :got.k].reshape(-1, 512)[:, B.NS]
    assert 3 in info and 2 in info  # version 1: sequence start, continuation


def test_python_mirror(ctx, golden):
    from celestia_eds import ExtendBlock, PrepareProposal, ProcessProposal, square
    txs = block408_txs()
    data_hash = bytes.fromhex(golden["block408"]["data_hash"])
    ok, commitments = ProcessProposal(ctx, txs, data_hash)
    assert ok and len(commitments) == 1
    flipped = bytes([data_hash[0] ^ 1]) + data_hash[1:]
    assert not ProcessProposal(ctx, txs, flipped)[0]
    assert ProcessProposal(ctx, B.misordered_block(), data_hash) == (False, [])
    eds, dah = ExtendBlock(ctx, txs)
    assert dah.Hash() == data_hash and eds.cells.shape == (64, 64, 512)
    assert np.array_equal(eds.cells[:32, :32].reshape(-1, 512), square.Construct(txs))
    drop = B.dropping_block()
    kept, k, root = PrepareProposal(ctx, drop, max_square_size=8)
    shares, want_kept = square.Build(drop, 8)
    assert kept == want_kept and k == 8
    assert root == three_calls(ctx, want_kept, 8, 0, False).dah
