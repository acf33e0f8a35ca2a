"""GPU: k_square_build (square_build.hip) and cel_block_extend at the blob lengths,
alignments, block sizes and square widths where their code branches:

  every blob length 1..1443 at every byte alignment through cel_dev_square_build, against a
    numpy expansion of the layout and against the sparse share splitter of commitment_ref.py
    (neither is the library's host builder);
  k = 1 (a 32-lane block) and k = 2 (128 lanes);
  k = 512 through cel_block_extend, against the three-call path and the hashlib commitment;
  txs in page-locked memory, which cel_block_extend uploads in place.
"""
import ctypes

import numpy as np
import pytest

import block_inputs as B
import commitment_ref as ref
from test_gpu_block import assert_same, block_extend, three_calls

pytestmark = pytest.mark.gpu


def square_build(ctx, raw, segs, k, odd=0):
    """cel_dev_square_build over a compact-free layout, the bytes `odd` bytes into a device
    buffer filled with 0xA5 (as is the EDS buffer). -> the EDS buffer [2k][2k][512]."""
    from hipmem import DeviceBuffer, hip, synchronize
    raw = np.frombuffer(raw, np.uint8)
    d_txs = DeviceBuffer(odd + len(raw) + 8, fill=0xA5)
    assert d_txs.ptr.value % 4 == 0
    assert hip().hipMemcpy(ctypes.c_void_p(d_txs.ptr.value + odd), raw.ctypes.data_as(ctypes.c_void_p), len(raw), 1) == 0
    d_eds = DeviceBuffer(4 * k * k * 512, fill=0xA5)
    arr = (B.Segment * len(segs))(*segs)
    ctx.check(ctx.lib.cel_dev_square_build(ctx.handle, ctypes.c_void_p(d_txs.ptr.value + odd), arr, len(segs), None, 0,
                                           k, d_eds.ptr, None))
    synchronize()
    eds = d_eds.download((2 * k, 2 * k, 512))
    d_txs.free()
    d_eds.free()
    return eds


def assert_square(eds, raw, segs, k):
    """Q0 is the layout's bytes (two independent restatements); nothing else is written."""
    q0 = eds[:k, :k].reshape(k * k, 512)
    want = B.expand(raw, k, segs, None)
    bad = [i for i in range(k * k) if not np.array_equal(q0[i], want[i])]
    assert not bad, f"{len(bad)} shares differ, first {bad[:12]}"
    for s in segs:
        if s.kind == B.SEG_BLOB:
            shares = ref.split_blob(bytes(s.ns)[:B.NS], raw[s.off:s.off + s.len], s.share_version)
            assert q0[s.start:s.start + s.count].tobytes() == b"".join(shares), (s.start, s.len)
    assert (eds[:k, k:] == 0xA5).all() and (eds[k:] == 0xA5).all()


# --- 1. every length at every alignment -----------------------------------------------------

@pytest.fixture(scope="module")
def every_length():
    raw, segs = B.blob_layout(range(1, 1444), 64, 1443, version1=(0, 477, 478, 700, 1442))
    blobs = [s for s in segs if s.kind == B.SEG_BLOB]
    assert len(blobs) == 1443 and sum(s.count for s in blobs) == 2892 and segs[-1].kind == B.SEG_PAD
    for s in blobs:  # over the four shifts every length starts at every address mod 4
        assert {(s.off + odd) % 4 for odd in range(4)} == {0, 1, 2, 3}
    return raw, segs


@pytest.mark.parametrize("odd", [0, 1, 2, 3])
def test_every_length(ctx, every_length, odd):
    raw, segs = every_length
    assert_square(square_build(ctx, raw, segs, 64, odd), raw, segs, 64)


# --- 2. small blocks ------------------------------------------------------------------------

@pytest.mark.parametrize("length", [1, 477, 478])
def test_k1_single_share_blob(ctx, length):
    """k = 1: one workgroup of 32 lanes."""
    raw, segs = B.blob_layout([length], 1, length)
    assert len(segs) == 1
    assert_square(square_build(ctx, raw, segs, 1, odd=length % 4), raw, segs, 1)


def test_k2_three_shares_and_padding(ctx):
    """k = 2: one workgroup of 128 lanes."""
    raw, segs = B.blob_layout([B.FIRST + B.CONT + 100], 2, 2)
    assert [(s.kind, s.count) for s in segs] == [(B.SEG_BLOB, 3), (B.SEG_PAD, 1)]
    assert_square(square_build(ctx, raw, segs, 2, odd=3), raw, segs, 2)


# --- 3. k = 512 -----------------------------------------------------------------------------

def test_k512_block(ctx):
    """One blob of 70000 shares (subtree width 512) and four 1 MiB blobs: k = 512."""
    import celestia_eds._lib as L
    from celestia_eds import inclusion
    from square_inputs import blob_tx
    rng = np.random.default_rng(512)
    big = rng.bytes(ref.blob_len_for_shares(70000) - 7)
    txs = []
    for i, data in enumerate([big] + [rng.bytes(1 << 20) for _ in range(4)]):
        ns_id = bytes(18) + rng.integers(0, 256, 10, np.uint8).tobytes()
        txs.append(blob_tx(rng.integers(0, 256, 200 + i, np.uint8).tobytes(), [(ns_id, data)]))
    assert inclusion.blob_subtree_sizes(len(big), 64)[:2] == (70000, 512)
    assert inclusion.blob_subtree_sizes(1 << 20, 64)[0] == 2176
    assert B.layout(txs, 512)[2] == 512
    small = block_extend(ctx, txs, 256, cap=0)
    assert small.status == L.ETOOBIG
    got = block_extend(ctx, txs, 512, eds="full")
    want = three_calls(ctx, txs, 512)
    assert got.status == 0 and got.k == 512 and len(got.commitments) == 5
    assert_same(got, want)
    ns, data, _ = ref.blob_tx_blobs(txs[0])[0]
    assert data == big and got.commitments[0] == (0, ref.create_commitment(ns, big))


# --- 4. page-locked txs ---------------------------------------------------------------------

def test_page_locked_txs(ctx):
    """The edge block from cel_host_alloc memory: uploaded from the caller's bytes, from the
    first blob byte on."""
    txs, _ = B.edge_block()
    raw = b"".join(txs)
    pageable = block_extend(ctx, txs, eds="full")
    p = ctx.lib.cel_host_alloc(len(raw))
    assert p, "cel_host_alloc failed"
    try:
        ctypes.memmove(p, raw, len(raw))
        got = block_extend(ctx, txs, eds="full", txs_at=ctypes.c_void_p(p))
    finally:
        ctx.lib.cel_host_free(p)
    assert got.status == 0 and got.k == 32 and len(got.commitments) == len(B.EDGE_LENGTHS)
    assert (got.k, got.included, got.dah, got.commitments) == (pageable.k, pageable.included, pageable.dah,
                                                               pageable.commitments)
    assert np.array_equal(got.row_roots, pageable.row_roots) and np.array_equal(got.col_roots, pageable.col_roots)
    assert np.array_equal(got.eds, pageable.eds)
    assert_same(got, three_calls(ctx, txs))
