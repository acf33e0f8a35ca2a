"""CPU: celestia_eds.blob.parse_sparse_shares, the host statement of go-square v1.1.0
parseSparseShares and the checker of the device path (tests/test_gpu_blobs.py), and
cel_namespace_ods_ranges. The parser is pinned from two sides: it is the inverse of the square
constructor on every block of the layout tests (the blob segments of cel_square_layout, byte for
byte), and mainnet block 408's original data square gives the blobs its txs carry. Hand-made
shares cover what no constructed square holds."""
import numpy as np
import pytest

import block_inputs as B
import blob_cases as C
import commitment_ref
from celestia_eds import _lib, blob


def _region(segs, shares):
    """The shares behind the compact ones: padding, blobs, tail padding."""
    at = max([s.start + s.count for s in segs if s.kind == B.SEG_COMPACT], default=0)
    return at, shares[at:]


def _check_inverse(txs, max_square_size=128):
    st, _, k, _, shares = B.construct(txs, max_square_size)
    assert st == 0
    st, _, k2, _, segs, _ = B.layout(txs, max_square_size)
    assert st == 0 and k2 == k
    raw = b"".join(bytes(t) for t in txs)
    at, region = _region(segs, shares)
    got = blob.parse_sparse_shares(region)
    want = [s for s in segs if s.kind == B.SEG_BLOB]
    assert len(got) == len(want)
    for g, s in zip(got, want):
        assert g.namespace == bytes(s.ns)[:B.NS] and g.share_version == s.share_version == 0
        assert g.data == raw[s.off:s.off + s.len]
        assert g.index + at == s.start and g.shares == s.count
    return got


@pytest.mark.parametrize("name", [b[0] for b in B.layout_blocks() if b[3] is not None])
def test_inverse_of_construct(name):
    _, txs, mss, k = next(b for b in B.layout_blocks() if b[0] == name)
    _check_inverse(txs, mss)


def test_inverse_of_construct_edge_block():
    txs, _ = B.edge_block()
    got = _check_inverse(txs)
    assert sorted(len(g.data) for g in got) == sorted(B.EDGE_LENGTHS)


def test_version1_block_is_a_version_error():
    txs = B.version1_block()
    st, _, k, _, shares = B.construct(txs)
    assert st == 0
    st, _, _, _, segs, _ = B.layout(txs)
    assert [s.share_version for s in segs if s.kind == B.SEG_BLOB] == [1]
    with pytest.raises(blob.BlobParseError) as e:
        blob.parse_sparse_shares(_region(segs, shares)[1])
    assert e.value.kind == blob.EVERSION


def test_block408_ods_gives_the_blobs_of_its_txs(block408_ods):
    txs = B.block408_txs()
    st, _, k, _, segs, _ = B.layout(txs)
    assert st == 0 and k == 32
    at, region = _region(segs, block408_ods.reshape(-1, 512))
    got = blob.parse_sparse_shares(region)
    carried = [b for tx in txs if blob_is_tx(tx) for b in commitment_ref.blob_tx_blobs(tx)]
    assert len(carried) > 0
    # the square orders blobs by namespace; the txs carry them in tx order
    assert sorted((g.namespace, g.data) for g in got) == sorted((ns, data) for ns, data, _ in carried)
    assert [g.namespace for g in got] == sorted(g.namespace for g in got)


def blob_is_tx(tx):
    from celestia_eds import square
    return square.is_blob_tx(tx)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_hand_made_shares(case):
    shares = case.shares()
    if case.error:
        with pytest.raises(blob.BlobParseError) as e:
            blob.parse_sparse_shares(shares)
        assert e.value.kind == case.error
        return
    got = blob.parse_sparse_shares(shares)
    assert [(g.namespace, g.data, g.index, g.shares) for g in got] == case.want()


def test_parse_takes_lists_of_byte_strings():
    raw, segs = B.blob_layout([500, 3], 2, 5)
    shares = B.expand(raw, 2, segs, None)
    a = blob.parse_sparse_shares(shares)
    b = blob.parse_sparse_shares([s.tobytes() for s in shares])
    assert a == b and [len(x.data) for x in a] == [500, 3]
    assert blob.parse_sparse_shares([]) == []


def _ranges(k, n, entries):
    plan = dict(ns_idx=np.array([e[0] for e in entries], np.uint32), rows=np.array([e[1] for e in entries], np.uint32),
                starts=np.array([e[2] for e in entries], np.int32), ends=np.array([e[3] for e in entries], np.int32),
                kinds=np.array([e[4] for e in entries], np.uint8))
    return blob.ods_ranges(k, n, plan)


def test_namespace_ods_ranges():
    inc, absent = _lib.NS_INCLUSION, _lib.NS_ABSENCE
    # namespace 0: rows 1 .. 3 of k = 8, contiguous; namespace 1: absent; namespace 2: one row; 3: no entry
    entries = [(0, 1, 5, 8, inc), (0, 2, 0, 8, inc), (0, 3, 0, 2, inc), (1, 3, 2, 3, absent), (2, 3, 2, 7, inc)]
    assert _ranges(8, 4, entries) == [(13, 26), (0, 0), (26, 31), (0, 0)]
    assert _ranges(8, 2, []) == [(0, 0), (0, 0)]
    # duplicate namespaces are separate queries
    assert _ranges(8, 2, [(0, 0, 0, 3, inc), (1, 0, 0, 3, inc)]) == [(0, 3), (0, 3)]
    for bad in ([(0, 1, 5, 8, inc), (0, 3, 0, 2, inc)],      # a row is missing
                [(0, 1, 5, 7, inc), (0, 2, 0, 8, inc)],      # the first row stops short of its end
                [(0, 1, 5, 8, inc), (0, 2, 1, 8, inc)],      # the second row starts late
                [(0, 2, 0, 8, inc), (0, 1, 5, 8, inc)],      # out of order
                [(0, 1, 5, 9, inc)],                         # reaches column k
                [(0, 8, 0, 1, inc)],                         # a row of the parity half
                [(2, 1, 0, 1, inc)]):                        # an index beyond the namespaces
        with pytest.raises(_lib.CelError) as e:
            _ranges(8, 2, bad)
        assert e.value.status == _lib.EINVAL


def test_reserved_namespaces_are_rejected():
    for ns in (bytes(28) + b"\x01", bytes(28) + b"\x04", bytes(28) + b"\xff", b"\xff" * 28 + b"\xfe", b"\xff" * 29,
               bytes(28)):
        with pytest.raises(_lib.CelError) as e:
            blob.check_blob_namespaces([ns])
        assert e.value.status == _lib.EINVAL
    assert blob.check_blob_namespaces([bytes(19) + b"\x01" * 10]) == [bytes(19) + b"\x01" * 10]
