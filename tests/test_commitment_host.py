"""CPU: the host side of the blob share commitments (cel_blob_subtree_sizes, argument
checks) against the hashlib restatement in commitment_ref.py, and that restatement against
the one commitment the reference data holds."""
import ctypes

import pytest

import commitment_ref as ref
from square_inputs import block408_txs

SHARE_COUNTS = [63, 64, 65, 267, 352, 1031, 16384, 70000]
LENGTHS = [1, 478, 479, 960, 961] + [ref.blob_len_for_shares(n) for n in SHARE_COUNTS]
THRESHOLDS = [1, 8, 64, 4096]


def test_subtree_sizes_match_restatement():
    from celestia_eds import inclusion
    for length in LENGTHS + [ref.blob_len_for_shares(n) - ref.CONT + 1 for n in SHARE_COUNTS]:
        for t in THRESHOLDS:
            n = ref.sparse_shares_needed(length)
            w = ref.subtree_width(n, t)
            assert inclusion.blob_subtree_sizes(length, t) == (n, w, ref.mountain_range(n, w)), (length, t)
            assert inclusion.merkle_mountain_range_sizes(n, w) == ref.mountain_range(n, w)


@pytest.mark.parametrize("n,w,trees,tail", [(64, 1, 64, []), (65, 2, 32, [1]), (267, 8, 33, [2, 1]),
                                            (1031, 32, 32, [4, 2, 1]), (70000, 512, 136, [256, 64, 32, 16])])
def test_subtree_sizes_known_values(n, w, trees, tail):
    from celestia_eds import inclusion
    assert inclusion.blob_subtree_sizes(ref.blob_len_for_shares(n), 64) == (n, w, [w] * trees + tail)


def test_subtree_sizes_argument_errors():
    import celestia_eds._lib as L
    lib = L.load()
    n = ctypes.c_uint32()
    assert lib.cel_blob_subtree_sizes(0, 64, None, None, None, 0, ctypes.byref(n)) == L.EINVAL
    assert lib.cel_blob_subtree_sizes(100, 0, None, None, None, 0, ctypes.byref(n)) == L.EINVAL
    assert lib.cel_blob_subtree_sizes(100, 64, None, None, None, 0, None) == L.EINVAL
    assert lib.cel_blob_subtree_sizes(ref.blob_len_for_shares(1 << 20), 64, None, None, None, 0,
                                      ctypes.byref(n)) == L.OK
    assert lib.cel_blob_subtree_sizes(ref.blob_len_for_shares(1 << 20) + 1, 64, None, None, None, 0,
                                      ctypes.byref(n)) == L.ETOOBIG


def test_commitment_entry_points_validate_without_a_device():
    import celestia_eds._lib as L
    lib = L.load()
    out = (ctypes.c_uint8 * 32)()
    off = (ctypes.c_uint64 * 2)(0, 10)
    data = (ctypes.c_uint8 * 10)()
    ns = (ctypes.c_uint8 * 29)()
    n = ctypes.c_uint32()
    assert lib.cel_create_commitments(None, data, off, 1, ns, None, 64, out) == L.EINVAL
    assert lib.cel_dev_create_commitments(None, data, off, 1, ns, None, 64, out, out, None) == L.EINVAL
    assert lib.cel_blob_tx_commitments(None, data, None, 0, 64, None, None, 0, ctypes.byref(n)) == L.EINVAL
    assert lib.cel_dev_commitments_workspace_size(1000, 10) > 1000 * 96


def test_restatement_reproduces_block408_signed_commitment():
    """The only commitment the reference data holds: block 408's one blob tx carries the
    share commitment its sender signed in the MsgPayForBlobs. The restatement reproduces it
    from the blob bytes (1 blob, 352 shares, width 8, 44 roots). It pins the SHA-256 paths
    only (share splitting, NMT, RFC-6962); no GF arithmetic is involved."""
    blob_txs = []
    for tx in block408_txs():
        try:
            blobs, signed = ref.blob_tx_parts(tx)
        except (StopIteration, IndexError, ValueError):
            continue
        if blobs and signed:
            blob_txs.append((blobs, signed))
    assert len(blob_txs) == 1
    blobs, signed = blob_txs[0]
    assert len(blobs) == 1 and len(signed) == 1 and len(signed[0]) == 32
    ns, data, ver = blobs[0]
    n = ref.sparse_shares_needed(len(data))
    assert (n, ref.subtree_width(n)) == (352, 8) and len(ref.mountain_range(n, 8)) == 44
    assert ref.create_commitment(ns, data, ver) == signed[0]
