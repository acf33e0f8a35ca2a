"""GPU parity of the generic hashers at the lengths and counts where a byte-wise SHA-256 and
an odd-node-carrying tree go wrong: cel_nmt_root over leaves of any length (the SHA-256
padding boundaries, where 1 + len = 55, 56, 63, 0 mod 64) and any count (non-powers of two,
more than one workgroup), cel_merkle_hash_slices over slices of every length 0..200 and of
counts past one stride of its one-workgroup tree."""
import ctypes

import numpy as np
import pytest

from merkle_ref import hash_from_byte_slices

pytestmark = pytest.mark.gpu

NS = 29
PARITY_NS = b"\xff" * NS
NMT_COUNTS = [0, 1, 2, 3, 5, 13, 255, 256, 257, 600]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sorted_leaves(rng, n, leaf_len):
    """n namespaced leaves in push order: runs of equal namespaces, and for n >= 3 a closing
    run of the parity namespace (the ignore-max-namespace rule then decides the range of
    every node whose right child starts in that run)."""
    tail = max(1, n // 4) if n >= 3 else 0
    m = n - tail
    pool = rng.integers(0, 256, (max(1, m // 3), NS), dtype=np.uint8)
    pool[:, 0] = np.minimum(pool[:, 0], 0xFE)  # below the parity namespace
    names = sorted(pool[i].tobytes() for i in rng.integers(0, len(pool), m))
    names += [PARITY_NS] * tail
    return [ns + rng.integers(0, 256, leaf_len - NS, dtype=np.uint8).tobytes() for ns in names]


@pytest.mark.parametrize("leaf_len", [29, 54, 55, 56, 62, 63, 64, 118, 119, 120, 541])
def test_nmt_root_leaf_lengths_and_counts(ctx, oracle, leaf_len):
    """cel_nmt_root = the oracle's NMT (pinned in test_oracle.py) for every count in
    NMT_COUNTS at this leaf length: leaf message 0x00 || leaf of 1 + leaf_len bytes."""
    from celestia_eds import _lib
    for n in NMT_COUNTS:
        rng = np.random.default_rng(100000 + 1000 * leaf_len + n)
        leaves = _sorted_leaves(rng, n, leaf_len)
        if n >= 3:
            assert leaves[-1][:NS] == PARITY_NS and leaves[0][:NS] != PARITY_NS
        rc, want = oracle.nmt_root(leaves)
        assert rc == 0
        buf = np.frombuffer(b"".join(leaves), np.uint8).copy() if n else np.zeros(1, np.uint8)
        out = np.zeros(_lib.NMT_NODE_SIZE, np.uint8)
        st = ctx.lib.cel_nmt_root(ctx.handle, _p(buf), n, leaf_len, _p(out), _lib.FLAG_ORDER_CHECK)
        assert st == _lib.OK, (leaf_len, n, st)
        assert out.tobytes() == want, (leaf_len, n)


def _hash_slices(ctx, slices):
    from celestia_eds import _lib
    offs = np.zeros(len(slices) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in slices], dtype=np.uint64)
    data = np.frombuffer(b"".join(slices) or b"\0", np.uint8).copy()
    out = np.zeros(32, np.uint8)
    st = ctx.lib.cel_merkle_hash_slices(ctx.handle, _p(data), _p(offs), len(slices), _p(out))
    assert st == _lib.OK, st
    return out.tobytes()


def test_merkle_hash_slices_every_length(ctx):
    """201 slices of lengths 0, 1, ..., 200: every SHA-256 padding residue of the leaf
    message 0x00 || slice (1 to 4 blocks) and a count that is no power of two."""
    rng = np.random.default_rng(201)
    slices = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(201)]
    assert _hash_slices(ctx, slices) == hash_from_byte_slices(slices)


@pytest.mark.parametrize("count", [1, 2, 3, 255, 256, 257, 513, 1025])
def test_merkle_hash_slices_counts(ctx, count):
    """32-byte slices at counts around the 256-thread workgroup of the tree kernel: 513 and
    1025 make a level's pair count exceed one stride, 255 / 257 / 513 / 1025 carry an odd
    node up at one or more levels."""
    rng = np.random.default_rng(32000 + count)
    slices = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(count)]
    assert _hash_slices(ctx, slices) == hash_from_byte_slices(slices)
