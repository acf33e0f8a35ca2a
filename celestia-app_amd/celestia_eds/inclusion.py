"""pkg/inclusion mirror: blob share commitments read from the EDS.

  calculate_commitment_paths  paths.go:16-47 (host: cel_commitment_paths)
  gen_subtree_root_path       paths.go:49-63
  GetCommitment               get_commit.go:12-30 over device-built row trees
                              (cel_get_commitment; the reference walks the
                              EDSSubTreeRootCacher of nmt_caching.go filled while rsmt2d
                              computed the row roots)
  CreateCommitment(s)         go-square inclusion.CreateCommitment from blob bytes, batched
                              on the device (cel_create_commitments), as ValidateBlobTx
                              needs it before the square exists
  BlobTxCommitments           the same for every blob of a block's BlobTxs
                              (cel_blob_tx_commitments)
  blob_subtree_sizes          MerkleMountainRangeSizes / SubTreeWidth (host)
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import CelError

WALK_LEFT, WALK_RIGHT = False, True
DEFAULT_SUBTREE_ROOT_THRESHOLD = 64


def gen_subtree_root_path(depth, pos):
    """WalkInstructions from a subtree root at (depth, pos) down: the bits of pos, most
    significant first (False = left, True = right)."""
    return [bool(pos & (1 << i)) for i in range(depth - 1, -1, -1)]


def _paths(square_size, start, blob_len, threshold):
    l = _lib.load()
    n = ctypes.c_uint32()
    st = l.cel_commitment_paths(square_size, start, blob_len, threshold, None, None, None, 0, ctypes.byref(n))
    if st != _lib.OK:
        raise CelError(st, "cannot get commitment for blob that doesn't fit in square" if st == _lib.ETOOBIG
                       else "invalid commitment path arguments")
    rows, depths, pos = (np.zeros(max(n.value, 1), np.uint32) for _ in range(3))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    l.cel_commitment_paths(square_size, start, blob_len, threshold, P(rows), P(depths), P(pos), n.value,
                           ctypes.byref(n))
    return [(int(rows[i]), int(depths[i]), int(pos[i])) for i in range(n.value)]


def calculate_subtree_root_coordinates(max_depth, min_depth, start, end):
    """paths.go:95-173 -> [(depth, position)]"""
    l = _lib.load()
    n = ctypes.c_uint32()
    cap = 64
    d, p = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = l.cel_subtree_root_coordinates(max_depth, min_depth, start, end, P(d), P(p), cap, ctypes.byref(n))
    if st != _lib.OK:
        raise CelError(st, "invalid subtree root coordinate arguments")
    return [(int(d[i]), int(p[i])) for i in range(min(n.value, cap))]


def calculate_commitment_paths(square_size, start, blob_len, threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD):
    """-> [(row, [WalkInstruction...])] inside each row's ODS half (the reference walk
    from the row root prepends one WalkLeft)."""
    return [(r, gen_subtree_root_path(d, p)) for r, d, p in _paths(square_size, start, blob_len, threshold)]


def blob_subtree_sizes(blob_len, threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD):
    """(shares, width, sizes): SparseSharesNeeded(blob_len), SubTreeWidth(shares, threshold)
    and MerkleMountainRangeSizes(shares, width) (host: cel_blob_subtree_sizes)."""
    l = _lib.load()
    n, w, cnt = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    st = l.cel_blob_subtree_sizes(blob_len, threshold, ctypes.byref(n), ctypes.byref(w), None, 0, ctypes.byref(cnt))
    if st != _lib.OK:
        raise CelError(st, "blob too large for the device path" if st == _lib.ETOOBIG
                       else "invalid blob length or subtree root threshold")
    sizes = np.zeros(max(cnt.value, 1), np.uint32)
    l.cel_blob_subtree_sizes(blob_len, threshold, None, None, sizes.ctypes.data_as(ctypes.c_void_p), cnt.value,
                             ctypes.byref(cnt))
    return n.value, w.value, [int(x) for x in sizes[:cnt.value]]


def merkle_mountain_range_sizes(n, w):
    """inclusion.MerkleMountainRangeSizes: n leaves as trees of w leaves, then the
    remainder in descending powers of two."""
    out, left = [], int(n)
    while left:
        t = w if left >= w else 1 << (left.bit_length() - 1)
        out.append(t)
        left -= t
    return out


def _pack_blobs(blobs):
    """[(ns29, data) or (ns29, data, share_version)] -> (data, offsets, namespaces, versions)"""
    blobs = [tuple(b) for b in blobs]
    for b in blobs:
        if len(b[0]) != _lib.NAMESPACE_SIZE:
            raise CelError(_lib.EINVAL, f"namespace must be {_lib.NAMESPACE_SIZE} bytes (version || id)")
    data = np.frombuffer(b"".join(bytes(b[1]) for b in blobs), np.uint8)
    offsets = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum([len(b[1]) for b in blobs], out=offsets[1:])
    ns = np.frombuffer(b"".join(bytes(b[0]) for b in blobs), np.uint8)
    ver = np.array([b[2] if len(b) > 2 else 0 for b in blobs], np.uint8)
    return data, offsets, ns, ver


def CreateCommitments(blobs, threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD, ctx=None):
    """inclusion.CreateCommitments on the device (cel_create_commitments): blobs is a list
    of (namespace (29 B: version || id), data[, share_version]); -> [commitment (32 B)]."""
    ctx = ctx or _lib.default_context()
    data, offsets, ns, ver = _pack_blobs(blobs)
    out = np.zeros((max(len(blobs), 1), 32), np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # an empty batch still reaches the library: it owns the argument errors
    ctx.check(ctx.lib.cel_create_commitments(ctx.handle, P(data) if len(data) else P(out), P(offsets), len(blobs),
                                             P(ns) if len(ns) else P(out), P(ver) if len(ver) else None, threshold,
                                             P(out)))
    return [out[i].tobytes() for i in range(len(blobs))]


def CreateCommitment(ns, data, share_version=0, threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD, ctx=None):
    """inclusion.CreateCommitment of one blob -> 32 bytes."""
    return CreateCommitments([(ns, data, share_version)], threshold, ctx)[0]


def BlobTxCommitments(txs, threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD, ctx=None):
    """The share commitment of every blob of every BlobTx among txs, one device batch
    (cel_blob_tx_commitments) -> [(tx_index, commitment)] in tx, then blob, order: what
    ProcessProposal compares with the PFBs' signed share_commitments."""
    ctx = ctx or _lib.default_context()
    txs = [bytes(t) for t in txs]
    lens = (ctypes.c_uint32 * max(len(txs), 1))(*[len(t) for t in txs])
    raw = b"".join(txs)
    buf = ctypes.create_string_buffer(raw, max(len(raw), 1))
    n = ctypes.c_uint32()
    ctx.check(ctx.lib.cel_blob_tx_commitments(ctx.handle, buf, lens, len(txs), threshold, None, None, 0,
                                              ctypes.byref(n)))
    if n.value == 0:
        return []
    out = np.zeros((n.value, 32), np.uint8)
    idx = np.zeros(n.value, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ctx.check(ctx.lib.cel_blob_tx_commitments(ctx.handle, buf, lens, len(txs), threshold, P(out), P(idx), n.value,
                                              ctypes.byref(n)))
    return [(int(idx[i]), out[i].tobytes()) for i in range(n.value)]


def GetCommitment(eds, start, blob_share_len, subtree_root_threshold=DEFAULT_SUBTREE_ROOT_THRESHOLD, ctx=None):
    """The blob share commitment (32 B) of the blob of blob_share_len shares at share
    index `start` (first aligned index >= start) of the EDS's original square."""
    ctx = ctx or eds.ctx
    cells = np.ascontiguousarray(eds.cells)
    k = cells.shape[0] // 2
    out = np.zeros(32, np.uint8)
    ctx.check(ctx.lib.cel_get_commitment(ctx.handle, cells.ctypes.data_as(ctypes.c_void_p), k, _lib.SHARE_SIZE,
                                         start, blob_share_len, subtree_root_threshold,
                                         out.ctypes.data_as(ctypes.c_void_p)))
    return out.tobytes()
