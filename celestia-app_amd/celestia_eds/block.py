"""The block path from txs, mirrored over the C ABI's cel_block_extend: the host lays the
data square out, the tx bytes cross PCIe once, the device writes the square, extends it and
hashes the roots, and the blob share commitments come from the same upload.

  ExtendBlock(ctx, txs)                    app/extend_block.go:16-25: square.Construct +
      da.ExtendShares + NewDataAvailabilityHeader -> (eds, dah)
  ProcessProposal(ctx, txs, data_hash)     app/process_proposal.go:101-156: the blob txs'
      share commitments (ValidateBlobTx recomputes them, :107), square.Construct (:122) and
      the data root compared with the header's -> (accept, commitments)
  PrepareProposal(ctx, txs)                app/prepare_proposal.go:48-92: square.Build (txs
      that do not fit are dropped) and the data root -> (kept txs, k, data root)

The defaults are appconsts SquareSizeUpperBound = 128 and SubtreeRootThreshold = 64.
"""
import ctypes

import numpy as np

from . import _lib
from .da import DataAvailabilityHeader
from .rsmt2d import ExtendedDataSquare
from .square import SQUARE_SIZE_UPPER_BOUND, SUBTREE_ROOT_THRESHOLD


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class _Block:
    """One cel_block_extend call's outputs."""


def _pack(txs):
    txs = [bytes(t) for t in txs]
    lens = (ctypes.c_uint32 * max(len(txs), 1))(*[len(t) for t in txs])
    blob = b"".join(txs)
    return txs, lens, ctypes.create_string_buffer(blob, max(len(blob), 1))


def block_extend(ctx, txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD,
                 greedy=False, want_eds=False, want_commitments=False, flags=_lib.FLAG_ORDER_CHECK):
    """cel_block_extend -> an object with k, included, row_roots, col_roots (uint8 [2k][90]),
    dah (bytes), eds (uint8 [2k][2k][512] or None; with FLAG_PARITY_ONLY its Q0 stays zero) and
    commitments ([(tx index, 32 bytes)] for every blob of every blob tx, or None)."""
    ctx = ctx or _lib.default_context()
    l = ctx.lib
    txs, lens, buf = _pack(txs)
    ntx, greedy = len(txs), 1 if greedy else 0
    k = ctypes.c_uint32()
    included = (ctypes.c_uint8 * max(ntx, 1))()
    eds, eds_cap = None, 0
    if want_eds:  # the EDS buffer needs k: the layout alone (host only) reports it
        nseg, ncomp = ctypes.c_uint32(), ctypes.c_uint32()
        st = l.cel_square_layout(buf, lens, ntx, max_square_size, subtree_root_threshold, greedy, ctypes.byref(k),
                                 None, None, 0, ctypes.byref(nseg), None, 0, ctypes.byref(ncomp))
        if st != _lib.OK:
            raise _lib.CelError(st, l.cel_square_last_error().decode())
        eds = np.zeros((2 * k.value, 2 * k.value, _lib.SHARE_SIZE), np.uint8)
        eds_cap = eds.nbytes
    cap, n = 0, ctypes.c_uint32()
    if want_commitments:  # cap = 0 only counts the blobs (no device work)
        ctx.check(l.cel_blob_tx_commitments(ctx.handle, buf, lens, ntx, subtree_root_threshold, None, None, 0,
                                            ctypes.byref(n)))
        cap = n.value
    commitments = np.zeros((max(cap, 1), 32), np.uint8)
    tx_index = np.zeros(max(cap, 1), np.uint32)
    rr = np.zeros((2 * max_square_size, _lib.NMT_NODE_SIZE), np.uint8)
    cr = np.zeros((2 * max_square_size, _lib.NMT_NODE_SIZE), np.uint8)
    dah = np.zeros(32, np.uint8)
    ctx.check(l.cel_block_extend(ctx.handle, buf, lens, ntx, max_square_size, subtree_root_threshold, greedy,
                                 ctypes.byref(k), included, _p(rr), _p(cr), _p(dah),
                                 _p(eds) if want_eds else None, eds_cap, _p(commitments) if cap else None,
                                 _p(tx_index) if cap else None, cap, ctypes.byref(n), flags))
    out = _Block()
    out.k = k.value
    out.included = [int(included[i]) for i in range(ntx)]
    out.row_roots, out.col_roots = rr[:2 * out.k].copy(), cr[:2 * out.k].copy()
    out.dah = dah.tobytes()
    out.eds = eds
    out.commitments = [(int(tx_index[i]), commitments[i].tobytes()) for i in range(cap)] if want_commitments else None
    out.txs = txs
    return out


def ExtendBlock(ctx, txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """app.ExtendBlock: -> (*rsmt2d.ExtendedDataSquare, DataAvailabilityHeader); raises
    CelError with go-square's message if the txs do not construct a square."""
    b = block_extend(ctx, txs, max_square_size, subtree_root_threshold, want_eds=True)
    eds = ExtendedDataSquare(b.eds, b.row_roots, b.col_roots, ctx=ctx)
    eds._dah = b.dah
    dah = DataAvailabilityHeader([r.tobytes() for r in b.row_roots], [c.tobytes() for c in b.col_roots])
    dah.hash = b.dah
    return eds, dah


def ProcessProposal(ctx, txs, data_hash, max_square_size=SQUARE_SIZE_UPPER_BOUND,
                    subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """-> (accept, commitments). Accept iff every blob's commitment can be computed, the txs
    construct a square in their order, and its data root equals data_hash; commitments are
    [(tx index, 32 bytes)] for the caller to compare with the signed ones ([] on reject by
    construction). Device failures still raise."""
    try:
        b = block_extend(ctx, txs, max_square_size, subtree_root_threshold, want_commitments=True)
    except _lib.CelError as e:
        if e.status in (_lib.EINVAL, _lib.ETOOBIG, _lib.EORDER):
            return False, []
        raise
    return b.dah == bytes(data_hash), b.commitments


def PrepareProposal(ctx, txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """-> (kept txs: normal txs first, then blob txs, as square.Build orders them; k; data
    root)."""
    b = block_extend(ctx, txs, max_square_size, subtree_root_threshold, greedy=True)
    kept = [t for t, s in zip(b.txs, b.included) if s == 1] + [t for t, s in zip(b.txs, b.included) if s == 2]
    return kept, b.k, b.dah
