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

  ExtendBlocks(ctx, blocks) / ProcessProposals(ctx, blocks, data_hashes)   the first two for a
      range of blocks in one call (cel_block_extend_batch): a DataAvailabilityHeader, or
      (accept, commitments), per block

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


def block_extend_batch(ctx, blocks, max_square_size=SQUARE_SIZE_UPPER_BOUND,
                       subtree_root_threshold=SUBTREE_ROOT_THRESHOLD, greedy=False, want_commitments=False,
                       flags=_lib.FLAG_ORDER_CHECK, host_threads=1, max_eds_bytes=0):
    """cel_block_extend_batch over blocks (a list of tx lists) -> a list of the objects
    block_extend returns (eds None), one per block. A block that failed carries its .status and
    .error (k 0, no roots, a zero dah, commitments []); the others carry status 0 and error "".
    Argument and device errors raise."""
    ctx = ctx or _lib.default_context()
    l = ctx.lib
    blocks = [[bytes(t) for t in b] for b in blocks]
    n = len(blocks)
    flat = [t for b in blocks for t in b]
    lens = np.array([len(t) for t in flat] + [0], np.uint32)
    nt = np.array([len(b) for b in blocks] + [0], np.uint32)
    raw = b"".join(flat)
    buf = ctypes.create_string_buffer(raw, max(len(raw), 1))
    k = np.zeros(max(n, 1), np.uint32)
    status = np.zeros(max(n, 1), np.int32)
    included = np.zeros(max(len(flat), 1), np.uint8)
    cap = n * 2 * max_square_size
    rr = np.zeros((max(cap, 1), _lib.NMT_NODE_SIZE), np.uint8)
    cr = np.zeros((max(cap, 1), _lib.NMT_NODE_SIZE), np.uint8)
    root_off = np.zeros(n + 1, np.uint32)
    dah = np.zeros((max(n, 1), 32), np.uint8)
    ccap, ncom = 0, ctypes.c_uint32()
    if want_commitments:  # cap = 0 only counts the blobs (no device work)
        ctx.check(l.cel_blob_tx_commitments(ctx.handle, buf, _p(lens), len(flat), subtree_root_threshold, None, None, 0,
                                            ctypes.byref(ncom)))
        ccap = ncom.value
    com = np.zeros((max(ccap, 1), 32), np.uint8)
    cblock = np.zeros(max(ccap, 1), np.uint32)
    ctx_index = np.zeros(max(ccap, 1), np.uint32)
    st = l.cel_block_extend_batch(ctx.handle, buf, _p(lens), _p(nt), n, max_square_size, subtree_root_threshold,
                                  1 if greedy else 0, host_threads, max_eds_bytes, _p(k), _p(status), _p(included),
                                  _p(rr), _p(cr), _p(root_off), cap, _p(dah), _p(com) if ccap else None,
                                  _p(cblock) if ccap else None, _p(ctx_index) if ccap else None, ccap,
                                  ctypes.byref(ncom), None, flags)
    # the first failed block's status is the call's too: anything else (an argument or device
    # error, after which the per-block outputs may not be written) raises
    failed = [int(s) for s in status[:n] if s != 0]
    if st != _lib.OK and (not failed or st != failed[0] or not l.cel_last_error(ctx.handle).startswith(b"block ")):
        ctx.check(st)
    out, t0 = [], 0
    for i, txs in enumerate(blocks):
        b = _Block()
        b.status = int(status[i])
        b.error = l.cel_block_batch_error(ctx.handle, i).decode() if b.status else ""
        b.k = int(k[i])
        b.included = [int(x) for x in included[t0:t0 + len(txs)]]
        t0 += len(txs)
        r0 = int(root_off[i])
        b.row_roots, b.col_roots = rr[r0:r0 + 2 * b.k].copy(), cr[r0:r0 + 2 * b.k].copy()
        b.dah = dah[i].tobytes()
        b.eds = None
        b.commitments = [] if want_commitments else None
        b.txs = txs
        out.append(b)
    if want_commitments:
        for j in range(ncom.value):
            out[int(cblock[j])].commitments.append((int(ctx_index[j]), com[j].tobytes()))
    return out


def ExtendBlocks(ctx, blocks, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD,
                 host_threads=1):
    """app.ExtendBlock over a range of blocks in one call -> a DataAvailabilityHeader per block
    (no EDS comes back); raises CelError with go-square's message, prefixed "block <i>: ", for
    the first block whose txs do not construct a square."""
    out = []
    for i, b in enumerate(block_extend_batch(ctx, blocks, max_square_size, subtree_root_threshold,
                                             host_threads=host_threads)):
        if b.status:
            raise _lib.CelError(b.status, f"block {i}: {b.error}")
        dah = DataAvailabilityHeader([r.tobytes() for r in b.row_roots], [c.tobytes() for c in b.col_roots])
        dah.hash = b.dah
        out.append(dah)
    return out


def ProcessProposals(ctx, blocks, data_hashes, max_square_size=SQUARE_SIZE_UPPER_BOUND,
                     subtree_root_threshold=SUBTREE_ROOT_THRESHOLD, host_threads=1):
    """ProcessProposal over a range of blocks in one call -> [(accept, commitments)] per block,
    by ProcessProposal's rule: a block that does not construct or whose commitments cannot be
    computed is (False, []); any other block status raises."""
    out = []
    for i, (b, want) in enumerate(zip(block_extend_batch(ctx, blocks, max_square_size, subtree_root_threshold,
                                                         want_commitments=True, host_threads=host_threads),
                                      data_hashes)):
        if b.status in (_lib.EINVAL, _lib.ETOOBIG, _lib.EORDER):
            out.append((False, []))
        elif b.status:
            raise _lib.CelError(b.status, f"block {i}: {b.error}")
        else:
            out.append((b.dah == bytes(want), b.commitments))
    return out


def PrepareProposal(ctx, txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """-> (kept txs: normal txs first, then blob txs, as square.Build orders them; k; data
    root)."""
    b = block_extend(ctx, txs, max_square_size, subtree_root_threshold, greedy=True)
    kept = [t for t, s in zip(b.txs, b.included) if s == 1] + [t for t, s in zip(b.txs, b.included) if s == 2]
    return kept, b.k, b.dah
