"""rsmt2d v0.14.0 surface over the device library (Codec, ExtendedDataSquare, Repair).

Mirrors the pieces of github.com/celestiaorg/rsmt2d that celestia-app uses
(pkg/da/data_availability_header.go:45-74, pkg/appconsts/global_consts.go:92):
  LeoRSCodec: Encode / Decode / MaxChunks / Name / ValidateChunkSize
  ComputeExtendedDataSquare, ImportExtendedDataSquare, ExtendedDataSquare.{RowRoots,
  ColRoots, Row, Col, GetCell, Flattened, Width, Repair}
  RepairFromSamples: cells with NMT inclusion proofs, verified on the device, then Repair
  RepairBatch: Repair over many squares in one device call, one outcome per square
  ExtendedDataSquare.SampleProofs: the producer of such samples, one device batch
All arithmetic runs in libcelestia_eds.so (HIP); this module marshals bytes.

Tree constructors. rsmt2d computes each axis root through the TreeConstructorFn it
was given (nmt_wrapper.go:14-17,83). The default constructor (wrapper.NewConstructor)
is served by the device pass that also extends the square. Any other constructor
(pkg/inclusion/nmt_caching.go:96-104's subtree-root cacher, test/util/malicious/
tree.go:36-71's out-of-order tree) is honoured: RowRoots/ColRoots push every cell into
a tree it builds and return that tree's Root(), exactly as rsmt2d does. A codec other
than LeoRSCodec is refused (the device implements Leopard only).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import CelError

Row, Col = 0, 1  # rsmt2d.Axis


class ErrByzantineData(CelError):
    """rsmt2d *ErrByzantineData{Axis, Index, Shares}: Shares lists the axis's 2k shares,
    None where the repair did not know the cell (celestia-node builds bad-encoding fraud
    proofs from them, specs/src/specs/fraud_proofs.md:3-13; here fraud.CreateBadEncodingProof)."""

    def __init__(self, axis, index, message, shares=None):
        super().__init__(_lib.EBYZANTINE, message)
        self.Axis = axis
        self.Index = index
        self.Shares = shares


class ErrUnrepairableDataSquare(CelError):
    def __init__(self, message="failed to solve data square"):
        super().__init__(_lib.EUNREPAIRABLE, message)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class LeoRSCodec:
    """rsmt2d.NewLeoRSCodec(): Leopard GF(2^8) (<=256 shards) / GF(2^16)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or _lib.default_context()

    def Name(self):
        return _lib.load().cel_codec_name().decode()

    def MaxChunks(self):
        return int(_lib.load().cel_codec_max_chunks())

    def ValidateChunkSize(self, chunk_size):
        if _lib.load().cel_codec_validate_chunk_size(int(chunk_size)) != _lib.OK:
            raise CelError(_lib.ECHUNK, f"chunkSize {chunk_size} must be a multiple of 64 bytes")

    def Encode(self, data):
        """data: list of n equal-length byte strings -> list of n parity shards."""
        arr = np.frombuffer(b"".join(bytes(d) for d in data), np.uint8).copy()
        n = len(data)
        ln = len(data[0]) if n else 0
        par = np.zeros(n * ln, np.uint8)
        self.ctx.check(self.ctx.lib.cel_codec_encode(self.ctx.handle, _p(arr), n, ln, _p(par)))
        return [par[i * ln:(i + 1) * ln].tobytes() for i in range(n)]

    def Decode(self, shards):
        """shards: list of 2n entries (None = missing) -> full list of 2n shards."""
        n2 = len(shards)
        ln = next(len(s) for s in shards if s is not None)
        buf = np.zeros(n2 * ln, np.uint8)
        present = np.zeros(n2, np.uint8)
        for i, s in enumerate(shards):
            if s is not None:
                buf[i * ln:(i + 1) * ln] = np.frombuffer(bytes(s), np.uint8)
                present[i] = 1
        self.ctx.check(self.ctx.lib.cel_codec_decode(self.ctx.handle, _p(buf), _p(present), n2 // 2, ln))
        return [buf[i * ln:(i + 1) * ln].tobytes() for i in range(n2)]


def NewLeoRSCodec():
    return LeoRSCodec()


def _default_constructor(tree_constructor, width):
    """True for None and for wrapper.NewConstructor(k) with k = width / 2 (served by the
    device pass). A wrapper constructor for another square size builds trees with another
    Q0 boundary (or fails to push, nmt_wrapper.go:93-99) upstream, so it is treated like
    any caller constructor: its own trees give the roots."""
    if tree_constructor is None:
        return True
    return (getattr(tree_constructor, "_cel_wrapper_constructor", False)
            and getattr(tree_constructor, "square_size", None) == width // 2)


class ExtendedDataSquare:
    """2k x 2k square of 512-byte cells, row-major (rsmt2d flattened layout)."""

    def __init__(self, cells: np.ndarray, row_roots=None, col_roots=None, ctx=None, tree_constructor=None):
        self.cells = cells  # (W, W, share) uint8
        self._row_roots = row_roots
        self._col_roots = col_roots
        self._ctx = ctx
        self._tree = None if _default_constructor(tree_constructor, cells.shape[0]) else tree_constructor

    @property
    def ctx(self):
        # bound on first device use: a square whose roots come from a caller's trees
        # needs no device
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def Width(self):
        return self.cells.shape[0]

    def GetCell(self, r, c):
        return self.cells[r, c].tobytes()

    def Row(self, r):
        return [self.cells[r, c].tobytes() for c in range(self.Width())]

    def Col(self, c):
        return [self.cells[r, c].tobytes() for r in range(self.Width())]

    def Flattened(self):
        return [self.cells[r, c].tobytes() for r in range(self.Width()) for c in range(self.Width())]

    def FlattenedODS(self):
        """The original data square (Q0) row-major, as rsmt2d's FlattenedODS; pkg/proof
        sizes the square from it (pkg/proof/proof.go:84)."""
        k = self.Width() // 2
        return [self.cells[r, c].tobytes() for r in range(k) for c in range(k)]

    def RowRoots(self):
        if self._row_roots is None:
            self._compute_roots()
        return [r.tobytes() for r in self._row_roots]

    def ColRoots(self):
        if self._col_roots is None:
            self._compute_roots()
        return [r.tobytes() for r in self._col_roots]

    def _compute_roots(self):
        w = self.Width()
        if self._tree is not None:
            # a caller's TreeConstructorFn: rsmt2d computeRoots pushes each axis's cells
            rr, cr = [], []
            for axis, out in ((Row, rr), (Col, cr)):
                for i in range(w):
                    tree = self._tree(axis, i)
                    for c in (self.Row(i) if axis == Row else self.Col(i)):
                        tree.Push(c)
                    out.append(np.frombuffer(bytes(tree.Root()), np.uint8))
            self._row_roots, self._col_roots = rr, cr
            return
        rr = np.zeros((w, _lib.NMT_NODE_SIZE), np.uint8)
        cr = np.zeros((w, _lib.NMT_NODE_SIZE), np.uint8)
        for axis, out in ((Row, rr), (Col, cr)):
            for i in range(w):
                cells = np.ascontiguousarray(self.cells[i] if axis == Row else self.cells[:, i])
                self.ctx.check(self.ctx.lib.cel_axis_root(self.ctx.handle, _p(cells), w // 2, i,
                                                          _lib.SHARE_SIZE, _p(out[i]), 0))
        self._row_roots, self._col_roots = rr, cr

    def SharesByNamespace(self, namespace):
        """Every share of `namespace` (29 bytes) in this square with the proofs that none was left
        out, what celestia-node's GetSharesByNamespace serves: for each row whose root range holds
        the namespace, in row order, (row, NMTProof, shares) with nmt ProveNamespace's proof
        against RowRoots()[row]: the namespace's shares of that row, or an absence proof (LeafHash
        set, no shares). One device call (cel_namespace_rows: upload, tree index, search, proofs,
        download). The parity namespace raises CelError(EINVAL); a square whose shares are not in
        namespace order, CelError(EORDER)."""
        from .proof import NMTProof
        ns = bytes(namespace)
        if len(ns) != _lib.NAMESPACE_SIZE:
            raise CelError(_lib.EINVAL, f"a namespace is {_lib.NAMESPACE_SIZE} bytes")
        c, w, share, node = self.ctx, self.Width(), _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
        cells = np.ascontiguousarray(self.cells, dtype=np.uint8)
        nsa = np.frombuffer(ns, np.uint8).copy()
        cnt, tl, tn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        c.check(c.lib.cel_namespace_rows(c.handle, _p(cells), w // 2, 1, _p(nsa), 0, 0, 0, *([None] * 9),
                                         ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn)))
        m = cnt.value
        if m == 0:
            return []
        ns_idx, rows = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        starts, ends, kinds = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
        leaf_off, node_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
        leaves, nodes = np.zeros((max(tl.value, 1), share), np.uint8), np.zeros((max(tn.value, 1), node), np.uint8)
        c.check(c.lib.cel_namespace_rows(c.handle, _p(cells), w // 2, 1, _p(nsa), m, tl.value, tn.value, _p(ns_idx),
                                         _p(rows), _p(starts), _p(ends), _p(kinds), _p(leaf_off), _p(node_off),
                                         _p(leaves), _p(nodes), ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn)))
        out = []
        for e in range(m):
            nd = [nodes[j].tobytes() for j in range(int(node_off[e]), int(node_off[e + 1]))]
            absent = int(kinds[e]) == _lib.NS_ABSENCE
            out.append((int(rows[e]),
                        NMTProof(Start=int(starts[e]), End=int(ends[e]), Nodes=nd[:-1] if absent else nd,
                                 LeafHash=nd[-1] if absent else None),
                        [leaves[j].tobytes() for j in range(int(leaf_off[e]), int(leaf_off[e + 1]))]))
        return out

    def Blobs(self, namespaces, commitments=True, threshold=64):
        """The blobs of `namespaces` (29 bytes each, no reserved ones) in this square, what
        celestia-node's blob.GetAll serves: per namespace a list of blob.Blob (each with its share
        commitment and the ODS index of its first share), or the blob.BlobParseError of a
        namespace whose shares do not parse. The host-memory form: cel_namespace_rows finds the
        shares, cel_namespace_ods_ranges turns them into ODS ranges, cel_blobs_by_range uploads,
        parses, gathers and commits."""
        from . import blob as _blob
        nss = _blob.check_blob_namespaces(namespaces)
        n = len(nss)
        if n == 0:
            return []
        c, k = self.ctx, self.Width() // 2
        cells = np.ascontiguousarray(self.cells, dtype=np.uint8)
        nsa = np.frombuffer(b"".join(nss), np.uint8).copy()
        cnt, tl, tn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        c.check(c.lib.cel_namespace_rows(c.handle, _p(cells), k, n, _p(nsa), 0, 0, 0, *([None] * 9),
                                         ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn)))
        m = cnt.value
        plan = dict(ns_idx=np.zeros(m, np.uint32), rows=np.zeros(m, np.uint32), starts=np.zeros(m, np.int32),
                    ends=np.zeros(m, np.int32), kinds=np.zeros(m, np.uint8))
        if m:
            leaf_off, node_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
            leaves = np.zeros((max(tl.value, 1), _lib.SHARE_SIZE), np.uint8)
            nodes = np.zeros((max(tn.value, 1), _lib.NMT_NODE_SIZE), np.uint8)
            c.check(c.lib.cel_namespace_rows(c.handle, _p(cells), k, n, _p(nsa), m, tl.value, tn.value,
                                             _p(plan["ns_idx"]), _p(plan["rows"]), _p(plan["starts"]), _p(plan["ends"]),
                                             _p(plan["kinds"]), _p(leaf_off), _p(node_off), _p(leaves), _p(nodes),
                                             ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn)))
        ranges = _blob.ods_ranges(k, n, plan)
        starts = np.array([a for a, _ in ranges], np.uint32)
        ends = np.array([b for _, b in ranges], np.uint32)
        status = np.zeros(n, np.uint32)
        nb, tb = ctypes.c_uint64(), ctypes.c_uint64()
        c.check(c.lib.cel_blobs_by_range(c.handle, _p(cells), k, n, _p(starts), _p(ends), 0, 0, None, _p(status), None,
                                         None, threshold, ctypes.byref(nb), ctypes.byref(tb)))
        cap, nbytes = nb.value, tb.value
        recs = (_blob.BlobRec * max(cap, 1))()
        data = np.zeros(max(nbytes, 1), np.uint8)
        com = np.zeros((max(cap, 1), 32), np.uint8) if commitments else None
        if cap:
            c.check(c.lib.cel_blobs_by_range(c.handle, _p(cells), k, n, _p(starts), _p(ends), cap, nbytes, recs,
                                             _p(status), _p(data), _p(com) if commitments else None, threshold,
                                             ctypes.byref(nb), ctypes.byref(tb)))
        return _blob.blobs_from_records(list(recs[:cap]), status, data, com, n)

    def Txs(self, hashes=False):
        """The units of this square's two compact namespaces, what shares.ParseTxs and
        square.Deconstruct read: (txs, PayForBlob index wrappers), or with hashes=True
        ((txs, their SHA-256), (wrappers, theirs)). The host-memory form: the runs of the two
        namespaces at the head of the ODS are found here, cel_txs_by_range uploads, parses,
        gathers and hashes. Shares that do not parse raise square.TxParseError."""
        from . import square as _square
        c, k = self.ctx, self.Width() // 2
        cells = np.ascontiguousarray(self.cells, dtype=np.uint8)
        ranges = _square._compact_runs(cells[:k, :k].reshape(k * k, _lib.SHARE_SIZE))
        starts = np.array([a for a, _ in ranges], np.uint32)
        ends = np.array([b for _, b in ranges], np.uint32)
        status, flags = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        nu, tb = ctypes.c_uint64(), ctypes.c_uint64()
        c.check(c.lib.cel_txs_by_range(c.handle, _p(cells), k, 2, _p(starts), _p(ends), 0, 0, None, _p(status),
                                       _p(flags), None, None, ctypes.byref(nu), ctypes.byref(tb)))
        cap, nbytes = nu.value, tb.value
        recs = (_square.TxRec * max(cap, 1))()
        data = np.zeros(max(nbytes, 1), np.uint8)
        hs = np.zeros((max(cap, 1), 32), np.uint8)
        if cap:
            c.check(c.lib.cel_txs_by_range(c.handle, _p(cells), k, 2, _p(starts), _p(ends), cap, nbytes, recs,
                                           _p(status), _p(flags), _p(data), _p(hs) if hashes else None,
                                           ctypes.byref(nu), ctypes.byref(tb)))
        out = _square.units_from_records(list(recs[:cap]), status, data, 2)
        for got in out:
            if isinstance(got, Exception):
                raise got
        if not hashes:
            return tuple(out)
        n_tx = len(out[0])
        return (out[0], [h.tobytes() for h in hs[:n_tx]]), (out[1], [h.tobytes() for h in hs[n_tx:cap]])

    def SampleProofs(self, coords):
        """Samples of this square with their single-leaf NMT proofs, in one device batch
        (cel_prove_samples: upload, tree index, proofs, download). coords: (row, col, axis)
        each; returns (row, col, axis, share, nodes) each, RepairFromSamples' format: the cell
        proved against RowRoots()[row] at leaf col (axis Row) or against ColRoots()[col] at leaf
        row (axis Col) under the default wrapper trees. A coordinate outside the square or an
        axis other than Row / Col raises CelError(EINVAL)."""
        coords = [(int(r), int(c), int(a)) for r, c, a in coords]
        if not coords:
            return []
        w, share, node = self.Width(), _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
        for i, (r, c, a) in enumerate(coords):
            if not (0 <= r < w and 0 <= c < w and a in (Row, Col)):
                raise CelError(_lib.EINVAL, f"sample {i}: cell ({r}, {c}) axis {a} outside the square of width {w}")
        n, per = len(coords), w.bit_length() - 1  # a single-leaf proof has log2(2k) nodes
        rows = np.array([r for r, _, _ in coords], np.uint32)
        cols = np.array([c for _, c, _ in coords], np.uint32)
        axes = np.array([a for _, _, a in coords], np.uint8)
        cells = np.ascontiguousarray(self.cells, dtype=np.uint8)
        shares = np.zeros((n, share), np.uint8)
        nodes = np.zeros((max(n * per, 1), node), np.uint8)
        node_off = np.zeros(n + 1, np.uint64)
        self.ctx.check(self.ctx.lib.cel_prove_samples(self.ctx.handle, _p(cells), w // 2, n, _p(rows), _p(cols),
                                                      _p(axes), _p(shares), _p(nodes), _p(node_off)))
        return [(r, c, a, shares[i].tobytes(), [nodes[j].tobytes() for j in range(int(node_off[i]), int(node_off[i + 1]))])
                for i, (r, c, a) in enumerate(coords)]

    def Repair(self, row_roots, col_roots, present=None):
        """Fill every missing cell (present mask False) and verify against the roots.
        Raises ErrByzantineData (with the axis's Shares) / ErrUnrepairableDataSquare like
        rsmt2d, and CelError(EBADROOT) for rsmt2d's "bad root input". Returns the mask the
        square is valid under (all ones on success; the caller's array is not modified)."""
        w = self.Width()
        mask = np.ones((w, w), np.uint8) if present is None else np.array(present, np.uint8, copy=True)
        rr = np.frombuffer(b"".join(row_roots), np.uint8).copy()
        cr = np.frombuffer(b"".join(col_roots), np.uint8).copy()
        cells = np.array(self.cells, np.uint8, copy=True, order="C")
        ba, bi = ctypes.c_int32(-1), ctypes.c_int32(-1)
        bs = np.zeros((w, _lib.SHARE_SIZE), np.uint8)
        bp = np.zeros(w, np.uint8)
        st = self.ctx.lib.cel_repair(self.ctx.handle, _p(cells), _p(mask), w // 2, _lib.SHARE_SIZE, _p(rr),
                                     _p(cr), ctypes.byref(ba), ctypes.byref(bi), _p(bs), _p(bp))
        if st in (_lib.OK, _lib.EBYZANTINE, _lib.EBADROOT, _lib.EUNREPAIRABLE):
            self.cells = cells  # the most-repaired square (valid where mask is set)
            self._mask = mask
        if st == _lib.EBYZANTINE:
            shares = [bs[j].tobytes() if bp[j] else None for j in range(w)]
            raise ErrByzantineData(ba.value, bi.value, self.ctx.lib.cel_last_error(self.ctx.handle).decode(),
                                   shares)
        if st == _lib.EUNREPAIRABLE:
            raise ErrUnrepairableDataSquare()
        self.ctx.check(st)
        self._row_roots = np.frombuffer(rr.tobytes(), np.uint8).reshape(w, -1).copy()
        self._col_roots = np.frombuffer(cr.tobytes(), np.uint8).reshape(w, -1).copy()
        return mask


def RepairBatch(squares, row_roots, col_roots, presents=None, ctx=None):
    """ExtendedDataSquare.Repair over many squares of one width in one device call
    (cel_repair_batch): squares[i] an ExtendedDataSquare or a (W, W, 512) array, row_roots[i] /
    col_roots[i] its 2k roots, presents[i] its mask (None: all present). Returns one item per
    square: the repaired ExtendedDataSquare (with its _mask), or, not raised, the error Repair
    would raise for that square alone (ErrByzantineData with Axis, Index and Shares,
    ErrUnrepairableDataSquare, CelError(EBADROOT)); an error carries `.square`, the
    most-repaired ExtendedDataSquare with the mask it is valid under, as Repair leaves on self."""
    ctx = ctx or _lib.default_context()
    n = len(squares)
    if n == 0:
        return []
    if len(row_roots) != n or len(col_roots) != n or (presents is not None and len(presents) != n):
        raise CelError(_lib.EINVAL, f"need roots (and masks) for each of the {n} squares")
    cells = np.stack([np.asarray(s.cells if isinstance(s, ExtendedDataSquare) else s, np.uint8) for s in squares])
    w = cells.shape[1]
    if cells.shape != (n, w, w, _lib.SHARE_SIZE):
        raise CelError(_lib.EINVAL, f"squares must be {w} x {w} cells of {_lib.SHARE_SIZE} bytes")
    cells = np.ascontiguousarray(cells)
    mask = (np.ones((n, w, w), np.uint8) if presents is None
            else np.ascontiguousarray(np.stack([np.asarray(p, np.uint8) for p in presents])))
    rr = np.frombuffer(b"".join(b"".join(bytes(x) for x in r) for r in row_roots), np.uint8).copy()
    cr = np.frombuffer(b"".join(b"".join(bytes(x) for x in c) for c in col_roots), np.uint8).copy()
    if mask.shape != (n, w, w) or rr.size != n * w * _lib.NMT_NODE_SIZE or cr.size != rr.size:
        raise CelError(_lib.EINVAL, f"need {w} x {w} masks and {w} row and column roots per square")
    status = np.zeros(n, np.int32)
    ba, bi = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    bs = np.zeros((n, w, _lib.SHARE_SIZE), np.uint8)
    bp = np.zeros((n, w), np.uint8)
    ctx.check(ctx.lib.cel_repair_batch(ctx.handle, _p(cells), _p(mask), n, w // 2, _lib.SHARE_SIZE, _p(rr), _p(cr),
                                       _p(status), _p(ba), _p(bi), _p(bs), _p(bp)))
    out = []
    for i in range(n):
        sq = ExtendedDataSquare(cells[i], ctx=ctx)
        sq._mask = mask[i]
        st = int(status[i])
        if st == _lib.OK:
            node = _lib.NMT_NODE_SIZE
            sq._row_roots = rr[i * w * node:(i + 1) * w * node].reshape(w, node).copy()
            sq._col_roots = cr[i * w * node:(i + 1) * w * node].reshape(w, node).copy()
            out.append(sq)
            continue
        dirn = "column" if ba[i] else "row"
        if st == _lib.EBYZANTINE:
            err = ErrByzantineData(int(ba[i]), int(bi[i]), f"byzantine {dirn} {int(bi[i])}",
                                   [bs[i, j].tobytes() if bp[i, j] else None for j in range(w)])
        elif st == _lib.EUNREPAIRABLE:
            err = ErrUnrepairableDataSquare()
        else:
            err = CelError(st, f"bad root input: {'col' if ba[i] else 'row'} {int(bi[i])}")
        err.square = sq
        out.append(err)
    return out


def _check_codec(codec):
    if codec is not None and not isinstance(codec, LeoRSCodec):
        raise CelError(_lib.EINVAL, f"unsupported codec {type(codec).__name__}: the device path implements "
                                    "rsmt2d's LeoRSCodec only")


def ComputeExtendedDataSquare(data, codec=None, tree_constructor=None, ctx=None):
    """rsmt2d.ComputeExtendedDataSquare(data, codec, treeCreatorFn). One device pass
    extends the square; with the default wrapper constructor it also computes all 4k
    roots, with any other constructor the roots come from the caller's trees."""
    from . import da
    _check_codec(codec)
    eds = da._extend(data, ctx=ctx, order_check=True)
    if not _default_constructor(tree_constructor, eds.Width()):
        eds._row_roots = eds._col_roots = None
        eds._tree = tree_constructor
    return eds


def ImportExtendedDataSquare(flattened, codec=None, tree_constructor=None, ctx=None):
    _check_codec(codec)
    n = len(flattened)
    w = int(round(n ** 0.5))
    cells = np.frombuffer(b"".join(flattened), np.uint8).reshape(w, w, -1).copy()
    return ExtendedDataSquare(cells, ctx=ctx, tree_constructor=tree_constructor)


def RepairFromSamples(k, samples, row_roots, col_roots, ctx=None):
    """Repair a 2k x 2k square from sampled cells that come with NMT inclusion proofs
    (cel_repair_samples): samples = (row, col, axis, share, nodes) with `nodes` the
    single-leaf nmt proof of the cell against row_roots[row] (axis Row) or col_roots[col]
    (axis Col). Every proof is verified on the device; accepted samples fill the square,
    which is then repaired as ExtendedDataSquare.Repair does. Returns (ExtendedDataSquare,
    ok) with ok[i] the verdict of sample i; a share that is not 512 bytes long or a node
    that is not 90 is False without reaching the device. Raises what Repair raises."""
    ctx = ctx or _lib.default_context()
    w, share, node = 2 * k, _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
    samples = list(samples)
    ok = [False] * len(samples)
    keep = [i for i, s in enumerate(samples) if len(s[3]) == share and all(len(x) == node for x in s[4])
            and 0 <= s[0] < 1 << 32 and 0 <= s[1] < 1 << 32 and 0 <= s[2] < 256]
    buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    rows = np.array([samples[i][0] for i in keep] or [0], np.uint32)
    cols = np.array([samples[i][1] for i in keep] or [0], np.uint32)
    axes = np.array([samples[i][2] for i in keep] or [0], np.uint8)
    shares = buf(bytes(samples[i][3]) for i in keep)
    nodes = buf(bytes(x) for i in keep for x in samples[i][4])
    node_off = np.cumsum([0] + [len(samples[i][4]) for i in keep]).astype(np.uint64)
    rr = np.frombuffer(b"".join(row_roots), np.uint8).copy()
    cr = np.frombuffer(b"".join(col_roots), np.uint8).copy()
    if rr.size != w * node or cr.size != w * node:
        raise CelError(_lib.EINVAL, f"need {w} row roots and {w} column roots of {node} bytes")
    okd = np.zeros(max(len(keep), 1), np.uint8)
    cells = np.zeros((w, w, share), np.uint8)
    mask = np.zeros((w, w), np.uint8)
    ba, bi = ctypes.c_int32(-1), ctypes.c_int32(-1)
    bs = np.zeros((w, share), np.uint8)
    bp = np.zeros(w, np.uint8)
    st = ctx.lib.cel_repair_samples(ctx.handle, k, _p(rr), _p(cr), len(keep), _p(rows), _p(cols), _p(axes),
                                    _p(shares), _p(nodes), _p(node_off), _p(okd), _p(cells), _p(mask),
                                    ctypes.byref(ba), ctypes.byref(bi), _p(bs), _p(bp))
    for i, v in zip(keep, okd):
        ok[i] = bool(v)
    sq = ExtendedDataSquare(cells, ctx=ctx)
    sq._mask = mask
    if st == _lib.EBYZANTINE:
        shares_out = [bs[j].tobytes() if bp[j] else None for j in range(w)]
        raise ErrByzantineData(ba.value, bi.value, ctx.lib.cel_last_error(ctx.handle).decode(), shares_out)
    if st == _lib.EUNREPAIRABLE:
        raise ErrUnrepairableDataSquare()
    ctx.check(st)
    sq._row_roots = rr.reshape(w, -1).copy()
    sq._col_roots = cr.reshape(w, -1).copy()
    return sq, ok


def _squares_by_width(squares, picks, what):
    """`squares` as (W, W, 512) arrays, and the numbers of the requests whose square (picks[i]) has
    each width, in request order: {W: (the squares of that width that are asked for, their
    stacked cells, request numbers)}."""
    cells = [np.ascontiguousarray(getattr(s, "cells", s), dtype=np.uint8) for s in squares]
    groups = {}
    for i, q in enumerate(picks):
        if not 0 <= q < len(cells):
            raise CelError(_lib.EINVAL, f"{what} {i}: square {q} of {len(cells)}")
        x = cells[q]
        if x.ndim != 3 or x.shape[0] != x.shape[1] or x.shape[2] != _lib.SHARE_SIZE:
            raise CelError(_lib.EINVAL, f"square {q}: need a (2k, 2k, {_lib.SHARE_SIZE}) square, got {x.shape}")
        sqs, ids = groups.setdefault(x.shape[0], ([], []))
        if q not in sqs:
            sqs.append(q)
        ids.append(i)
    return {w: (sqs, np.stack([cells[q] for q in sqs]), ids) for w, (sqs, ids) in groups.items()}


def SampleProofsBatch(squares, samples, ctx=None):
    """ExtendedDataSquare.SampleProofs over many squares at once: samples = (square, row, col,
    axis) each, `square` a position in `squares` (ExtendedDataSquares or (2k, 2k, 512) arrays,
    mixed widths). The squares that are asked for go up grouped by width, one
    cel_prove_samples_squares per width (upload, batch tree index, proofs, download). Returns
    (square, row, col, axis, share, nodes) per sample, in the samples' order; the last five are
    RepairFromSamples' format."""
    ctx = ctx or next((s._ctx for s in squares if getattr(s, "_ctx", None)), None) or _lib.default_context()
    reqs = [(int(q), int(r), int(c), int(a)) for q, r, c, a in samples]
    out = [None] * len(reqs)
    share, node = _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
    for w, (sqs, cells, ids) in _squares_by_width(squares, [q for q, _, _, _ in reqs], "sample").items():
        for i in ids:
            _, r, c, a = reqs[i]
            if not (0 <= r < w and 0 <= c < w and a in (Row, Col)):
                raise CelError(_lib.EINVAL, f"sample {i}: cell ({r}, {c}) axis {a} outside the square of width {w}")
        n, per = len(ids), w.bit_length() - 1
        sq = np.array([sqs.index(reqs[i][0]) for i in ids], np.uint32)
        rows = np.array([reqs[i][1] for i in ids], np.uint32)
        cols = np.array([reqs[i][2] for i in ids], np.uint32)
        axes = np.array([reqs[i][3] for i in ids], np.uint8)
        shares, nodes = np.zeros((n, share), np.uint8), np.zeros((max(n * per, 1), node), np.uint8)
        node_off = np.zeros(n + 1, np.uint64)
        ctx.check(ctx.lib.cel_prove_samples_squares(ctx.handle, _p(cells), len(sqs), w // 2, n, _p(sq), _p(rows), _p(cols),
                                                    _p(axes), _p(shares), _p(nodes), _p(node_off)))
        for j, i in enumerate(ids):
            out[i] = reqs[i] + (shares[j].tobytes(),
                                [nodes[t].tobytes() for t in range(int(node_off[j]), int(node_off[j + 1]))])
    return out


def SharesByNamespaceBatch(squares, queries, ctx=None):
    """ExtendedDataSquare.SharesByNamespace over many squares at once: queries = (square,
    namespace) each. Returns, per query, what squares[square].SharesByNamespace(namespace)
    returns: (row, NMTProof, shares) for each row whose root range holds the namespace. One
    cel_namespace_rows_squares per width, called twice as SharesByNamespace calls the
    single-square form twice: once for the counts, once for the entries. Each call uploads that
    width's squares and builds their index, so a width costs two uploads and two index builds; a
    caller that asks the same squares more than once keeps them resident with
    proof.TreeIndexBatch, which uploads and indexes once and plans once per call. The parity
    namespace raises CelError(EINVAL); a square whose shares are not in namespace order,
    CelError(EORDER)."""
    from .proof import NMTProof
    ctx = ctx or next((s._ctx for s in squares if getattr(s, "_ctx", None)), None) or _lib.default_context()
    qs = [(int(q), bytes(ns)) for q, ns in queries]
    if any(len(ns) != _lib.NAMESPACE_SIZE for _, ns in qs):
        raise CelError(_lib.EINVAL, f"a namespace is {_lib.NAMESPACE_SIZE} bytes")
    out = [[] for _ in qs]
    share, node = _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
    for w, (sqs, cells, ids) in _squares_by_width(squares, [q for q, _ in qs], "query").items():
        n = len(ids)
        sq = np.array([sqs.index(qs[i][0]) for i in ids], np.uint32)
        nsa = np.frombuffer(b"".join(qs[i][1] for i in ids), np.uint8).copy()
        cnt, tl, tn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        tail = (ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn))
        ctx.check(ctx.lib.cel_namespace_rows_squares(ctx.handle, _p(cells), len(sqs), w // 2, n, _p(sq), _p(nsa), 0, 0, 0,
                                                     *([None] * 9), *tail))
        m = cnt.value
        if m == 0:
            continue
        qi, rows = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        starts, ends, kinds = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
        leaf_off, node_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
        leaves, nodes = np.zeros((max(tl.value, 1), share), np.uint8), np.zeros((max(tn.value, 1), node), np.uint8)
        ctx.check(ctx.lib.cel_namespace_rows_squares(ctx.handle, _p(cells), len(sqs), w // 2, n, _p(sq), _p(nsa), m,
                                                     tl.value, tn.value, _p(qi), _p(rows), _p(starts), _p(ends), _p(kinds),
                                                     _p(leaf_off), _p(node_off), _p(leaves), _p(nodes), *tail))
        for e in range(m):
            nd = [nodes[j].tobytes() for j in range(int(node_off[e]), int(node_off[e + 1]))]
            absent = int(kinds[e]) == _lib.NS_ABSENCE
            out[ids[int(qi[e])]].append((int(rows[e]),
                                         NMTProof(Start=int(starts[e]), End=int(ends[e]), Nodes=nd[:-1] if absent else nd,
                                                  LeafHash=nd[-1] if absent else None),
                                         [leaves[j].tobytes() for j in range(int(leaf_off[e]), int(leaf_off[e + 1]))]))
    return out
