"""go-square v1.1.0 data-square construction, mirrored over the
C ABI's cel_square_construct (host code in csrc/square.cpp, no device needed).

  Construct(txs, max_square_size, subtree_root_threshold)
      square.Construct as called by app/extend_block.go:16-25 and
      app/process_proposal.go:121-130: the exact ordered tx list -> the k*k shares
      handed to da.ExtendShares; raises CelError if a tx does not fit or a normal tx
      follows a blob tx (go-square's error strings).
  Build(txs, max_square_size, subtree_root_threshold)
      square.Build as called by app/prepare_proposal.go:48-61: greedy, drops what does
      not fit; returns (shares, kept txs with normal txs before blob txs).
  parse_compact_shares(shares), ParseTxs(shares)
      shares.parseCompactShares / ParseTxs on the host: the units of compact shares, the
      checker of the device path (cel_dev_txs_plan, proof.TreeIndex.txs_flat).
  Deconstruct(index_or_eds_or_ods)
      square.Deconstruct, the inverse of Construct: the block's txs out of its square, the
      BlobTxs rebuilt from the PayForBlob index wrappers and the blobs they point at.

The defaults are appconsts SquareSizeUpperBound = 128 and SubtreeRootThreshold = 64
(pkg/appconsts/v1,v2/app_consts.go).
"""
import bisect
import ctypes

import numpy as np

from . import _lib

SQUARE_SIZE_UPPER_BOUND = 128
SUBTREE_ROOT_THRESHOLD = 64


def _call(txs, max_square_size, subtree_root_threshold, greedy):
    l = _lib.load()
    txs = [bytes(t) for t in txs]
    lens = (ctypes.c_uint32 * max(len(txs), 1))(*[len(t) for t in txs])
    blob = b"".join(txs)
    buf = ctypes.create_string_buffer(blob, max(len(blob), 1))
    k = ctypes.c_uint32()
    included = (ctypes.c_uint8 * max(len(txs), 1))()

    def run(out, cap):
        return l.cel_square_construct(buf, lens, len(txs), max_square_size, subtree_root_threshold, greedy,
                                      out, cap, ctypes.byref(k), included)

    st = run(None, 0)
    if st != _lib.OK:
        raise _lib.CelError(st, l.cel_square_last_error().decode())
    n = k.value * k.value
    out = np.zeros((n, _lib.SHARE_SIZE), np.uint8)
    st = run(out.ctypes.data_as(ctypes.c_void_p), n)
    if st != _lib.OK:
        raise _lib.CelError(st, l.cel_square_last_error().decode())
    return out, [int(included[i]) for i in range(len(txs))]


def Construct(txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """-> uint8 array [k*k][512]: the ODS shares (shares.ToBytes of the square)."""
    return _call(txs, max_square_size, subtree_root_threshold, 0)[0]


def Build(txs, max_square_size=SQUARE_SIZE_UPPER_BOUND, subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """-> (shares [k*k][512], kept txs: normal txs first, then blob txs)."""
    out, kept = _call(txs, max_square_size, subtree_root_threshold, 1)
    normal = [bytes(t) for t, s in zip(txs, kept) if s == 1]
    blob = [bytes(t) for t, s in zip(txs, kept) if s == 2]
    return out, normal + blob


def TxShareRange(txs, tx_index, max_square_size=SQUARE_SIZE_UPPER_BOUND,
                 subtree_root_threshold=SUBTREE_ROOT_THRESHOLD):
    """Builder.FindTxShareRange after square.Construct(txs): (start, end) ODS shares of tx
    `tx_index` (its PFB index wrapper for a blob tx)."""
    l = _lib.load()
    txs = [bytes(t) for t in txs]
    lens = (ctypes.c_uint32 * max(len(txs), 1))(*[len(t) for t in txs])
    blob = b"".join(txs)
    buf = ctypes.create_string_buffer(blob, max(len(blob), 1))
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    st = l.cel_square_tx_range(buf, lens, len(txs), max_square_size, subtree_root_threshold, tx_index,
                               ctypes.byref(a), ctypes.byref(b))
    if st != _lib.OK:
        raise _lib.CelError(st, l.cel_square_last_error().decode())
    return a.value, b.value


def is_blob_tx(tx):
    """blob.UnmarshalBlobTx's verdict, read from a one-tx square.Build (included code 2 =
    kept blob tx; a blob tx too large for a 128 x 128 square reads as not kept)."""
    return _call([tx], SQUARE_SIZE_UPPER_BOUND, SUBTREE_ROOT_THRESHOLD, 1)[1][0] == 2


# ------------------------------------------------------------------ compact shares back to txs
# go-square v1.1.0 parseCompactShares / square.Deconstruct, the inverse of Construct. The rules
# are those of include/celestia_eds.h ("txs by range"); this is their plain statement, the
# checker of the device path (csrc/tx_parse.hip).
TX_NAMESPACE = bytes(28) + b"\x01"
PFB_NAMESPACE = bytes(28) + b"\x04"
TX_EVERSION, TX_ENAMESPACE, TX_ERESERVED, TX_EVARINT = _lib.TX_EVERSION, _lib.TX_ENAMESPACE, _lib.TX_ERESERVED, \
    _lib.TX_EVARINT
TX_FHINTS = _lib.TX_FHINTS
_TX_MESSAGES = {TX_EVERSION: "unsupported share version", TX_ENAMESPACE: "a share of a namespace that holds no compact shares",
                TX_ERESERVED: "the reserved bytes of the first share point beyond it",
                TX_EVARINT: "a unit's length prefix overflows 64 bits"}


class TxRec(ctypes.Structure):
    """cel_tx_rec"""
    _fields_ = [("range", ctypes.c_uint32), ("share", ctypes.c_uint32), ("share_off", ctypes.c_uint32),
                ("shares", ctypes.c_uint32), ("len", ctypes.c_uint64), ("data_off", ctypes.c_uint64)]


assert ctypes.sizeof(TxRec) == 32


def units_from_records(recs, status, data, n_ranges):
    """Per range the list of its units' bytes, or the TxParseError of a failed range."""
    out = [[] if int(status[r]) == 0 else TxParseError(int(status[r]), f"range {r}") for r in range(n_ranges)]
    for r in recs:
        out[r.range].append(data[int(r.data_off):int(r.data_off) + int(r.len)].tobytes())
    return out


class TxParseError(_lib.CelError):
    """A range that the compact share parser rejects: kind is one of TX_E* (the range status
    codes CEL_TX_E* of the C ABI)."""

    def __init__(self, kind, detail=""):
        super().__init__(_lib.EINVAL, _TX_MESSAGES[kind] + (f": {detail}" if detail else ""))
        self.kind = kind


def _uvarint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def compact_walk(shares):
    """The compact share parser over `shares` ([n][512] uint8 or a list of 512-byte strings):
    (status, flags, units). status: 0 or the first TX_E* in the order version, namespace,
    reserved, varint; a failed range has no units. units: (bytes, share, share_off, shares) with
    the share of the list in which the unit's length prefix begins, the byte of that share it
    begins at and the number of shares that prefix and unit touch (FindTxShareRange's count).
    flags: TX_FHINTS where the reserved bytes disagree with this sequential parse: with the last
    unit beginning in share t, a later share j <= t in which a unit begins must name the first
    such unit's byte (h <= R < 512), and one in which none begins must hold no usable value."""
    a = np.asarray(shares, np.uint8) if not isinstance(shares, (list, tuple)) else \
        np.frombuffer(b"".join(bytes(s) for s in shares), np.uint8)
    a = a.reshape(-1, _lib.SHARE_SIZE)
    n = len(a)
    ns = _lib.NAMESPACE_SIZE
    if any(int(sh[ns]) >> 1 for sh in a):
        return TX_EVERSION, 0, []
    if any(sh[:ns].tobytes() not in (TX_NAMESPACE, PFB_NAMESPACE) for sh in a):
        return TX_ENAMESPACE, 0, []
    if n == 0:
        return 0, 0, []
    hs = [38 if int(sh[ns]) & 1 else 34 for sh in a]
    rs = [int.from_bytes(a[j, hs[j] - 4:hs[j]].tobytes(), "big") for j in range(n)]
    if rs[0] >= 512:
        return TX_ERESERVED, 0, []
    hdr = [rs[0]] + hs[1:]  # the share byte at which a share's contribution begins
    parts = [b"" if rs[0] == 0 else a[0, rs[0]:].tobytes()] + [a[j, hs[j]:].tobytes() for j in range(1, n)]
    base = [0]
    for part in parts:
        base.append(base[-1] + len(part))
    stream = b"".join(parts)
    size = len(stream)

    def share_of(x):  # the last share whose contribution begins at or before stream byte x
        return min(bisect.bisect_right(base, x) - 1, n - 1)

    status, units, starts, p = 0, [], [], 0
    while p < size:
        window = stream[p:p + 10].ljust(10, b"\0")
        length, i = 0, 0
        while i < 10 and window[i] & 0x80:
            length |= (window[i] & 0x7F) << (7 * i)
            i += 1
        if i == 10 or (i == 9 and window[i] > 1):
            status = TX_EVARINT
            break
        length |= window[i] << (7 * i)
        k = len(_uvarint(length))
        if length == 0 or length > size - (p + k):
            break
        first, last = share_of(p), share_of(p + k + length - 1)
        units.append((stream[p + k:p + k + length], first, hdr[first] + p - base[first], last - first + 1))
        starts.append(p)
        p += k + length
    flags = 0
    if starts:
        begin = {}
        for s in starts:
            begin.setdefault(share_of(s), s)
        for j in range(1, share_of(starts[-1]) + 1):
            usable = hs[j] <= rs[j] < 512
            if (j in begin) != usable or (usable and rs[j] != hs[j] + begin[j] - base[j]):
                flags = TX_FHINTS
    return status, flags, ([] if status else units)


def parse_compact_shares(shares):
    """go-square parseCompactShares: the units (txs, or PFB index wrappers) of the compact
    shares in order, or TxParseError with the range's status."""
    status, _, units = compact_walk(shares)
    if status:
        raise TxParseError(status)
    return [u[0] for u in units]


def ParseTxs(shares):
    """shares.ParseTxs: parse_compact_shares over the shares of the tx namespace among `shares`."""
    a = np.asarray(shares, np.uint8) if not isinstance(shares, (list, tuple)) else \
        np.frombuffer(b"".join(bytes(s) for s in shares), np.uint8)
    a = a.reshape(-1, _lib.SHARE_SIZE)
    keep = [j for j in range(len(a)) if a[j, :_lib.NAMESPACE_SIZE].tobytes() == TX_NAMESPACE]
    return parse_compact_shares(a[keep])


def unwrap_index_wrapper(unit):
    """(inner tx, share indexes) of an IndexWrapper {1: tx, 2: packed share_indexes, 3: type_id
    "INDX"}, the inverse of marshal_index_wrapper in csrc/square.cpp; None when `unit` does not
    decode as one."""
    from .proof import _Reader
    r = _Reader(unit, "IndexWrapper")
    tx, idx, type_id = b"", [], b""
    try:
        for f, wt in r.fields():
            if f == 1 and wt == 2:
                tx = r.lendelim()
            elif f == 2 and wt == 2:
                packed = _Reader(r.lendelim(), "IndexWrapper.share_indexes")
                while packed.i < len(packed.buf):
                    idx.append(packed.uvarint() & 0xFFFFFFFF)
            elif f == 2 and wt == 0:
                idx.append(r.uvarint() & 0xFFFFFFFF)
            elif f == 3 and wt == 2:
                type_id = r.lendelim()
            elif f in (1, 2, 3):
                return None
            else:
                r.skip(wt)
    except _lib.CelError:
        return None
    return (tx, idx) if type_id == b"INDX" else None


def marshal_blob_tx(inner, blobs):
    """The gogoproto bytes of BlobTx {1: tx, 2: blobs, 3: type_id "BLOB"} with every Blob
    {1: namespace_id, 2: data, 3: share_version, 4: namespace_version}; blobs: blob.Blob or
    (namespace (29 bytes), data[, share_version]). Zero-valued fields are omitted."""
    def field(num, data):
        return _uvarint(num << 3 | 2) + _uvarint(len(data)) + data

    out = field(1, bytes(inner)) if len(inner) else b""
    for b in blobs:
        ns, data, ver = (b.namespace, b.data, b.share_version) if hasattr(b, "namespace") else \
            (bytes(b[0]), bytes(b[1]), b[2] if len(b) > 2 else 0)
        m = (field(1, ns[1:]) if len(ns) > 1 else b"") + (field(2, data) if len(data) else b"")
        if ver:
            m += _uvarint(3 << 3) + _uvarint(ver)
        if ns[0]:
            m += _uvarint(4 << 3) + _uvarint(ns[0])
        out += field(2, m)
    return out + field(3, b"BLOB")


def _compact_runs(ods):
    """[(start, end)] of the tx and the PFB shares of an ODS array: each namespace's run."""
    ns = _lib.NAMESPACE_SIZE
    out, at = [], 0
    for want in (TX_NAMESPACE, PFB_NAMESPACE):
        end = at
        while end < len(ods) and ods[end, :ns].tobytes() == want:
            end += 1
        out.append((at, end))
        at = end
    return out


def Deconstruct(x):
    """square.Deconstruct: the txs of a block out of its square, in order: the units of the tx
    namespace, then for every PFB unit the BlobTx of its inner tx and the blobs that start at its
    share indexes. x: a proof.TreeIndex (the compact shares are parsed and the blobs gathered on
    the device: txs_flat, blobs_flat), an rsmt2d.ExtendedDataSquare or an ODS array
    [k*k][512]."""
    from . import blob as _blob
    if hasattr(x, "txs_flat"):  # a proof.TreeIndex
        k = x.k
        runs = _blob.ods_ranges(k, 2, x.namespace_flat([TX_NAMESPACE, PFB_NAMESPACE]))
        got = x.txs(runs)
        for g in got:
            if isinstance(g, Exception):
                raise g
        txs, wrappers = got
        first_blob = max(runs[0][1], runs[1][1])
        blobs = x.blobs([(first_blob, k * k)], commitments=False)[0] if wrappers else []
    else:
        ods = np.frombuffer(b"".join(x.FlattenedODS()), np.uint8) if hasattr(x, "FlattenedODS") else np.asarray(x, np.uint8)
        ods = ods.reshape(-1, _lib.SHARE_SIZE)
        runs = _compact_runs(ods)
        txs, wrappers = (parse_compact_shares(ods[a:b]) for a, b in runs)
        first_blob = runs[1][1]
        blobs = _blob.parse_sparse_shares(ods[first_blob:]) if wrappers else []
        for b in blobs:
            b.index += first_blob
    if isinstance(blobs, Exception):
        raise blobs
    by_start = {b.index: b for b in blobs}
    out = list(txs)
    for i, w in enumerate(wrappers):
        got = unwrap_index_wrapper(w)
        if got is None:
            raise _lib.CelError(_lib.EINVAL, f"PayForBlob unit {i} is not an index wrapper")
        inner, idx = got
        missing = [s for s in idx if s not in by_start]
        if missing:
            raise _lib.CelError(_lib.EINVAL, f"PayForBlob unit {i}: no blob starts at share {missing[0]}")
        out.append(marshal_blob_tx(inner, [by_start[s] for s in idx]))
    return out
