"""Blobs by namespace, celestia-node's blob service over a square (go-square v1.1.0
parseSparseShares, inclusion.CreateCommitment).

  parse_sparse_shares(shares)        the parser on the host in numpy and Python: the checker of
                                     the device path, and the inverse of square.Construct's
                                     blob shares
  GetAll(index_or_eds, namespaces)   blob.GetAll: every blob of the namespaces
  Get(.., namespace, commitment)     blob.Get: the blob with that share commitment
  Included(.., namespace, commitment)
  GetProof(index, blob)              blob.GetProof: the NMT range proofs of the blob's shares

On a proof.TreeIndex the shares stay on the device: the namespace plan gives the rows and
ranges (cel_dev_namespace_plan), cel_namespace_ods_ranges one ODS range per namespace,
cel_dev_blobs_plan / cel_dev_blobs_emit the blobs and their commitments. An
rsmt2d.ExtendedDataSquare goes through its Blobs(), the host-memory form.

The parser, over the shares of a range in order: a share version other than 0 fails the range;
tail padding, primary reserved padding and namespace padding (a sequence start of length 0) are
skipped; any other sequence start opens a blob; a continuation appends its bytes 30 .. 511 to the
blob opened last, whatever its own namespace (go-square carries a FIXME on that), and fails the
range with none open; a blob closes at the next start or the range's end, where fewer bytes than
its length fail the range and more are trimmed.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CelError

NS = _lib.NAMESPACE_SIZE
SHARE = _lib.SHARE_SIZE
FIRST, CONT = 478, 482  # payload bytes of a first and of a continuation share
TAIL_PADDING_NS = b"\xff" * 28 + b"\xfe"
PRIMARY_RESERVED_PADDING_NS = bytes(28) + b"\xff"
MAX_PRIMARY_RESERVED_NS = PRIMARY_RESERVED_PADDING_NS  # tx, state roots, PayForBlob .. : compact shares

EVERSION, ENOSTART, ESHORT = _lib.BLOB_EVERSION, _lib.BLOB_ENOSTART, _lib.BLOB_ESHORT
_MESSAGES = {EVERSION: "unsupported share version", ENOSTART: "continuation share without a sequence start share",
             ESHORT: "the shares of a blob carry fewer bytes than its sequence length"}


class BlobRec(ctypes.Structure):
    """cel_blob_rec"""
    _fields_ = [("range", ctypes.c_uint32), ("start", ctypes.c_uint32), ("shares", ctypes.c_uint32),
                ("share_version", ctypes.c_uint32), ("len", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("data_off", ctypes.c_uint64), ("ns", ctypes.c_uint8 * 32)]


assert ctypes.sizeof(BlobRec) == 64


class BlobParseError(CelError):
    """A range that parseSparseShares rejects: kind is EVERSION, ENOSTART or ESHORT (the range
    status codes CEL_BLOB_E* of the C ABI)."""

    def __init__(self, kind, detail=""):
        super().__init__(_lib.EINVAL, _MESSAGES[kind] + (f": {detail}" if detail else ""))
        self.kind = kind


class BlobNotFound(CelError):
    """blob.Get: no blob of the namespace has the commitment (celestia-node's ErrBlobNotFound)."""

    def __init__(self):
        super().__init__(_lib.EINVAL, "blob: not found")


@dataclass
class Blob:
    namespace: bytes
    data: bytes
    share_version: int = 0
    commitment: bytes = None
    index: int = -1  # of the blob's first share, in the ODS (or in the list parsed)
    shares: int = 0  # shares the blob was found with


def sparse_shares_needed(n):
    return 0 if n == 0 else 1 if n <= FIRST else 1 + (n - FIRST + CONT - 1) // CONT


def parse_sparse_shares(shares):
    """go-square parseSparseShares over `shares` ([n][512] uint8, or a list of 512-byte strings):
    the blobs in order (commitment None, index the position of the start share), or
    BlobParseError with the first error."""
    a = np.asarray(shares, np.uint8) if not isinstance(shares, (list, tuple)) else \
        np.frombuffer(b"".join(bytes(s) for s in shares), np.uint8)
    a = a.reshape(-1, SHARE)
    seqs = []  # [namespace, length, [payloads], index, shares]
    for i in range(len(a)):
        sh = a[i]
        info = int(sh[NS])
        if info >> 1:
            raise BlobParseError(EVERSION, f"share {i} has version {info >> 1}")
        ns = sh[:NS].tobytes()
        start = info & 1
        length = int.from_bytes(sh[NS + 1:NS + 5].tobytes(), "big")
        if ns == TAIL_PADDING_NS or ns == PRIMARY_RESERVED_PADDING_NS or (start and length == 0):
            continue
        if start:
            seqs.append([ns, length, [sh[NS + 5:].tobytes()], i, 1])
        else:
            if not seqs:
                raise BlobParseError(ENOSTART, f"share {i}")
            seqs[-1][2].append(sh[NS + 1:].tobytes())
            seqs[-1][4] += 1
    out = []
    for ns, length, parts, i, n in seqs:
        if FIRST + CONT * (n - 1) < length:
            raise BlobParseError(ESHORT, f"the blob at share {i} declares {length} bytes and has {n} shares")
        out.append(Blob(ns, b"".join(parts)[:length], 0, None, i, n))
    return out


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def check_blob_namespaces(namespaces):
    """The namespaces as bytes; CelError(EINVAL) for one that is not 29 bytes or is reserved: the
    primary reserved ones (tx, PayForBlob, ...) hold compact shares, the secondary reserved ones
    padding and parity."""
    nss = [bytes(x) for x in namespaces]
    for ns in nss:
        if len(ns) != NS:
            raise CelError(_lib.EINVAL, f"a namespace is {NS} bytes")
        if ns <= MAX_PRIMARY_RESERVED_NS or ns[0] == 0xFF:
            raise CelError(_lib.EINVAL, f"namespace {ns.hex()} is reserved: it holds no blobs")
    return nss


def ods_ranges(k, n_namespaces, plan):
    """cel_namespace_ods_ranges over the entry arrays of a namespace plan (a dict with ns_idx,
    rows, starts, ends, kinds): [(start, end)] per namespace."""
    l = _lib.load()
    m = len(plan["rows"])
    arr = lambda key, t: np.ascontiguousarray(plan[key][:m], t) if m else np.zeros(1, t)
    a, b = np.zeros(max(n_namespaces, 1), np.uint32), np.zeros(max(n_namespaces, 1), np.uint32)
    st = l.cel_namespace_ods_ranges(k, n_namespaces, m, _p(arr("ns_idx", np.uint32)), _p(arr("rows", np.uint32)),
                                    _p(arr("starts", np.int32)), _p(arr("ends", np.int32)), _p(arr("kinds", np.uint8)),
                                    _p(a), _p(b))
    if st != _lib.OK:
        raise CelError(st, "the shares of a namespace are not one contiguous run of the original data square")
    return [(int(a[i]), int(b[i])) for i in range(n_namespaces)]


def blobs_from_records(recs, status, data, commitments, n_ranges):
    """Per range a list of Blob, or the BlobParseError of a failed range."""
    out = [[] if int(status[r]) == 0 else BlobParseError(int(status[r]), f"range {r}") for r in range(n_ranges)]
    for i, r in enumerate(recs):
        off = int(r.data_off)
        out[r.range].append(Blob(bytes(r.ns)[:NS], data[off:off + r.len].tobytes(), int(r.share_version),
                                 commitments[i].tobytes() if commitments is not None else None, int(r.start),
                                 int(r.shares)))
    return out


def _per_namespace(x, namespaces, commitments=True, threshold=64):
    nss = check_blob_namespaces(namespaces)
    if hasattr(x, "blobs"):  # a proof.TreeIndex
        ranges = ods_ranges(x.k, len(nss), x.namespace_flat(nss)) if nss else []
        return x.blobs(ranges, commitments=commitments, threshold=threshold)
    return x.Blobs(nss, commitments=commitments, threshold=threshold)


def GetAll(index_or_eds, namespaces, threshold=64):
    """blob.GetAll: the blobs of `namespaces` (29 bytes each) in the square, namespace after
    namespace in share order, each with its commitment and the ODS index of its first share.
    A reserved namespace raises CelError(EINVAL), shares that do not parse BlobParseError."""
    out = []
    for got in _per_namespace(index_or_eds, namespaces, threshold=threshold):
        if isinstance(got, Exception):
            raise got
        out += got
    return out


def Get(index_or_eds, namespace, commitment, threshold=64):
    """blob.Get: the blob of `namespace` whose share commitment is `commitment`; BlobNotFound."""
    for b in GetAll(index_or_eds, [namespace], threshold=threshold):
        if b.commitment == bytes(commitment):
            return b
    raise BlobNotFound()


def Included(index_or_eds, namespace, commitment, threshold=64):
    """blob.Included: is there a blob of `namespace` with that share commitment in the square?"""
    try:
        Get(index_or_eds, namespace, commitment, threshold=threshold)
        return True
    except BlobNotFound:
        return False


def GetProof(index, blob):
    """blob.GetProof: the NMT range proofs of the blob's shares, one per row of the ODS the blob
    touches, in row order, from the tree index (prove_ranges: no other device code). Proof i
    verifies the blob's shares of its row against index.row_roots[row]. -> [(row, NMTProof)]"""
    k = index.k
    first, last = blob.index, blob.index + sparse_shares_needed(len(blob.data)) - 1
    if not 0 <= first <= last < k * k:
        raise CelError(_lib.EINVAL, f"blob shares [{first}, {last + 1}) outside the {k}x{k} square")
    rows = list(range(first // k, last // k + 1))
    starts = [first % k if r == rows[0] else 0 for r in rows]
    ends = [last % k + 1 if r == rows[-1] else k for r in rows]
    return list(zip(rows, index.prove_ranges([0] * len(rows), rows, starts, ends)))
