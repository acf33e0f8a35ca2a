"""pkg/proof mirror: share inclusion proofs to the data root.

Construction (NewShareInclusionProofFromEDS, pkg/proof/proof.go:78-140, and
CreateShareToRowRootProofs, :147-202) reads the NMT nodes of the rows that hold the
shares from the device (cel_axis_trees: every node of those row trees, hashed on the
MI355X) and the row-root proofs from the device-built RFC-6962 tree over
rowRoots || colRoots (cel_dah_tree); cel_nmt_prove_range / cel_merkle_aunts pick the
proof nodes (nmt ProveRange, merkle.ProofsFromByteSlices). The reference instead
rebuilds every row tree on the CPU.

Verification (ShareProof.Validate / VerifyProof, share_proof.go:15-82; RowProof,
row_proof.go:12-48) mirrors the reference on the host: nmt VerifyInclusion (nmt
v0.22.0 proof.go [dep]: leaf hashing with the namespace prefix, completeness check,
computeRoot) and go-square merkle Proof.Verify (RFC-6962). Host-side hashing is the
reference's own choice for verifiers (a light client verifies on its CPU).

A node that reconstructs squares or validates many ShareProofs checks tens of thousands of
NMT proofs per square: VerifyInclusionBatch / VerifyShareProofs run those on the device
(cel_nmt_verify_batch), with the host verifier above as their checker.

A node that serves samples or many ShareProofs of one square builds them in batches:
TreeIndex keeps the square and every node of its 4k trees on the device
(cel_dev_tree_index_build) and cel_dev_prove_batch selects and packs the nodes of any number
of range proofs there; NewShareInclusionProofsBatch builds many ShareProofs that way.

A node that serves a namespace ("every share of namespace N in this block, and a proof that
none was left out": celestia-node GetSharesByNamespace) asks every row whose root range holds N
for nmt ProveNamespace: TreeIndex.namespace_rows finds those rows and the namespace's leaves in
them on the device, for any number of namespaces at once (cel_dev_namespace_plan /
cel_dev_namespace_prove), and VerifyNamespaceBatch checks such proofs there
(cel_nmt_verify_namespace_batch). NMTProof.VerifyNamespace / verify_namespace and
nmt_prove_namespace are their host mirrors. nmt is a dependency outside the reference tree, so
these rules are this project's restatement of nmt v0.22.0 (include/celestia_eds.h states them).

Wire format (proto/celestia/core/v1/proof/proof.proto:8-49, gogoproto-generated
pkg/proof/proof.pb.go): ShareProof / RowProof / NMTProof / Proof .Marshal() and
Unmarshal(bytes), the bytes QueryTxInclusionProof / QueryShareInclusionProof return
(pkg/proof/querier.go:53-63).
"""
import ctypes
import hashlib
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import CelError

NS = _lib.NAMESPACE_SIZE
NODE = _lib.NMT_NODE_SIZE
PARITY_NS = b"\xff" * NS


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------- hashing
def _sha(b):
    return hashlib.sha256(b).digest()


def _nmt_leaf(ns, data):
    """nmt HashLeaf: ns || ns || SHA256(0x00 || ns || data) (data without the ns prefix)."""
    return ns + ns + _sha(b"\x00" + ns + data)


def _nmt_node(left, right, nsz=NS):
    """nmt HashNode with IgnoreMaxNamespace (test/util/malicious/hasher.go:186-310 text copy):
    minNs = L.min; maxNs = L.max if R.min is the max namespace (0xFF * nsz) else
    max(L.max, R.max). Children must be ordered (L.max <= R.min). nmt is generic in the
    namespace size: the app uses 29 bytes, nsz follows the verified namespace."""
    lmin, lmax, rmin, rmax = left[:nsz], left[nsz:2 * nsz], right[:nsz], right[nsz:2 * nsz]
    if lmax > rmin:
        raise ValueError("unordered nmt children")
    mx = lmax if rmin == b"\xff" * nsz else (rmax if rmax > lmax else lmax)
    return lmin + mx + _sha(b"\x01" + left + right)


def _split_point(n):
    """largest power of two strictly less than n (n >= 2)"""
    k = 1
    while k * 2 < n:
        k *= 2
    return k


def _rfc_leaf(item):
    return _sha(b"\x00" + item)


def _rfc_inner(left, right):
    return _sha(b"\x01" + left + right)


def _compute_root(start, end, hashes, nodes, nsz):
    """nmt Proof.computeRoot over the leaf hashes of [start, end) and the proof nodes, then the
    surplus nodes as right siblings at the top. ValueError on unordered children."""
    state = {"nodes": list(nodes), "leaves": list(hashes)}

    def pop(key):
        lst = state[key]
        if not lst:
            return None
        v = lst[0]
        state[key] = lst[1:]
        return v

    def compute(s, e):
        if e - s == 1:
            return pop("leaves") if start <= s < end else pop("nodes")
        if e <= start or s >= end:
            return pop("nodes")
        k = _split_point(e - s)
        lh = compute(s, s + k)
        rh = compute(s + k, e)
        if rh is None:
            return lh
        return _nmt_node(lh, rh, nsz)

    est = max(_split_point(end) * 2 if end > 1 else 1, 1)
    h = compute(0, est)
    for n in state["nodes"]:
        h = _nmt_node(h, n, nsz)
    return h


NS_INCLUSION, NS_ABSENCE = _lib.NS_INCLUSION, _lib.NS_ABSENCE


def verify_namespace(start, end, kind, namespace, leaves, nodes, root):
    """nmt Proof.VerifyNamespace in the flat form the device takes (cel_nmt_verify_namespace_batch):
    `leaves` are whole shares, and an absence proof's leaf hash is the last of `nodes`. Every
    input is untrusted; a malformed proof is False.

    empty proof  inclusion, start == end, no nodes, no leaves: True iff the namespace lies
                 outside the root's range. Any other proof with start == end is False.
    inclusion    0 <= start < end, end - start leaves, each share starting with the namespace
                 (celestia-node hands nmt share[:29] || share; nmt checks that prefix).
    absence      end == start + 1, no leaves, at least popcount(start) + 1 nodes; the leaf hash
                 has min <= max and namespace < min, and is the single leaf folded.
    both         of the nodes, the first popcount(start) are the left siblings of the range and
                 each must end below the namespace; the others are right siblings and each must
                 begin above it (completeness); the folded node equals the root."""
    namespace, root = bytes(namespace), bytes(root)
    nsz = len(namespace)
    nodes = [bytes(x) for x in nodes]
    if kind not in (NS_INCLUSION, NS_ABSENCE):
        return False
    if len(root) != 2 * nsz + 32 or any(len(x) != 2 * nsz + 32 for x in nodes):
        return False
    if start == end:
        if kind != NS_INCLUSION or nodes or leaves:
            return False
        return namespace < root[:nsz] or namespace > root[nsz:2 * nsz]
    if start < 0 or end < start:
        return False
    nl = bin(start).count("1")
    if kind == NS_INCLUSION:
        if len(leaves) != end - start or len(nodes) < nl:
            return False
        if any(bytes(x[:nsz]) != namespace for x in leaves):
            return False
        hashes = [_nmt_leaf(namespace, bytes(x)) for x in leaves]
    else:
        if end != start + 1 or leaves or len(nodes) < nl + 1:
            return False
        leaf_hash, nodes = nodes[-1], nodes[:-1]
        if leaf_hash[:nsz] > leaf_hash[nsz:2 * nsz] or not namespace < leaf_hash[:nsz]:
            return False
        hashes = [leaf_hash]
    if any(not x[nsz:2 * nsz] < namespace for x in nodes[:nl]):
        return False
    if any(not x[:nsz] > namespace for x in nodes[nl:]):
        return False
    try:
        return _compute_root(start, end, hashes, nodes, nsz) == root
    except (ValueError, TypeError):  # unordered children; a node missing
        return False


# ---------------------------------------------------------------- proto3 wire
# gogoproto's generated Marshal / Unmarshal for these four messages (proof.pb.go):
# fields in ascending number; scalars and singular bytes omitted when zero / empty;
# every element of a repeated field written (empty ones too); a set sub-message written
# even when empty; negative int32 / int64 as 10-byte two's-complement varints. Unmarshal
# skips unknown fields by wire type and rejects a known field with the wrong wire type.
def _uvarint(n):
    n &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def _key(field, wt):
    return _uvarint(field << 3 | wt)


def _w_varint(field, v):
    return _key(field, 0) + _uvarint(v) if v else b""


def _w_bytes(field, b, always=False):
    b = bytes(b) if b is not None else b""
    return _key(field, 2) + _uvarint(len(b)) + b if (b or always) else b""


class _Reader:
    def __init__(self, buf, msg):
        self.buf, self.i, self.msg = bytes(buf), 0, msg

    def _err(self, what):
        return CelError(_lib.EINVAL, f"proto: {self.msg}: {what}")

    def uvarint(self):
        v, shift = 0, 0
        while True:
            if self.i >= len(self.buf):
                raise self._err("unexpected EOF")
            if shift >= 64:
                raise self._err("integer overflow")
            b = self.buf[self.i]
            self.i += 1
            v |= (b & 0x7F) << shift
            if not b & 0x80:
                return v & ((1 << 64) - 1)
            shift += 7

    def fields(self):
        """Yield (field number, wire type) until the end; the caller reads the value."""
        while self.i < len(self.buf):
            key = self.uvarint()
            field, wt = key >> 3, key & 7
            if field <= 0 or key >> 3 > 0x7FFFFFFF:
                raise self._err(f"illegal tag {field} (wire type {wt})")
            yield field, wt

    def lendelim(self):
        n = self.uvarint()
        if n > len(self.buf) - self.i:
            raise self._err("unexpected EOF")
        b = self.buf[self.i:self.i + n]
        self.i += n
        return b

    def skip(self, wt, depth=0):
        if wt == 0:
            self.uvarint()
        elif wt == 1:
            self._need(8)
        elif wt == 2:
            self.lendelim()
        elif wt == 5:
            self._need(4)
        elif wt == 3:  # start group: skip to the matching end group
            if depth > 100:
                raise self._err("nesting too deep")
            while True:
                if self.i >= len(self.buf):
                    raise self._err("unexpected EOF")
                key = self.uvarint()
                if key & 7 == 4:
                    return
                self.skip(key & 7, depth + 1)
        else:  # 4 (end group outside a group), 6, 7
            raise self._err(f"illegal wireType {wt}")

    def _need(self, n):
        if n > len(self.buf) - self.i:
            raise self._err("unexpected EOF")
        self.i += n

    def want(self, wt, need, name):
        if wt != need:
            raise self._err(f"wrong wireType = {wt} for field {name}")


def _int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _int64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


# -------------------------------------------------------------------- types
@dataclass
class NMTProof:
    """proof.NMTProof (proto/celestia/core/v1/proof/proof.proto): nmt range proof."""
    Start: int
    End: int
    Nodes: List[bytes]
    LeafHash: Optional[bytes] = None

    def Marshal(self):
        out = _w_varint(1, self.Start) + _w_varint(2, self.End)
        for n in self.Nodes:
            out += _w_bytes(3, n, always=True)
        return out + _w_bytes(4, self.LeafHash)

    @classmethod
    def Unmarshal(cls, buf):
        m, r = cls(0, 0, []), _Reader(buf, "NMTProof")
        for f, wt in r.fields():
            if f == 1:
                r.want(wt, 0, "Start")
                m.Start = _int32(r.uvarint())
            elif f == 2:
                r.want(wt, 0, "End")
                m.End = _int32(r.uvarint())
            elif f == 3:
                r.want(wt, 2, "Nodes")
                m.Nodes.append(r.lendelim())
            elif f == 4:
                r.want(wt, 2, "LeafHash")
                m.LeafHash = r.lendelim()
            else:
                r.skip(wt)
        return m

    def VerifyInclusion(self, namespace, leaves, root):
        """nmt Proof.VerifyInclusion: recompute the root from the leaves (all in `namespace`,
        given without the namespace prefix) and the proof nodes. Like nmt, no completeness
        check: the leaves may be a subset of the namespace's leaves (VerifyNamespace is
        the completeness-checking form)."""
        start, end = self.Start, self.End
        nsz = len(namespace)
        if start < 0 or end <= start or len(leaves) != end - start:
            return False
        hashes = [_nmt_leaf(namespace, d) for d in leaves]
        try:
            return _compute_root(start, end, hashes, self.Nodes, nsz) == root
        except ValueError:
            return False

    def IsOfAbsence(self):
        """nmt Proof.IsOfAbsence: the proof carries a leaf hash."""
        return bool(self.LeafHash)

    def IsEmptyProof(self):
        """nmt Proof.IsEmptyProof: the proof of a namespace outside the tree's range."""
        return self.Start == self.End and not self.Nodes and not self.LeafHash

    def VerifyNamespace(self, namespace, leaves, root):
        """nmt Proof.VerifyNamespace: `leaves` (whole 512-byte shares) are all the leaves of
        `namespace` under `root`, none left out; or, for an absence proof (LeafHash set, no
        leaves) and for the empty proof, the tree holds none. verify_namespace states the rules."""
        absent = self.IsOfAbsence()
        nodes = list(self.Nodes) + ([bytes(self.LeafHash)] if absent else [])
        return verify_namespace(self.Start, self.End, NS_ABSENCE if absent else NS_INCLUSION, namespace, leaves, nodes,
                                root)


@dataclass
class Proof:
    """merkle.Proof (RFC-6962) of one item among Total."""
    Total: int
    Index: int
    LeafHash: bytes
    Aunts: List[bytes]

    def Marshal(self):
        out = _w_varint(1, self.Total) + _w_varint(2, self.Index) + _w_bytes(3, self.LeafHash)
        for a in self.Aunts:
            out += _w_bytes(4, a, always=True)
        return out

    @classmethod
    def Unmarshal(cls, buf):
        m, r = cls(0, 0, b"", []), _Reader(buf, "Proof")
        for f, wt in r.fields():
            if f == 1:
                r.want(wt, 0, "Total")
                m.Total = _int64(r.uvarint())
            elif f == 2:
                r.want(wt, 0, "Index")
                m.Index = _int64(r.uvarint())
            elif f == 3:
                r.want(wt, 2, "LeafHash")
                m.LeafHash = r.lendelim()
            elif f == 4:
                r.want(wt, 2, "Aunts")
                m.Aunts.append(r.lendelim())
            else:
                r.skip(wt)
        return m

    def _compute(self, index, total, leaf, aunts):
        if total == 1:
            return leaf if not aunts else None
        if not aunts:
            return None
        k = _split_point(total)
        if index < k:
            lh = self._compute(index, k, leaf, aunts[:-1])
            return None if lh is None else _rfc_inner(lh, aunts[-1])
        rh = self._compute(index - k, total - k, leaf, aunts[:-1])
        return None if rh is None else _rfc_inner(aunts[-1], rh)

    def Verify(self, root, leaf):
        """go-square merkle Proof.Verify: error (CelError) unless leaf is item Index of root."""
        if self.Total < 0 or self.Index < 0:
            raise CelError(_lib.EINVAL, "proof total and index must be non-negative")
        if _rfc_leaf(leaf) != self.LeafHash:
            raise CelError(_lib.EINVAL, "invalid leaf hash")
        if self._compute(self.Index, self.Total, self.LeafHash, list(self.Aunts)) != root:
            raise CelError(_lib.EINVAL, "invalid root hash")


@dataclass
class RowProof:
    RowRoots: List[bytes]
    Proofs: List[Proof]
    StartRow: int
    EndRow: int
    Root: bytes = b""  # proof.proto field 3; NewShareInclusionProofFromEDS leaves it empty

    def Marshal(self):
        out = b"".join(_w_bytes(1, r, always=True) for r in self.RowRoots)
        for p in self.Proofs:
            out += _w_bytes(2, p.Marshal(), always=True)
        return out + _w_bytes(3, self.Root) + _w_varint(4, self.StartRow) + _w_varint(5, self.EndRow)

    @classmethod
    def Unmarshal(cls, buf):
        m, r = cls([], [], 0, 0), _Reader(buf, "RowProof")
        for f, wt in r.fields():
            if f == 1:
                r.want(wt, 2, "RowRoots")
                m.RowRoots.append(r.lendelim())
            elif f == 2:
                r.want(wt, 2, "Proofs")
                m.Proofs.append(Proof.Unmarshal(r.lendelim()))
            elif f == 3:
                r.want(wt, 2, "Root")
                m.Root = r.lendelim()
            elif f == 4:
                r.want(wt, 0, "StartRow")
                m.StartRow = r.uvarint() & 0xFFFFFFFF
            elif f == 5:
                r.want(wt, 0, "EndRow")
                m.EndRow = r.uvarint() & 0xFFFFFFFF
            else:
                r.skip(wt)
        return m

    def Validate(self, root):
        if self.EndRow - self.StartRow + 1 != len(self.RowRoots):
            raise CelError(_lib.EINVAL, f"the number of rows {self.EndRow - self.StartRow + 1} must equal the "
                                        f"number of row roots {len(self.RowRoots)}")
        if len(self.Proofs) != len(self.RowRoots):
            raise CelError(_lib.EINVAL, f"the number of proofs {len(self.Proofs)} must equal the number of row "
                                        f"roots {len(self.RowRoots)}")
        if not self.VerifyProof(root):
            raise CelError(_lib.EINVAL, "row proof failed to verify")

    def VerifyProof(self, root):
        for p, r in zip(self.Proofs, self.RowRoots):
            try:
                p.Verify(root, r)
            except CelError:
                return False
        return True


@dataclass
class ShareProof:
    Data: List[bytes]
    ShareProofs: List[NMTProof]
    NamespaceId: bytes
    RowProof: Optional[RowProof]
    NamespaceVersion: int = 0

    def Marshal(self):
        """gogoproto ShareProof.Marshal (proof.pb.go): the bytes of the ABCI proof queries."""
        out = b"".join(_w_bytes(1, d, always=True) for d in self.Data)
        for p in self.ShareProofs:
            out += _w_bytes(2, p.Marshal(), always=True)
        out += _w_bytes(3, self.NamespaceId)
        if self.RowProof is not None:
            out += _w_bytes(4, self.RowProof.Marshal(), always=True)
        return out + _w_varint(5, self.NamespaceVersion)

    @classmethod
    def Unmarshal(cls, buf):
        m, r = cls([], [], b"", None), _Reader(buf, "ShareProof")
        for f, wt in r.fields():
            if f == 1:
                r.want(wt, 2, "Data")
                m.Data.append(r.lendelim())
            elif f == 2:
                r.want(wt, 2, "ShareProofs")
                m.ShareProofs.append(NMTProof.Unmarshal(r.lendelim()))
            elif f == 3:
                r.want(wt, 2, "NamespaceId")
                m.NamespaceId = r.lendelim()
            elif f == 4:
                r.want(wt, 2, "RowProof")
                m.RowProof = RowProof.Unmarshal(r.lendelim())
            elif f == 5:
                r.want(wt, 0, "NamespaceVersion")
                m.NamespaceVersion = r.uvarint() & 0xFFFFFFFF
            else:
                r.skip(wt)
        return m

    def Validate(self, root):
        if self.RowProof is None:  # the reference dereferences a nil *RowProof (a panic)
            raise CelError(_lib.EINVAL, "share proof has no row proof")
        if not self.Data:
            raise CelError(_lib.EINVAL, "empty share proof")
        n = sum(p.End - p.Start for p in self.ShareProofs)
        if len(self.ShareProofs) != len(self.RowProof.RowRoots):
            raise CelError(_lib.EINVAL, f"the number of share proofs {len(self.ShareProofs)} must equal the "
                                        f"number of row roots {len(self.RowProof.RowRoots)}")
        if len(self.Data) != n:
            raise CelError(_lib.EINVAL, f"the number of shares {len(self.Data)} must equal the number of shares "
                                        f"in share proofs {n}")
        for p in self.ShareProofs:
            if p.Start < 0:
                raise CelError(_lib.EINVAL, "proof index cannot be negative")
            if p.End - p.Start <= 0:
                raise CelError(_lib.EINVAL, "proof total must be positive")
        self.RowProof.Validate(root)
        if not self.VerifyProof():
            raise CelError(_lib.EINVAL, "share proof failed to verify")

    def VerifyProof(self):
        if self.NamespaceVersion > 255:
            return False
        ns = bytes([self.NamespaceVersion]) + bytes(self.NamespaceId)
        cursor = 0
        for i, p in enumerate(self.ShareProofs):
            used = p.End - p.Start
            if not p.VerifyInclusion(ns, self.Data[cursor:cursor + used], self.RowProof.RowRoots[i]):
                return False
            cursor += used
        return True


# ---------------------------------------------------------------- construction
def axis_trees(eds, axis, first, count, ctx=None):
    """All nodes of the NMTs of EDS rows (axis 0) or columns (1) [first, first+count):
    array [count][4k-1][90] (level-major from the leaves), hashed on the device."""
    ctx = ctx or eds.ctx
    cells = np.ascontiguousarray(eds.cells)
    W = cells.shape[0]
    out = np.zeros((count, 2 * W - 1, NODE), np.uint8)
    ctx.check(ctx.lib.cel_axis_trees(ctx.handle, _p(cells), W // 2, _lib.SHARE_SIZE, axis, first, count, _p(out)))
    return out


def dah_tree(eds, ctx=None):
    """RFC-6962 levels over rowRoots || colRoots: array [4w-1][32], root last."""
    ctx = ctx or eds.ctx
    rr = np.ascontiguousarray(np.frombuffer(b"".join(eds.RowRoots()), np.uint8))
    cr = np.ascontiguousarray(np.frombuffer(b"".join(eds.ColRoots()), np.uint8))
    w = len(eds.RowRoots())
    out = np.zeros((4 * w - 1, 32), np.uint8)
    ctx.check(ctx.lib.cel_dah_tree(ctx.handle, _p(rr), _p(cr), w, _p(out)))
    return out


def nmt_prove_range(tree, start, end):
    """nmt ProveRange(start, end) over one tree of axis_trees(): the proof nodes."""
    l = _lib.load()
    tree = np.ascontiguousarray(tree)
    nleaves = (tree.shape[0] + 1) // 2
    cnt = ctypes.c_uint32()
    out = np.zeros((64, NODE), np.uint8)
    st = l.cel_nmt_prove_range(_p(tree), nleaves, start, end, _p(out), ctypes.byref(cnt))
    if st != _lib.OK:
        raise CelError(st, f"invalid proof range [{start}, {end}) over {nleaves} leaves")
    return [out[i].tobytes() for i in range(cnt.value)]


def nmt_prove_namespace(tree, nleaves, namespace):
    """nmt ProveNamespace(namespace) on one tree of axis_trees() (nleaves leaves, a power of two),
    as celestia-node asks it of a row: None when the namespace lies outside the root's range (or
    above every leaf); the inclusion proof of all its leaves [lt, le); or, when the tree holds
    none, the absence proof: ProveRange(lt, lt + 1) with LeafHash = the leaf that follows where the
    namespace would be. lt / le count the leaves whose namespace is below / not above it."""
    namespace = bytes(namespace)
    tree = np.ascontiguousarray(tree)
    root = tree[-1].tobytes()
    if not root[:NS] <= namespace <= root[NS:2 * NS]:
        return None
    mins = [tree[i, :NS].tobytes() for i in range(nleaves)]
    lt = sum(1 for m in mins if m < namespace)
    le = sum(1 for m in mins if m <= namespace)
    if lt >= nleaves:
        return None
    if le > lt:
        return NMTProof(Start=lt, End=le, Nodes=nmt_prove_range(tree, lt, le))
    return NMTProof(Start=lt, End=lt + 1, Nodes=nmt_prove_range(tree, lt, lt + 1), LeafHash=tree[lt].tobytes())


def merkle_aunts(levels, n, index):
    l = _lib.load()
    levels = np.ascontiguousarray(levels)
    cnt = ctypes.c_uint32()
    out = np.zeros((64, 32), np.uint8)
    st = l.cel_merkle_aunts(_p(levels), n, index, _p(out), ctypes.byref(cnt))
    if st != _lib.OK:
        raise CelError(st, f"invalid merkle index {index} of {n}")
    return [out[i].tobytes() for i in range(cnt.value)]


def CreateShareToRowRootProofs(eds, start_row, end_row, start_leaf, end_leaf):
    """pkg/proof/proof.go:147-202 on device-built trees: per row, the nmt range proof of
    the selected shares and the raw shares."""
    k = eds.Width() // 2
    trees = axis_trees(eds, 0, start_row, end_row - start_row + 1)
    share_proofs, raw = [], []
    roots = eds.RowRoots()
    for i, r in enumerate(range(start_row, end_row + 1)):
        if trees[i, -1].tobytes() != roots[r]:
            raise CelError(_lib.EINVAL, "eds row root is different than tree root")
        s = start_leaf if i == 0 else 0
        e = end_leaf if r == end_row else k - 1  # ODS part of the row (proof.go:180-183, squareSize = k)
        raw += [eds.GetCell(r, c) for c in range(s, e + 1)]
        share_proofs.append(NMTProof(Start=s, End=e + 1, Nodes=nmt_prove_range(trees[i], s, e + 1)))
    return share_proofs, raw


def NewShareInclusionProofFromEDS(eds, namespace, share_start, share_end):
    """pkg/proof/proof.go:78-140: ShareProof of ODS shares [share_start, share_end) (all in
    `namespace`, 29 bytes) to the data root of `eds`."""
    k = eds.Width() // 2
    if not 0 <= share_start < share_end <= k * k:
        raise CelError(_lib.EINVAL, f"share range [{share_start}, {share_end}) outside the {k}x{k} square")
    start_row, end_row = share_start // k, (share_end - 1) // k
    start_leaf, end_leaf = share_start % k, (share_end - 1) % k
    levels = dah_tree(eds)
    n = 4 * k
    roots = eds.RowRoots()
    proofs = []
    for r in range(start_row, end_row + 1):
        proofs.append(Proof(Total=n, Index=r, LeafHash=levels[r].tobytes(), Aunts=merkle_aunts(levels, n, r)))
    share_proofs, raw = CreateShareToRowRootProofs(eds, start_row, end_row, start_leaf, end_leaf)
    ns = bytes(namespace)
    return ShareProof(Data=raw, ShareProofs=share_proofs, NamespaceId=ns[1:], NamespaceVersion=ns[0],
                      RowProof=RowProof(RowRoots=[roots[r] for r in range(start_row, end_row + 1)], Proofs=proofs,
                                        StartRow=start_row, EndRow=end_row))


def NewShareInclusionProof(ods_shares, namespace, share_start, share_end):
    """pkg/proof/proof.go:64-76: extend the ODS on the device, then prove."""
    from . import da
    return NewShareInclusionProofFromEDS(da.ExtendShares(ods_shares), namespace, share_start, share_end)


# ------------------------------------------------------- batched construction
def prove_offsets(k, starts, ends):
    """cel_prove_offsets: (leaf_off, node_off), the prefix sums of each range's leaves and of
    its ProveRange node count over 2k leaves. A bad range raises CelError naming the proof."""
    l = _lib.load()
    starts, ends = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(ends, np.int32)
    n = len(starts)
    leaf_off, node_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    st = l.cel_prove_offsets(k, n, _p(starts), _p(ends), _p(leaf_off), _p(node_off))
    if st != _lib.OK:
        raise CelError(st, l.cel_prove_last_error().decode())
    return leaf_off, node_off


class TreeIndex:
    """A square resident on the device with every node of its 4k row and column NMTs
    (cel_dev_tree_index_build), for proofs in batches (cel_dev_prove_batch): one upload and
    one hashing pass serve any number of range proofs and samples, where axis_trees +
    nmt_prove_range download every node and pick one proof per call. `eds`: an
    ExtendedDataSquare or a (2k, 2k, 512) uint8 array, any cells. PyTorch holds the device
    memory and the stream, as in device.py."""

    def __init__(self, eds, ctx=None, order_check=False):
        import torch
        cells = np.ascontiguousarray(getattr(eds, "cells", eds), dtype=np.uint8)
        if cells.ndim != 3 or cells.shape[0] != cells.shape[1] or cells.shape[2] != _lib.SHARE_SIZE:
            raise CelError(_lib.EINVAL, f"need a (2k, 2k, {_lib.SHARE_SIZE}) square, got {cells.shape}")
        self.ctx = ctx or getattr(eds, "_ctx", None) or _lib.default_context()
        self.cells = cells
        self.w = cells.shape[0]
        self.k = self.w // 2
        self._torch = torch
        self._dev = torch.device("cuda", self.ctx.device)
        self._stream = torch.cuda.Stream(device=self._dev)
        c, w = self.ctx, self.w
        size = c.lib.cel_dev_tree_index_size(self.k)
        if size == 0 or 2 * self.k != w:
            raise CelError(_lib.ENOTPOW2, f"square width is not a power of 2: got {w / 2:g}")
        with torch.cuda.stream(self._stream):
            self.d_eds = torch.as_tensor(cells).to(self._dev)
            self.d_index = torch.empty((size,), dtype=torch.uint8, device=self._dev)
            d_roots = torch.empty((2, w, NODE), dtype=torch.uint8, device=self._dev)
            d_dah = torch.empty((32,), dtype=torch.uint8, device=self._dev)
            status = ctypes.c_int32(-1)
            c.check(c.lib.cel_dev_tree_index_build(c.handle, self._ptr(self.d_eds), self.k, self._ptr(self.d_index),
                                                   self._ptr(d_roots[0]), self._ptr(d_roots[1]), self._ptr(d_dah),
                                                   ctypes.byref(status), _lib.FLAG_ORDER_CHECK if order_check else 0,
                                                   self._stream_ptr()))
            self._stream.synchronize()
            roots = d_roots.cpu().numpy()
            self.dah = d_dah.cpu().numpy().tobytes()
        self.d_row_roots, self.d_col_roots = d_roots[0], d_roots[1]
        if status.value != _lib.OK:
            raise CelError(status.value, "invalid push order: a namespace is smaller than the previous one")
        self.row_roots = [r.tobytes() for r in roots[0]]
        self.col_roots = [r.tobytes() for r in roots[1]]

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def _stream_ptr(self):
        return ctypes.c_void_p(self._stream.cuda_stream)

    def prove_flat(self, axes, index, starts, ends, shares=True):
        """One cel_dev_prove_batch: (leaves [total leaves][512] or None, nodes [total nodes][90],
        leaf_off, node_off) as host arrays, the flat layout of cel_nmt_verify_batch."""
        torch, c = self._torch, self.ctx
        axes, index = np.ascontiguousarray(axes, np.uint8), np.ascontiguousarray(index, np.uint32)
        starts, ends = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(ends, np.int32)
        n = len(axes)
        if not (len(index) == len(starts) == len(ends) == n):
            raise CelError(_lib.EINVAL, "axes, index, starts and ends differ in number")
        leaf_off, node_off = prove_offsets(self.k, starts, ends)
        tl, tn = int(leaf_off[-1]), int(node_off[-1])
        with torch.cuda.stream(self._stream):
            d_leaves = torch.empty((tl, _lib.SHARE_SIZE), dtype=torch.uint8, device=self._dev) if shares else None
            d_nodes = torch.empty((max(tn, 1), NODE), dtype=torch.uint8, device=self._dev)  # whole-tree ranges: none
            d_work = torch.empty((c.lib.cel_dev_prove_workspace_size(n),), dtype=torch.uint8, device=self._dev)
            c.check(c.lib.cel_dev_prove_batch(c.handle, self._ptr(self.d_eds), self._ptr(self.d_index), self.k, n,
                                              _p(axes), _p(index), _p(starts), _p(ends),
                                              self._ptr(d_leaves) if shares else None, self._ptr(d_nodes),
                                              self._ptr(d_work), self._stream_ptr()))
            self._stream.synchronize()
            return (d_leaves.cpu().numpy() if shares else None), d_nodes[:tn].cpu().numpy(), leaf_off, node_off

    def prove_ranges(self, axes, index, starts, ends, shares=False):
        """nmt ProveRange(starts[i], ends[i]) on row (axes[i] = 0) or column (1) index[i]: a list of
        NMTProof; with shares=True also the list of each proof's raw shares."""
        leaves, nodes, leaf_off, node_off = self.prove_flat(axes, index, starts, ends, shares=shares)
        proofs = [NMTProof(Start=int(s), End=int(e), Nodes=[nodes[j].tobytes() for j in range(int(a), int(b))])
                  for s, e, a, b in zip(starts, ends, node_off[:-1], node_off[1:])]
        if not shares:
            return proofs
        return proofs, [[leaves[j].tobytes() for j in range(int(a), int(b))]
                        for a, b in zip(leaf_off[:-1], leaf_off[1:])]

    def prove_samples(self, coords_axes):
        """Samples (row, col, axis) -> (row, col, axis, share, nodes), RepairFromSamples' format:
        the cell proved at leaf col of row `row` (axis 0) or at leaf row of column `col` (1)."""
        coords = [(int(r), int(c), int(a)) for r, c, a in coords_axes]
        for i, (r, c, a) in enumerate(coords):
            if not (0 <= r < self.w and 0 <= c < self.w and 0 <= a <= 1):
                raise CelError(_lib.EINVAL, f"sample {i}: cell ({r}, {c}) axis {a} outside the square of width {self.w}")
        index = [c if a else r for r, c, a in coords]
        starts = [r if a else c for r, c, a in coords]
        leaves, nodes, _, node_off = self.prove_flat([a for _, _, a in coords], index, starts,
                                                     [s + 1 for s in starts])
        return [(r, c, a, leaves[i].tobytes(), [nodes[j].tobytes() for j in range(int(node_off[i]), int(node_off[i + 1]))])
                for i, (r, c, a) in enumerate(coords)]


    def namespace_flat(self, namespaces):
        """cel_dev_namespace_plan + cel_dev_namespace_prove for `namespaces` (29 bytes each): a dict
        of the entries' host arrays (ns_idx, rows, starts, ends, kinds, leaf_off, node_off) with
        leaves [total shares][512] and nodes [total nodes][90], the flat layout of
        cel_nmt_verify_namespace_batch."""
        torch, c = self._torch, self.ctx
        nss = [bytes(x) for x in namespaces]
        n = len(nss)
        if any(len(x) != NS for x in nss):
            raise CelError(_lib.EINVAL, f"a namespace is {NS} bytes")
        ns = np.frombuffer(b"".join(nss) or b"\0", np.uint8).copy()
        cnt = ctypes.c_uint64(0)
        with torch.cuda.stream(self._stream):
            d_work = torch.empty((max(c.lib.cel_dev_namespace_workspace_size(self.k, n), 16),), dtype=torch.uint8,
                                 device=self._dev)
            cap = n * self.w
            out = dict(ns_idx=np.zeros(cap, np.uint32), rows=np.zeros(cap, np.uint32), starts=np.zeros(cap, np.int32),
                       ends=np.zeros(cap, np.int32), kinds=np.zeros(cap, np.uint8), leaf_off=np.zeros(cap + 1, np.uint64),
                       node_off=np.zeros(cap + 1, np.uint64))
            c.check(c.lib.cel_dev_namespace_plan(c.handle, self._ptr(self.d_index), self.k, n, _p(ns), cap,
                                                 _p(out["ns_idx"]), _p(out["rows"]), _p(out["starts"]), _p(out["ends"]),
                                                 _p(out["kinds"]), _p(out["leaf_off"]), _p(out["node_off"]),
                                                 ctypes.byref(cnt), self._ptr(d_work), self._stream_ptr()))
            m = cnt.value
            out = {key: v[:m + 1] if key.endswith("_off") else v[:m] for key, v in out.items()}
            tl, tn = int(out["leaf_off"][-1]), int(out["node_off"][-1])
            d_leaves = torch.empty((max(tl, 1), _lib.SHARE_SIZE), dtype=torch.uint8, device=self._dev)
            d_nodes = torch.empty((max(tn, 1), NODE), dtype=torch.uint8, device=self._dev)
            c.check(c.lib.cel_dev_namespace_prove(c.handle, self._ptr(self.d_eds), self._ptr(self.d_index), self.k, m,
                                                  self._ptr(d_leaves), self._ptr(d_nodes), self._ptr(d_work),
                                                  self._stream_ptr()))
            self._stream.synchronize()
            out["leaves"], out["nodes"] = d_leaves[:tl].cpu().numpy(), d_nodes[:tn].cpu().numpy()
        return out

    def namespace_rows(self, namespaces):
        """nmt ProveNamespace of every namespace on every row whose root range holds it: per
        namespace a list of (row, NMTProof, shares), rows ascending. An inclusion proof comes with
        the namespace's shares of that row; an absence proof has LeafHash set and no shares. A
        namespace that no row's range holds gives an empty list."""
        f = self.namespace_flat(namespaces)
        out = [[] for _ in namespaces]
        for e in range(len(f["rows"])):
            a, b = int(f["node_off"][e]), int(f["node_off"][e + 1])
            nodes = [f["nodes"][j].tobytes() for j in range(a, b)]
            absent = int(f["kinds"][e]) == NS_ABSENCE
            p = NMTProof(Start=int(f["starts"][e]), End=int(f["ends"][e]), Nodes=nodes[:-1] if absent else nodes,
                         LeafHash=nodes[-1] if absent else None)
            shares = [f["leaves"][j].tobytes() for j in range(int(f["leaf_off"][e]), int(f["leaf_off"][e + 1]))]
            out[int(f["ns_idx"][e])].append((int(f["rows"][e]), p, shares))
        return out

    def blobs_flat(self, ranges, commitments=True, threshold=64):
        """cel_dev_blobs_plan + cel_dev_blobs_emit over `ranges` ((start, end) in row-major ODS
        index) of the resident square: (records, range status, data, commitments [n][32] or
        None) as host arrays; blob i's bytes are data[rec.data_off : rec.data_off + rec.len]."""
        from . import blob as _blob
        torch, c = self._torch, self.ctx
        n = len(ranges)
        starts = np.array([r[0] for r in ranges] or [0], np.uint32)
        ends = np.array([r[1] for r in ranges] or [0], np.uint32)
        if any(not (0 <= int(a) <= int(b) <= self.k * self.k) for a, b in ranges):
            raise CelError(_lib.EINVAL, f"a range is outside the {self.k}x{self.k} square or has start > end")
        total = int(sum(int(b) - int(a) for a, b in ranges))
        status = np.zeros(max(n, 1), np.uint32)
        cnt, tb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with torch.cuda.stream(self._stream):
            d_work = torch.empty((max(c.lib.cel_dev_blobs_workspace_size(total, n), 16),), dtype=torch.uint8,
                                 device=self._dev)
            cap = max(total, 1)  # a blob has at least one share
            recs = (_blob.BlobRec * cap)()
            c.check(c.lib.cel_dev_blobs_plan(c.handle, self._ptr(self.d_eds), self.k, n, _p(starts), _p(ends), cap,
                                             recs, _p(status), ctypes.byref(cnt), ctypes.byref(tb), self._ptr(d_work),
                                             self._stream_ptr()))
            m, nbytes = cnt.value, tb.value
            recs = list(recs[:m])
            d_data = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=self._dev)
            d_com = d_cwork = None
            if commitments and m:
                d_com = torch.empty((m, 32), dtype=torch.uint8, device=self._dev)
                size = c.lib.cel_dev_commitments_workspace_size(sum(r.shares for r in recs), m)
                d_cwork = torch.empty((size,), dtype=torch.uint8, device=self._dev)
            c.check(c.lib.cel_dev_blobs_emit(c.handle, self._ptr(self.d_eds), self.k, m, self._ptr(d_data),
                                             self._ptr(d_com) if d_com is not None else None, threshold,
                                             self._ptr(d_work), self._ptr(d_cwork) if d_cwork is not None else None,
                                             self._stream_ptr()))
            self._stream.synchronize()
            data = d_data[:nbytes].cpu().numpy()
            com = d_com.cpu().numpy() if d_com is not None else (np.zeros((0, 32), np.uint8) if commitments else None)
        return recs, status[:n], data, com

    def blobs(self, ranges, commitments=True, threshold=64):
        """go-square parseSparseShares over each range of ODS shares of the resident square, on
        the device: per range a list of blob.Blob (with commitments=True each with its share
        commitment), or the blob.BlobParseError of a range that does not parse."""
        from . import blob as _blob
        recs, status, data, com = self.blobs_flat(ranges, commitments=commitments, threshold=threshold)
        return _blob.blobs_from_records(recs, status, data, com, len(ranges))

    def txs_flat(self, ranges, hashes=True):
        """cel_dev_txs_plan + cel_dev_txs_emit over `ranges` ((start, end) in row-major ODS index)
        of the resident square: (records, range status, range flags, data, hashes [n][32] or
        None) as host arrays; unit i's bytes are data[rec.data_off : rec.data_off + rec.len]."""
        from . import square as _square
        torch, c = self._torch, self.ctx
        n = len(ranges)
        starts = np.array([r[0] for r in ranges] or [0], np.uint32)
        ends = np.array([r[1] for r in ranges] or [0], np.uint32)
        if any(not (0 <= int(a) <= int(b) <= self.k * self.k) for a, b in ranges):
            raise CelError(_lib.EINVAL, f"a range is outside the {self.k}x{self.k} square or has start > end")
        total = int(sum(int(b) - int(a) for a, b in ranges))
        status, flags = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        cnt, tb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with torch.cuda.stream(self._stream):
            d_work = torch.empty((max(c.lib.cel_dev_txs_workspace_size(total, n), 16),), dtype=torch.uint8,
                                 device=self._dev)
            c.check(c.lib.cel_dev_txs_plan(c.handle, self._ptr(self.d_eds), self.k, n, _p(starts), _p(ends), _p(status),
                                           _p(flags), ctypes.byref(cnt), ctypes.byref(tb), self._ptr(d_work),
                                           self._stream_ptr()))
            m, nbytes = cnt.value, tb.value
            d_recs = torch.empty((max(m, 1) * ctypes.sizeof(_square.TxRec),), dtype=torch.uint8, device=self._dev)
            d_data = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=self._dev)
            d_hash = torch.empty((max(m, 1), 32), dtype=torch.uint8, device=self._dev) if hashes else None
            c.check(c.lib.cel_dev_txs_emit(c.handle, self._ptr(self.d_eds), self.k, m, self._ptr(d_recs),
                                           self._ptr(d_data), self._ptr(d_hash) if hashes else None,
                                           self._ptr(d_work), self._stream_ptr()))
            self._stream.synchronize()
            raw = d_recs.cpu().numpy().tobytes()
            recs = list((_square.TxRec * m).from_buffer_copy(raw[:m * ctypes.sizeof(_square.TxRec)]))
            data = d_data[:nbytes].cpu().numpy()
            hs = d_hash[:m].cpu().numpy() if hashes else None
        return recs, status[:n], flags[:n], data, hs

    def txs(self, ranges):
        """The compact share parser over each range of ODS shares of the resident square, on the
        device: per range the list of its units (txs, or PayForBlob index wrappers), or the
        square.TxParseError of a range that does not parse."""
        from . import square as _square
        recs, status, _, data, _ = self.txs_flat(ranges, hashes=False)
        return _square.units_from_records(recs, status, data, len(ranges))


class TreeIndexBatch:
    """Many squares resident on the device with their tree indexes, for a node that serves
    samples and namespace queries over many heights at once. `squares`: ExtendedDataSquares or
    (2k, 2k, 512) arrays of mixed widths; they are grouped by width as ExtendBlocks groups blocks,
    one cel_dev_tree_index_build_batch per width, and a call's requests go to the device once per
    width (cel_dev_prove_squares, cel_dev_namespace_plan_squares). row_roots[i], col_roots[i],
    dah[i] and status[i] are square i's, in the caller's order. With order_check a square whose
    shares are not in namespace order keeps its status (EORDER) and the rest are served; a
    request that names such a square raises CelError."""

    def __init__(self, squares, ctx=None, order_check=False):
        import torch
        cells = [np.ascontiguousarray(getattr(s, "cells", s), dtype=np.uint8) for s in squares]
        self.ctx = ctx or next((s._ctx for s in squares if getattr(s, "_ctx", None)), None) or _lib.default_context()
        c = self.ctx
        self._torch = torch
        self._dev = torch.device("cuda", c.device)
        self._stream = torch.cuda.Stream(device=self._dev)
        self.n = len(cells)
        self.widths = []
        self._where = []   # square i -> (its width, its place among the squares of that width)
        self._groups = {}  # width -> dict(ids, d_eds, d_index, d_roots)
        for i, x in enumerate(cells):
            if x.ndim != 3 or x.shape[0] != x.shape[1] or x.shape[2] != _lib.SHARE_SIZE:
                raise CelError(_lib.EINVAL, f"square {i}: need a (2k, 2k, {_lib.SHARE_SIZE}) square, got {x.shape}")
            w = x.shape[0]
            if w < 2 or c.lib.cel_dev_tree_index_batch_size(w // 2, 1) == 0 or w % 2:
                raise CelError(_lib.ENOTPOW2, f"square {i}: square width is not a power of 2: got {w / 2:g}")
            g = self._groups.setdefault(w, dict(ids=[]))
            self._where.append((w, len(g["ids"])))
            g["ids"].append(i)
            self.widths.append(w)
        self.row_roots, self.col_roots = [None] * self.n, [None] * self.n
        self.dah, self.status = [None] * self.n, [0] * self.n
        flags = _lib.FLAG_ORDER_CHECK if order_check else 0
        with torch.cuda.stream(self._stream):
            for w, g in self._groups.items():
                m, k = len(g["ids"]), w // 2
                g["d_eds"] = torch.as_tensor(np.stack([cells[i] for i in g["ids"]])).to(self._dev)
                g["d_index"] = torch.empty((c.lib.cel_dev_tree_index_batch_size(k, m),), dtype=torch.uint8,
                                           device=self._dev)
                g["d_roots"] = torch.empty((2, m, w, NODE), dtype=torch.uint8, device=self._dev)
                d_dah = torch.empty((m, 32), dtype=torch.uint8, device=self._dev)
                status = np.full(m, -1, np.int32)
                c.check(c.lib.cel_dev_tree_index_build_batch(
                    c.handle, self._ptr(g["d_eds"]), m, k, self._ptr(g["d_index"]), self._ptr(g["d_roots"][0]),
                    self._ptr(g["d_roots"][1]), self._ptr(d_dah), _p(status), flags, self._stream_ptr()))
                self._stream.synchronize()
                roots, dahs = g["d_roots"].cpu().numpy(), d_dah.cpu().numpy()
                for j, i in enumerate(g["ids"]):
                    self.row_roots[i] = [r.tobytes() for r in roots[0, j]]
                    self.col_roots[i] = [r.tobytes() for r in roots[1, j]]
                    self.dah[i] = dahs[j].tobytes()
                    self.status[i] = int(status[j])

    _ptr = staticmethod(TreeIndex._ptr)
    _stream_ptr = TreeIndex._stream_ptr

    def _by_width(self, squares, what):
        """Request numbers per width, in request order; a square that is not there or not served raises."""
        out = {}
        for i, sq in enumerate(squares):
            if not 0 <= sq < self.n:
                raise CelError(_lib.EINVAL, f"{what} {i}: square {sq} of {self.n}")
            if self.status[sq] != _lib.OK:
                raise CelError(self.status[sq], f"{what} {i}: square {sq}: invalid push order: a namespace is smaller "
                                                "than the previous one")
            out.setdefault(self._where[sq][0], []).append(i)
        return out

    def prove_flat(self, squares, axes, index, starts, ends, shares=True):
        """Proof i = ProveRange(starts[i], ends[i]) on row (axes[i] = 0) or column (1) index[i] of
        square squares[i]: (leaves [total leaves][512] or None, nodes [total nodes][90], leaf_off,
        node_off) in request order, the flat layout of cel_nmt_verify_batch. One
        cel_dev_prove_squares per width among the requests."""
        torch, c = self._torch, self.ctx
        squares = [int(s) for s in squares]
        axes, index = np.ascontiguousarray(axes, np.uint8), np.ascontiguousarray(index, np.uint32)
        starts, ends = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(ends, np.int32)
        n = len(squares)
        if not (len(axes) == len(index) == len(starts) == len(ends) == n):
            raise CelError(_lib.EINVAL, "squares, axes, index, starts and ends differ in number")
        nl, nn = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        parts = {}
        for w, ids in self._by_width(squares, "proof").items():
            g, ids = self._groups[w], np.array(ids)
            sq = np.array([self._where[squares[i]][1] for i in ids], np.uint32)
            a, t, s, e = (np.ascontiguousarray(v[ids]) for v in (axes, index, starts, ends))
            lo, no = prove_offsets(w // 2, s, e)
            nl[ids], nn[ids] = np.diff(lo), np.diff(no)
            tl, tn = int(lo[-1]), int(no[-1])
            with torch.cuda.stream(self._stream):
                d_leaves = torch.empty((tl, _lib.SHARE_SIZE), dtype=torch.uint8, device=self._dev) if shares else None
                d_nodes = torch.empty((max(tn, 1), NODE), dtype=torch.uint8, device=self._dev)
                d_work = torch.empty((c.lib.cel_dev_prove_squares_workspace_size(len(ids)),), dtype=torch.uint8,
                                     device=self._dev)
                c.check(c.lib.cel_dev_prove_squares(
                    c.handle, self._ptr(g["d_eds"]), self._ptr(g["d_index"]), w // 2, len(g["ids"]), len(ids), _p(sq),
                    _p(a), _p(t), _p(s), _p(e), self._ptr(d_leaves) if shares else None, self._ptr(d_nodes),
                    self._ptr(d_work), self._stream_ptr()))
                self._stream.synchronize()
                parts[w] = (ids, d_leaves.cpu().numpy() if shares else None, d_nodes[:tn].cpu().numpy(), lo, no)
        leaf_off = np.concatenate([[0], np.cumsum(nl)]).astype(np.uint64)
        node_off = np.concatenate([[0], np.cumsum(nn)]).astype(np.uint64)
        leaves = np.zeros((int(leaf_off[-1]), _lib.SHARE_SIZE), np.uint8) if shares else None
        nodes = np.zeros((int(node_off[-1]), NODE), np.uint8)
        for ids, pl, pn, lo, no in parts.values():  # each width's outputs to the requests' own places
            for j, i in enumerate(ids):
                nodes[int(node_off[i]):int(node_off[i + 1])] = pn[int(no[j]):int(no[j + 1])]
                if shares:
                    leaves[int(leaf_off[i]):int(leaf_off[i + 1])] = pl[int(lo[j]):int(lo[j + 1])]
        return leaves, nodes, leaf_off, node_off

    def prove_samples(self, samples):
        """Samples (square, row, col, axis) -> (row, col, axis, share, nodes) each, what
        TreeIndex.prove_samples gives for that square: RepairFromSamples' format."""
        reqs = [(int(q), int(r), int(c), int(a)) for q, r, c, a in samples]
        for i, (q, r, c, a) in enumerate(reqs):
            w = self.widths[q] if 0 <= q < self.n else 0
            if w and not (0 <= r < w and 0 <= c < w and 0 <= a <= 1):
                raise CelError(_lib.EINVAL, f"sample {i}: cell ({r}, {c}) axis {a} outside the square of width {w}")
        index = [c if a else r for _, r, c, a in reqs]
        starts = [r if a else c for _, r, c, a in reqs]
        leaves, nodes, _, node_off = self.prove_flat([q for q, _, _, _ in reqs], [a for _, _, _, a in reqs], index,
                                                     starts, [s + 1 for s in starts])
        return [(r, c, a, leaves[i].tobytes(), [nodes[j].tobytes() for j in range(int(node_off[i]), int(node_off[i + 1]))])
                for i, (_, r, c, a) in enumerate(reqs)]

    def namespace_rows(self, queries):
        """Queries (square, namespace) -> per query what TreeIndex.namespace_rows gives for that
        namespace on that square: a list of (row, NMTProof, shares), rows ascending. One
        cel_dev_namespace_plan_squares and one cel_dev_namespace_prove_squares per width."""
        torch, c = self._torch, self.ctx
        qs = [(int(q), bytes(ns)) for q, ns in queries]
        if any(len(ns) != NS for _, ns in qs):
            raise CelError(_lib.EINVAL, f"a namespace is {NS} bytes")
        out = [[] for _ in qs]
        for w, ids in self._by_width([q for q, _ in qs], "query").items():
            g, k, n = self._groups[w], w // 2, len(ids)
            sq = np.array([self._where[qs[i][0]][1] for i in ids], np.uint32)
            ns = np.frombuffer(b"".join(qs[i][1] for i in ids), np.uint8).copy()
            cnt, cap = ctypes.c_uint64(0), n * w
            with torch.cuda.stream(self._stream):
                d_work = torch.empty((max(c.lib.cel_dev_namespace_squares_workspace_size(k, n), 16),), dtype=torch.uint8,
                                     device=self._dev)
                f = dict(query_idx=np.zeros(cap, np.uint32), rows=np.zeros(cap, np.uint32), starts=np.zeros(cap, np.int32),
                         ends=np.zeros(cap, np.int32), kinds=np.zeros(cap, np.uint8), leaf_off=np.zeros(cap + 1, np.uint64),
                         node_off=np.zeros(cap + 1, np.uint64))
                c.check(c.lib.cel_dev_namespace_plan_squares(
                    c.handle, self._ptr(g["d_index"]), k, len(g["ids"]), n, _p(sq), _p(ns), cap, _p(f["query_idx"]),
                    _p(f["rows"]), _p(f["starts"]), _p(f["ends"]), _p(f["kinds"]), _p(f["leaf_off"]), _p(f["node_off"]),
                    ctypes.byref(cnt), self._ptr(d_work), self._stream_ptr()))
                m = cnt.value
                tl, tn = int(f["leaf_off"][m]), int(f["node_off"][m])
                d_leaves = torch.empty((max(tl, 1), _lib.SHARE_SIZE), dtype=torch.uint8, device=self._dev)
                d_nodes = torch.empty((max(tn, 1), NODE), dtype=torch.uint8, device=self._dev)
                c.check(c.lib.cel_dev_namespace_prove_squares(
                    c.handle, self._ptr(g["d_eds"]), self._ptr(g["d_index"]), k, len(g["ids"]), m, self._ptr(d_leaves),
                    self._ptr(d_nodes), self._ptr(d_work), self._stream_ptr()))
                self._stream.synchronize()
                leaves, nodes = d_leaves[:tl].cpu().numpy(), d_nodes[:tn].cpu().numpy()
            for e in range(m):
                nd = [nodes[j].tobytes() for j in range(int(f["node_off"][e]), int(f["node_off"][e + 1]))]
                absent = int(f["kinds"][e]) == NS_ABSENCE
                p = NMTProof(Start=int(f["starts"][e]), End=int(f["ends"][e]), Nodes=nd[:-1] if absent else nd,
                             LeafHash=nd[-1] if absent else None)
                shares = [leaves[j].tobytes() for j in range(int(f["leaf_off"][e]), int(f["leaf_off"][e + 1]))]
                out[ids[int(f["query_idx"][e])]].append((int(f["rows"][e]), p, shares))
        return out


def NewShareInclusionProofsBatch(eds, requests, ctx=None):
    """NewShareInclusionProofFromEDS(eds, namespace, start, end) for every (namespace, start,
    end) of `requests`, from one tree index: each request splits into per-row ranges as
    CreateShareToRowRootProofs does, and all of them are one cel_dev_prove_batch. The row
    proofs come from the RFC-6962 tree over the roots as before (32 KB at k = 128)."""
    k = eds.Width() // 2
    requests = [(bytes(ns), int(s), int(e)) for ns, s, e in requests]
    for _, s, e in requests:
        if not 0 <= s < e <= k * k:
            raise CelError(_lib.EINVAL, f"share range [{s}, {e}) outside the {k}x{k} square")
    if not requests:
        return []
    index = TreeIndex(eds, ctx=ctx or eds.ctx)
    roots = eds.RowRoots()
    levels = dah_tree(eds, ctx=ctx)
    n = 4 * k
    rows, starts, ends, spans = [], [], [], []
    for _, s, e in requests:
        start_row, end_row = s // k, (e - 1) // k
        spans.append((len(rows), start_row, end_row))
        for r in range(start_row, end_row + 1):
            if index.row_roots[r] != roots[r]:
                raise CelError(_lib.EINVAL, "eds row root is different than tree root")
            rows.append(r)
            starts.append(s % k if r == start_row else 0)
            ends.append((e - 1) % k + 1 if r == end_row else k)  # the ODS part of the row
    proofs, shares = index.prove_ranges([0] * len(rows), rows, starts, ends, shares=True)
    out = []
    for (ns, _, _), (at, start_row, end_row) in zip(requests, spans):
        cnt = end_row - start_row + 1
        row_proofs = [Proof(Total=n, Index=r, LeafHash=levels[r].tobytes(), Aunts=merkle_aunts(levels, n, r))
                      for r in range(start_row, end_row + 1)]
        out.append(ShareProof(Data=[x for leaves in shares[at:at + cnt] for x in leaves],
                              ShareProofs=proofs[at:at + cnt], NamespaceId=ns[1:], NamespaceVersion=ns[0],
                              RowProof=RowProof(RowRoots=[roots[r] for r in range(start_row, end_row + 1)],
                                                Proofs=row_proofs, StartRow=start_row, EndRow=end_row)))
    return out


TX_NAMESPACE = bytes(28) + b"\x01"
PFB_NAMESPACE = bytes(28) + b"\x04"


def ParseNamespace(raw_shares, start_share, end_share):
    """pkg/proof/querier.go:134-166: check the end-exclusive share range and that every
    share in it carries the first one's namespace (29 bytes); return that namespace.
    Raises CelError(EINVAL) with the reference's messages."""
    if start_share < 0:
        raise CelError(_lib.EINVAL, f"start share {start_share} should be positive")
    if end_share < 0:
        raise CelError(_lib.EINVAL, f"end share {end_share} should be positive")
    if end_share <= start_share:
        raise CelError(_lib.EINVAL,
                       f"end share {end_share} cannot be lower or equal to the starting share {start_share}")
    if end_share > len(raw_shares):
        raise CelError(_lib.EINVAL, f"end share {end_share} is higher than block shares {len(raw_shares)}")
    first = bytes(raw_shares[start_share][:NS])
    if len(first) < NS:
        raise CelError(_lib.ESHORT, "share is too short to contain a namespace")
    # Each share's length is checked where the reference parses its namespace (querier.go:
    # 157-160, share.Namespace() per share). The mismatch message prints the namespaces in
    # hex; the reference formats them with %v (a byte-slice dump), so only the text before
    # the colon matches it.
    for i, sh in enumerate(raw_shares[start_share:end_share]):
        ns = bytes(sh[:NS])
        if len(ns) < NS:
            raise CelError(_lib.ESHORT, "share is too short to contain a namespace")
        if ns != first:
            raise CelError(_lib.EINVAL, f"shares range contain different namespaces at index {i}: "
                                        f"{first.hex()} and {ns.hex()} ")
    return first


def NewTxInclusionProof(txs, tx_index, max_square_size=128, subtree_root_threshold=64):
    """pkg/proof/proof.go:21-48: square.Construct, FindTxShareRange, then the share proof
    of that range in the tx's namespace (PayForBlob for blob txs, proof.go:50-56)."""
    from . import square
    if tx_index >= len(txs):
        raise CelError(_lib.EINVAL, f"txIndex {tx_index} out of bounds")
    start, end = square.TxShareRange(txs, tx_index, max_square_size, subtree_root_threshold)
    ods = square.Construct(txs, max_square_size, subtree_root_threshold)
    ns = PFB_NAMESPACE if bytes(ods[start][:NS]) == PFB_NAMESPACE else TX_NAMESPACE
    return NewShareInclusionProof(list(ods), ns, start, end)


# ------------------------------------------------------- batched verification
def _verify_batch(proofs, namespaces, leaves_per_proof, roots, ctx, nodes_of, kind_of):
    """The batch verifiers' common part: proofs of other sizes than the app's are False, the
    others flattened into one call. nodes_of(proof): its 90-byte nodes as they travel;
    kind_of: None for cel_nmt_verify_batch, else proof -> kind for cel_nmt_verify_namespace_batch."""
    n = len(proofs)
    if not (len(namespaces) == len(leaves_per_proof) == len(roots) == n):
        raise CelError(_lib.EINVAL, "proofs, namespaces, leaves and roots differ in number")
    out = [False] * n
    share = _lib.SHARE_SIZE
    keep = [i for i in range(n)
            if len(namespaces[i]) == NS and len(roots[i]) == NODE
            and -(1 << 31) <= proofs[i].Start < 1 << 31 and -(1 << 31) <= proofs[i].End < 1 << 31
            and all(len(x) == NODE for x in nodes_of(proofs[i])) and all(len(x) == share for x in leaves_per_proof[i])]
    if not keep:
        return out
    ctx = ctx or _lib.default_context()
    root_at, root_idx = {}, []
    for i in keep:
        root_idx.append(root_at.setdefault(bytes(roots[i]), len(root_at)))
    leaf_off = np.cumsum([0] + [len(leaves_per_proof[i]) for i in keep]).astype(np.uint64)
    node_off = np.cumsum([0] + [len(nodes_of(proofs[i])) for i in keep]).astype(np.uint64)
    buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    starts = np.array([proofs[i].Start for i in keep], np.int32)
    ends = np.array([proofs[i].End for i in keep], np.int32)
    ns = buf(bytes(namespaces[i]) for i in keep)
    leaves = buf(bytes(x) for i in keep for x in leaves_per_proof[i])
    nodes = buf(bytes(x) for i in keep for x in nodes_of(proofs[i]))
    rts = buf(root_at)
    ridx = np.array(root_idx, np.uint32)
    ok = np.zeros(len(keep), np.uint8)
    tail = (_p(ns), _p(leaves), _p(leaf_off), _p(nodes), _p(node_off), _p(rts), len(root_at), _p(ridx), _p(ok))
    if kind_of is None:
        ctx.check(ctx.lib.cel_nmt_verify_batch(ctx.handle, len(keep), _p(starts), _p(ends), *tail))
    else:
        kinds = np.array([kind_of(proofs[i]) for i in keep], np.uint8)
        ctx.check(ctx.lib.cel_nmt_verify_namespace_batch(ctx.handle, len(keep), _p(starts), _p(ends), _p(kinds), *tail))
    for i, v in zip(keep, ok):
        out[i] = bool(v)
    return out


def VerifyInclusionBatch(proofs, namespaces, leaves_per_proof, roots, ctx=None):
    """NMTProof.VerifyInclusion(namespaces[i], leaves_per_proof[i], roots[i]) for every proof
    in one device batch (cel_nmt_verify_batch): a list of bools. The device verifies the
    app's sizes: a proof with a node that is not 90 bytes long, a leaf that is not 512, a
    namespace that is not 29 or a root that is not 90 is False without reaching the device."""
    return _verify_batch(proofs, namespaces, leaves_per_proof, roots, ctx, lambda p: p.Nodes, None)


def VerifyNamespaceBatch(proofs, namespaces, leaves_per_proof, roots, ctx=None):
    """NMTProof.VerifyNamespace(namespaces[i], leaves_per_proof[i], roots[i]) for every proof in one
    device batch (cel_nmt_verify_namespace_batch): a list of bools. A proof with a non-empty
    LeafHash is an absence proof; its leaf hash travels as the last node. Sizes other than the
    app's are False without reaching the device, as in VerifyInclusionBatch."""
    return _verify_batch(proofs, namespaces, leaves_per_proof, roots, ctx,
                         lambda p: list(p.Nodes) + ([bytes(p.LeafHash)] if p.LeafHash else []),
                         lambda p: NS_ABSENCE if p.LeafHash else NS_INCLUSION)


def VerifyShareProofs(share_proofs, root, ctx=None):
    """[True where share_proofs[i].Validate(root) would not raise]. The structural checks of
    ShareProof.Validate and the RFC-6962 row proofs (18 compressions per row) run on the
    host; every NMT range proof of every ShareProof goes through one device batch."""
    out = [False] * len(share_proofs)
    proofs, nss, leaves, roots, owner = [], [], [], [], []
    for i, sp in enumerate(share_proofs):
        try:  # ShareProof.Validate up to its VerifyProof
            if sp.RowProof is None or not sp.Data:
                continue
            if len(sp.ShareProofs) != len(sp.RowProof.RowRoots):
                continue
            if len(sp.Data) != sum(p.End - p.Start for p in sp.ShareProofs):
                continue
            if any(p.Start < 0 or p.End - p.Start <= 0 for p in sp.ShareProofs):
                continue
            sp.RowProof.Validate(root)
        except CelError:
            continue
        if sp.NamespaceVersion > 255:
            continue
        ns = bytes([sp.NamespaceVersion]) + bytes(sp.NamespaceId)
        if len(ns) != NS:  # nmt is generic in the namespace size, the device is not
            out[i] = sp.VerifyProof()
            continue
        out[i] = True  # unless one of its range proofs fails
        cursor = 0
        for j, p in enumerate(sp.ShareProofs):
            used = p.End - p.Start
            proofs.append(p)
            nss.append(ns)
            leaves.append(sp.Data[cursor:cursor + used])
            roots.append(sp.RowProof.RowRoots[j])
            owner.append(i)
            cursor += used
    for i, v in zip(owner, VerifyInclusionBatch(proofs, nss, leaves, roots, ctx=ctx)):
        out[i] = out[i] and v
    return out
