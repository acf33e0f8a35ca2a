"""Bad-encoding fraud proofs over the device library, after celestia-node's
share/eds/byzantine (specs/src/specs/fraud_proofs.md:3-13, networking.md "Invalid Erasure
Coding", types.proto BadEncodingFraudProof):
  ShareWithProof, BadEncodingProof          the proof and its entries
  CreateBadEncodingProof                    from the ErrByzantineData a repair raised
  BadEncodingProof.Validate, ValidateBatch  the verdict, one proof or many in one device call
A proof accuses axis (Axis, Index) of a square (Axis 0 a row, 1 a column). Each entry is a
share of that axis at `Position` with its single-leaf NMT proof in the cell's row tree (entry
Axis 0) or column tree (entry Axis 1), the convention of RepairFromSamples: the cell is
(Index, Position) of an accused row, (Position, Index) of an accused column.

The verdict (_lib.BEFP_*), the rule in celestia-node's Validate order: MALFORMED (an axis above
1, an index or position outside the square, two entries at one position), TOO_FEW (fewer than k
entries), BAD_SHARE (an entry's proof does not verify), else the axis is rebuilt from the
entries (Decode, then Encode of the data half) and FRAUD / NOT_FRAUD says whether its root
differs from the accused root. All arithmetic runs in libcelestia_eds.so (cel_befp_verify_batch,
cel_befp_build); this module marshals bytes.
"""
import ctypes
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import _lib
from ._lib import BEFP_BAD_SHARE, BEFP_FRAUD, BEFP_MALFORMED, BEFP_NOT_FRAUD, BEFP_TOO_FEW, CelError  # noqa: F401

Row, Col = 0, 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@dataclass
class ShareWithProof:
    """byzantine.ShareWithProof: the share at `Position` of the accused axis, the nodes of its
    single-leaf nmt proof (nmt order) and the direction of the tree it is proved in."""
    Position: int
    Share: bytes
    Nodes: List[bytes]
    Axis: int


@dataclass
class BadEncodingProof:
    """byzantine.BadEncodingProof{headerHash/BlockHeight, Shares, Index, Axis}."""
    Height: int
    Axis: int
    Index: int
    Shares: List[ShareWithProof] = field(default_factory=list)

    def Validate(self, row_roots, col_roots, ctx=None):
        """The verdict against the header's roots (2k each); len(row_roots) gives the width."""
        return ValidateBatch([self], [row_roots], [col_roots], len(row_roots) // 2, ctx=ctx)[0]


def _u32(v):
    return isinstance(v, (int, np.integer)) and 0 <= int(v) < 1 << 32


def structural_verdict(proof, k):
    """Steps 1 and 2 of the rule, no device: BEFP_MALFORMED, BEFP_TOO_FEW, or None where the
    entries' proofs decide."""
    w = 2 * k
    if proof.Axis not in (Row, Col) or not _u32(proof.Index) or proof.Index >= w:
        return BEFP_MALFORMED
    seen = set()
    for s in proof.Shares:
        if s.Axis not in (Row, Col) or not _u32(s.Position) or s.Position >= w or s.Position in seen:
            return BEFP_MALFORMED
        seen.add(s.Position)
    return BEFP_TOO_FEW if len(proof.Shares) < k else None


def _packable(proof):
    """Can every field be handed to the library as it is? (Everything the library would call
    malformed can: only lengths and integer ranges are looked at.)"""
    return (_u32(proof.Axis) and proof.Axis < 256 and _u32(proof.Index) and
            all(_u32(s.Position) and _u32(s.Axis) and s.Axis < 256 and len(s.Share) == _lib.SHARE_SIZE and
                all(len(x) == _lib.NMT_NODE_SIZE for x in s.Nodes) for s in proof.Shares))


def ValidateBatch(proofs, row_roots, col_roots, k, ctx=None, rebuilt=False):
    """The verdicts of many proofs for squares of one k in one device call
    (cel_befp_verify_batch): row_roots[i] / col_roots[i] the 2k roots of proof i's square.
    Returns one verdict per proof; with rebuilt=True (verdicts, roots), roots[i] the rebuilt
    axis's 90-byte root where the verdict is FRAUD or NOT_FRAUD, else None. An entry whose share
    is not 512 bytes long or that has a node that is not 90 is a failing entry: its proof is
    BAD_SHARE (after the structural checks) without reaching the device."""
    proofs = list(proofs)
    n, w, share, node = len(proofs), 2 * k, _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
    if len(row_roots) != n or len(col_roots) != n:
        raise CelError(_lib.EINVAL, f"need row and column roots for each of the {n} proofs")
    verdicts, roots = [None] * n, [None] * n
    send = []
    for i, p in enumerate(proofs):
        if _packable(p):
            send.append(i)
        else:
            v = structural_verdict(p, k)
            verdicts[i] = BEFP_BAD_SHARE if v is None else v
    if send:
        rr = np.frombuffer(b"".join(b"".join(bytes(x) for x in row_roots[i]) for i in send), np.uint8).copy()
        cr = np.frombuffer(b"".join(b"".join(bytes(x) for x in col_roots[i]) for i in send), np.uint8).copy()
        if rr.size != len(send) * w * node or cr.size != rr.size:
            raise CelError(_lib.EINVAL, f"need {w} row roots and {w} column roots of {node} bytes per proof")
        ents = [s for i in send for s in proofs[i].Shares]
        buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
        axes = np.array([proofs[i].Axis for i in send], np.uint8)
        index = np.array([proofs[i].Index for i in send], np.uint32)
        ent_off = np.cumsum([0] + [len(proofs[i].Shares) for i in send]).astype(np.uint64)
        positions = np.array([s.Position for s in ents] or [0], np.uint32)
        ent_axes = np.array([s.Axis for s in ents] or [0], np.uint8)
        shares = buf(bytes(s.Share) for s in ents)
        nodes = buf(bytes(x) for s in ents for x in s.Nodes)
        node_off = np.cumsum([0] + [len(s.Nodes) for s in ents]).astype(np.uint64)
        out = np.zeros(len(send), np.uint8)
        reb = np.zeros((len(send), node), np.uint8)
        ctx = ctx or _lib.default_context()
        ctx.check(ctx.lib.cel_befp_verify_batch(ctx.handle, len(send), k, _p(axes), _p(index), _p(ent_off),
                                                _p(positions), _p(ent_axes), _p(shares), _p(nodes), _p(node_off),
                                                _p(rr), _p(cr), _p(out), _p(reb)))
        for j, i in enumerate(send):
            verdicts[i] = int(out[j])
            if verdicts[i] in (BEFP_FRAUD, BEFP_NOT_FRAUD):
                roots[i] = reb[j].tobytes()
    return (verdicts, roots) if rebuilt else verdicts


def CreateBadEncodingProof(height, err, square, row_roots, col_roots, samples=None):
    """byzantine.NewBadEncodingProof for the rsmt2d.ErrByzantineData `err` a repair raised:
    `square` is the most-repaired ExtendedDataSquare the repair left, with the mask it is valid
    under (square._mask), row_roots / col_roots the header's. The device producer
    (cel_befp_build) gives an entry for every known cell of the accused axis whose orthogonal
    axis is complete and matches its root in the header, proved in that orthogonal tree.
    `samples`, in RepairFromSamples' format (row, col, axis, share, nodes), fill positions it did
    not cover, in either proving direction; they are taken as they are (Validate checks them).
    The proof may hold fewer than k entries: Validate then says TOO_FEW."""
    ctx, w, share, node = square.ctx, square.Width(), _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE
    k, per = w // 2, w.bit_length() - 1
    axis, index = int(err.Axis), int(err.Index)
    mask = getattr(square, "_mask", None)
    mask = np.ones((w, w), np.uint8) if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    cells = np.ascontiguousarray(square.cells, dtype=np.uint8)
    rr = np.frombuffer(b"".join(bytes(x) for x in row_roots), np.uint8).copy()
    cr = np.frombuffer(b"".join(bytes(x) for x in col_roots), np.uint8).copy()
    if rr.size != w * node or cr.size != w * node or mask.shape != (w, w):
        raise CelError(_lib.EINVAL, f"need a {w} x {w} mask and {w} row and column roots of {node} bytes")
    positions, ent_axes = np.zeros(w, np.uint32), np.zeros(w, np.uint8)
    shares, nodes = np.zeros((w, share), np.uint8), np.zeros((w, per, node), np.uint8)
    count = ctypes.c_uint32()
    ctx.check(ctx.lib.cel_befp_build(ctx.handle, _p(cells), _p(mask), k, _p(rr), _p(cr), axis, index, _p(positions),
                                     _p(ent_axes), _p(shares), _p(nodes), ctypes.byref(count)))
    ents = {int(positions[e]): ShareWithProof(int(positions[e]), shares[e].tobytes(),
                                              [nodes[e, j].tobytes() for j in range(per)], int(ent_axes[e]))
            for e in range(count.value)}
    for r, c, a, sh, nd in samples or []:
        on_axis, pos = (r == index, c) if axis == Row else (c == index, r)
        if on_axis and 0 <= pos < w and pos not in ents:
            ents[int(pos)] = ShareWithProof(int(pos), bytes(sh), [bytes(x) for x in nd], int(a))
    return BadEncodingProof(height, axis, index, [ents[p] for p in sorted(ents)])
