"""The encoding checks of the device repair, by byte: where in a share, a shard and an axis list
a single flipped bit is still seen.

Every case starts from a complete, valid square (every cell present), flips one bit at cell
(r, c), byte b, and recomputes the two roots the flip changes (row r, column c, without the
push-order check), so every root matches and only rsmt2d's re-encoding of complete axes
(preRepairSanityCheck) can object. Flips stay out of the first 29 bytes of Q0 cells, so
namespaces and their order are untouched.

Expected outcome (the rule): CEL_EBYZANTINE; rsmt2d checks row i, then column i, so the axis
is row r if r <= c, else column c; all 2k shares of that axis are present and equal that
axis of the corrupted square. The rule is compared with the oracle's rsmt2d restatement
(oracle.repair through test_gpu_repair._assert_same_outcome) on a sample of the cases at
every width up to k = 32; above that the oracle's full repair takes too long and the rule
stands alone.

One device buffer per width holds the clean square; a case uploads the one changed cell and
puts the clean cell back afterwards, so a device that wrote into the square on a rejected
call would break the cases after it (and the final download, where there is one).

Paths by width (api_repair.cpp check_in_square):
  k = 1, 2, 16   gather -> encode -> k_cmp (uint4 compares over the parity half)
  k = 32..128    k_rs_check_axes<5|6|7>: one wave per (listed axis, 256-byte slice), one dword
                 per lane, OR over the K parity shards
  k = 256        the GF(2^16) register encoder in check mode, in place (rows at the cell
                 stride, columns at the row stride); k = 512 stays with
                 test_gpu_repair.test_sanity_check_bad_encoding
Stale roots (the clean square's roots with the same flips) must be CEL_EBADROOT on the same
axis; those cases compare with the oracle in full.
"""
import ctypes

import numpy as np
import pytest

from eds_inputs import random_ods

pytestmark = pytest.mark.gpu

SHARE = 512
_CLEAN = {}


def clean(oracle, k):
    """(eds, row roots, column roots) of one valid square per width, computed once and never
    written."""
    if k not in _CLEAN:
        eds, rr, cr, _ = oracle.extend_and_commit(random_ods(k, 8800 + k))
        for a in (eds, rr, cr):
            a.setflags(write=False)
        _CLEAN[k] = (eds, rr, cr)
    return _CLEAN[k]


class Square:
    """The clean square of width k resident on the device, and single-cell corruption."""

    def __init__(self, ctx, oracle, k):
        from hipmem import DeviceBuffer
        self.ctx, self.oracle, self.k, self.w = ctx, oracle, k, 2 * k
        self.eds, self.rr, self.cr = clean(oracle, k)
        self.dev = DeviceBuffer(self.eds.nbytes)
        self.dev.upload(self.eds)

    def flipped(self, r, c, b, bit):
        k = self.k
        assert not (r < k and c < k and b < 29), "flips stay out of Q0's namespace bytes"
        cell = self.eds[r, c].copy()
        cell[b] ^= 1 << bit
        return cell

    def roots_over(self, r, c, cell):
        """The clean roots with row r and column c recomputed over the corrupted cell."""
        row, col = self.eds[r].copy(), self.eds[:, c].copy()
        row[c] = cell
        col[r] = cell
        rr, cr = self.rr.copy(), self.cr.copy()
        rr[r] = np.frombuffer(self.oracle.axis_root(row, self.k, r, check_order=False)[1], np.uint8)
        cr[c] = np.frombuffer(self.oracle.axis_root(col, self.k, c, check_order=False)[1], np.uint8)
        return rr, cr, row, col

    def repair(self, r, c, cell, rr, cr):
        """cel_dev_repair over the resident square with cell (r, c) replaced; the clean cell
        is put back afterwards. Returns (status, (axis, index), shares, present)."""
        w = self.w
        off = (r * w + c) * SHARE
        self.dev.upload_at(off, cell)
        pres = np.ones((w, w), np.uint8)
        rra, cra = np.ascontiguousarray(rr), np.ascontiguousarray(cr)
        ba, bi = ctypes.c_int32(-1), ctypes.c_int32(-1)
        bs, bp = np.zeros((w, SHARE), np.uint8), np.zeros(w, np.uint8)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        st = self.ctx.lib.cel_dev_repair(self.ctx.handle, self.dev.ptr, P(pres), self.k, P(rra), P(cra),
                                         ctypes.byref(ba), ctypes.byref(bi), P(bs), P(bp))
        self.dev.upload_at(off, self.eds[r, c])
        assert pres.all(), "the mask of a complete square changed"
        return st, (ba.value, bi.value), bs, bp

    def assert_detected(self, r, c, b, bit):
        """The rule, on the device alone."""
        from celestia_eds import _lib
        cell = self.flipped(r, c, b, bit)
        rr, cr, row, col = self.roots_over(r, c, cell)
        st, axis, bs, bp = self.repair(r, c, cell, rr, cr)
        what = f"k={self.k} cell ({r}, {c}) byte {b} bit {bit}"
        assert st == _lib.EBYZANTINE, f"{what}: status {st}"
        assert axis == ((0, r) if r <= c else (1, c)), f"{what}: axis {axis}"
        assert bp.all(), f"{what}: shares missing"
        assert np.array_equal(bs, row if r <= c else col), f"{what}: shares differ"

    def assert_rule_is_oracles(self, r, c, b, bit):
        """The rule against the oracle's restatement, and the device against both (a fresh
        device copy: test_gpu_repair's helper)."""
        from celestia_eds import _lib
        from test_gpu_repair import _assert_same_outcome
        cell = self.flipped(r, c, b, bit)
        rr, cr, row, col = self.roots_over(r, c, cell)
        bad = self.eds.copy()
        bad[r, c] = cell
        st, axis, bs, bp = _assert_same_outcome(self.ctx, self.oracle, bad, np.ones((self.w, self.w), np.uint8),
                                                list(rr), list(cr))
        assert st == _lib.EBYZANTINE and axis == ((0, r) if r <= c else (1, c))
        assert bp.all() and np.array_equal(bs, row if r <= c else col)

    def assert_untouched(self):
        assert np.array_equal(self.dev.download(self.eds.shape), self.eds), "a rejected repair wrote into the square"


def _q0_safe(k, cells, b):
    """The cells of the list a flip at byte b may use."""
    return [(r, c) for r, c in cells if not (r < k and c < k and b < 29)]


def test_check_axes_k32_every_dword_lane(ctx, oracle):
    """k_rs_check_axes<5>: byte b = 4j + (j mod 4) for j in 0..127 is every dword lane of both
    256-byte slices and every byte within a dword, bit j mod 8 every bit. The cells walk
    parity shards k, k + 1, 2k - 1 and data shards 0, k - 1 of the reported axis, axes 0 and
    2k - 1 (the first and last listed), and both directions (r < c: row, r > c: column)."""
    k = 32
    sq = Square(ctx, oracle, k)
    w = 2 * k
    cells = [(0, k), (0, k + 1), (0, w - 1), (k, 0), (k + 1, 0), (w - 1, 0), (w - 1, w - 1), (w - 1, w - 2),
             (0, 0), (0, k - 1), (k - 1, 0), (k - 1, w - 1), (w - 1, k - 1), (k + 8, k + 19), (k + 19, k + 8)]
    n = 0
    for j in range(128):
        b = 4 * j + (j % 4)
        ok = _q0_safe(k, cells, b)
        for r, c in (ok[j % len(ok)], ok[(j + 7) % len(ok)]):
            sq.assert_detected(r, c, b, j % 8)
            n += 1
    assert n == 256
    sq.assert_untouched()


@pytest.mark.parametrize("k", [64, 128])
def test_check_axes_k64_k128(ctx, oracle, k):
    """k_rs_check_axes<6> and <7>: slice 1, lane 63 of both slices, lane 0, parity shards k and
    2k - 1, data shards 0 and k - 1, axes 0 and 2k - 1, both directions. The rule alone."""
    sq = Square(ctx, oracle, k)
    w = 2 * k
    for r, c, b, bit in [(0, k, 3, 0), (0, w - 1, 255, 7), (w - 1, 0, 256, 1), (w - 1, w - 1, 511, 6),
                         (k, 0, 300, 2), (5, k + 1, 252, 5), (k - 1, k - 1, 29, 3), (w - 1, w - 2, 508, 4),
                         (0, 0, 260, 7), (k + 1, k - 1, 131, 0)]:
        sq.assert_detected(r, c, b, bit)
    sq.assert_untouched()


@pytest.mark.parametrize("k", [1, 2, 16])
def test_gather_encode_cmp_every_uint4(ctx, oracle, k):
    """k < 32: gather -> encode -> k_cmp. Byte b = 16q + (q mod 16) for q in 0..31 is every
    uint4 of a share and every byte within one; the cells walk the first and last parity and
    data shard and the first and last axis, both directions."""
    sq = Square(ctx, oracle, k)
    w = 2 * k
    cells = sorted({(0, k), (0, w - 1), (k, 0), (w - 1, 0), (w - 1, w - 1), (w - 1, w - 2), (0, 0), (k - 1, k - 1),
                    (0, k - 1), (k - 1, 0), (k - 1, w - 1), (w - 1, k - 1)})
    for q in range(32):
        b = 16 * q + (q % 16)
        ok = _q0_safe(k, cells, b)
        for r, c in (ok[q % len(ok)], ok[(q + 5) % len(ok)]):
            sq.assert_detected(r, c, b, q % 8)
    sq.assert_untouched()


def test_gf16_check_k256_every_leopard_half_block(ctx, oracle):
    """k = 256: the GF(2^16) register encoder in check mode, in place on the square. A
    512-byte share is eight 64-byte Leopard blocks of 32 low and 32 high bytes: one flip in
    each half of each block (16 positions), over the first and last parity shard and a data
    shard, the first and last axis, rows (cell stride) and columns (row stride). One device
    buffer, one cell re-uploaded per case; the rule alone."""
    k = 256
    sq = Square(ctx, oracle, k)
    w = 2 * k
    cells = [(0, k), (0, w - 1), (k, 0), (w - 1, 0), (w - 1, w - 1), (w - 1, w - 2), (0, 0), (k - 1, 3)]
    for p in range(16):
        b = 64 * (p // 2) + 32 * (p % 2) + (5 * p + 29) % 32
        for r, c in (cells[p % len(cells)], cells[(p + 3) % len(cells)]):
            if r < k and c < k and b < 29:
                r += k
            sq.assert_detected(r, c, b, p % 8)


@pytest.mark.parametrize("k", [1, 2, 16, 32])
def test_rule_matches_oracle(ctx, oracle, k):
    """The rule this file asserts is the oracle's: status, axis and shares of the rsmt2d
    restatement on a sample of the cases above (both directions, the diagonal, data and
    parity shards, first and last axis)."""
    sq = Square(ctx, oracle, k)
    w = 2 * k
    cases = [(0, k, 3, 0), (0, w - 1, 255, 7), (w - 1, 0, 256, 1), (w - 1, w - 1, 511, 6), (k, 0, 300, 2),
             (w - 1, w - 2, 508, 4), (0, 0, 260, 7), (k - 1, k - 1, 29, 3), (k - 1, w - 1, 64, 5), (w - 1, k - 1, 447, 2)]
    cases = sorted(set(cases))
    assert len(cases) >= (4 if k == 1 else 8)
    for r, c, b, bit in cases:
        sq.assert_rule_is_oracles(r, c, b, bit)


@pytest.mark.parametrize("k", [8, 32])
def test_stale_roots_bad_root(ctx, oracle, k):
    """The same flips against the clean square's roots: the changed leaf moves the root of
    row r and column c, and rsmt2d's "bad root input" (CEL_EBADROOT) names row r if r <= c,
    else column c. One flip in each of the nine SHA-256 blocks of the 542-byte leaf message
    (share byte q is message byte 30 + q), at block edges, and in Q0's namespace bytes (part
    of the node's min / max namespace, not only of the digest). Status, axis and index, the
    mask and the square against the oracle in full."""
    from celestia_eds import _lib
    from test_gpu_repair import _assert_same_outcome
    eds, rr, cr = clean(oracle, k)
    w = 2 * k
    # block j of the leaf message holds share bytes [64j - 30, 64j + 34)
    offs = [0, 33, 34, 97, 98, 161, 200, 226, 289, 290, 353, 400, 418, 481, 482, 511]
    assert {(q + 30) // 64 for q in offs} == set(range(9))
    cells = [(0, k), (k, 0), (w - 1, w - 1), (w - 1, w - 2), (0, w - 1), (w - 1, 0), (k + 1, k + 2), (3, k - 1)]
    cases = [(cells[i % len(cells)] + (q, i % 8)) for i, q in enumerate(offs)]
    cases += [(0, 0, 0, 0), (0, 1, 28, 7), (k - 1, k - 1, 13, 3), (2, 1, 27, 0), (1, 2, 5, 4), (k - 1, 0, 19, 6),
              (0, k - 1, 28, 0), (3, 3, 1, 2)]
    assert len(cases) == 24
    present = np.ones((w, w), np.uint8)
    for r, c, b, bit in cases:
        bad = eds.copy()
        bad[r, c, b] ^= 1 << bit
        st, axis, _, _ = _assert_same_outcome(ctx, oracle, bad, present, list(rr), list(cr))
        what = f"k={k} cell ({r}, {c}) byte {b} bit {bit}"
        assert st == _lib.EBADROOT, f"{what}: status {st}"
        assert axis == ((0, r) if r <= c else (1, c)), f"{what}: axis {axis}"
