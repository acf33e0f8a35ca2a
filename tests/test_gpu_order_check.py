"""The push-order check (CEL_FLAG_ORDER_CHECK -> CEL_EORDER) by namespace byte, by position in
the square, by square of a batch and by entry point. A missed CEL_EORDER lets the device
commit to a square the reference's nmt Push refuses; a false one refuses a valid block.

Every expected status is the whole-square CPU oracle's
(oracle.roots(oracle.extend(ods), check_order=True)[0]); the one exception is the k = 512
case, which says so. Squares the oracle accepts must also come out with the oracle's roots
and DAH; nothing is asserted about the roots of a rejected square.

What a case is made of is asserted in numpy (`violations`): which cells are below their left
neighbour (a row violation) and which below the cell above (a column violation).
"""
import ctypes

import numpy as np
import pytest

from eds_inputs import parity_before_boundary_ods

pytestmark = pytest.mark.gpu

NS, SHARE, NODE = 29, 512, 90
EORDER = 5
_P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ------------------------------------------------------------------ construction and oracle

def ns_lt(a, b):
    """Lexicographic a < b over the last axis (29 namespace bytes)."""
    d = a != b
    i = d.argmax(-1)[..., None]
    return d.any(-1) & (np.take_along_axis(a, i, -1)[..., 0] < np.take_along_axis(b, i, -1)[..., 0])


def violations(ods):
    """(row, col): boolean [k][k]; row[r, c]: cell (r, c)'s namespace is below (r, c - 1)'s,
    col[r, c]: below (r - 1, c)'s."""
    ns = ods[:, :, :NS]
    row = np.zeros(ns.shape[:2], bool)
    col = np.zeros(ns.shape[:2], bool)
    row[:, 1:] = ns_lt(ns[:, 1:], ns[:, :-1])
    col[1:, :] = ns_lt(ns[1:, :], ns[:-1, :])
    return row, col


_PAYLOAD = {}


def payload(k):
    """Random share bytes of a k x k square, drawn once per width (copied by every user);
    above k = 128 the k = 128 bytes tiled: the push order never looks past byte 28."""
    if k not in _PAYLOAD:
        if k > 128:
            a = np.tile(payload(128), (k // 128, k // 128, 1))
        else:
            a = np.random.default_rng(4200 + k).integers(0, 256, (k, k, SHARE), dtype=np.uint8)
        a.setflags(write=False)
        _PAYLOAD[k] = a
    return _PAYLOAD[k]


def graded(k, by):
    """A valid square whose namespaces are 0x80 bytes with a big-endian grade in two of them:
    by = "row": grade r + 1 in bytes 27..28 (constant along a row, rising down a column);
    by = "col": grade c + 1 in bytes 0..1 (constant down a column, rising along a row)."""
    ods = payload(k).copy()
    ods[:, :, :NS] = 0x80
    g = np.arange(1, k + 1)
    g = g[:, None] if by == "row" else g[None, :]
    at = 27 if by == "row" else 0
    ods[:, :, at] = g >> 8
    ods[:, :, at + 1] = g & 0xFF
    return ods


def lowered(k, by, r, c):
    """graded(k, by) with cell (r, c)'s grade one lower. by = "row": the cell equals the one
    above and is below its left neighbour: a row-only violation (c > 0). by = "col": it
    equals its left neighbour and is below the cell above: column-only (r > 0)."""
    ods = graded(k, by)
    at = 27 if by == "row" else 0
    g = (r if by == "row" else c)  # the cell's grade, r + 1 or c + 1, minus one
    ods[r, c, at], ods[r, c, at + 1] = g >> 8, g & 0xFF
    row, col = violations(ods)
    want_row, want_col = np.zeros((k, k), bool), np.zeros((k, k), bool)
    (want_row if by == "row" else want_col)[r, c] = True
    assert np.array_equal(row, want_row) and np.array_equal(col, want_col), (k, by, r, c)
    return ods


def parity_tail_valid(k):
    """Valid: every cell outside the left half of Q0 carries 0xFF*29, so each row ends in
    parity-namespace shares and the next row starts, in row-major order, with a lower one."""
    ods = graded(k, "row")
    ods[:, k // 2:, :NS] = 0xFF
    row, col = violations(ods)
    assert not row.any() and not col.any()
    return ods


def position_cases(k):
    """name -> ods of the position sweep at width k. A leaf workgroup is 256 consecutive
    cells of the 2k-wide EDS: 256 / 2k rows (k = 16: eight, k = 32: four, k = 128: one)."""
    rows_wg = max(1, 256 // (2 * k))
    e = max(2, rows_wg)  # the first row of a workgroup after the first (k = 16: 8, k = 32: 4, k = 128: 2)
    m = {
        "clean_row": lambda: graded(k, "row"),
        "row(0,1)": lambda: lowered(k, "row", 0, 1),
        "col(1,0)": lambda: lowered(k, "col", 1, 0),
        "row(0,k-1)": lambda: lowered(k, "row", 0, k - 1),
        "col(k-1,0)": lambda: lowered(k, "col", k - 1, 0),
        "row(k-1,k-1)": lambda: lowered(k, "row", k - 1, k - 1),
        "col(k-1,k-1)": lambda: lowered(k, "col", k - 1, k - 1),
        # the first row of a workgroup against the last row of the one before, first and last Q0 lane
        "col(e,0)": lambda: lowered(k, "col", e, 0),
        "col(e,k-1)": lambda: lowered(k, "col", e, k - 1),
        # the last row of a workgroup, and a cell whose left neighbour is in the wave before (k = 128)
        "col(e-1,k/2)": lambda: lowered(k, "col", e - 1, k // 2),
        "row(e,1)": lambda: lowered(k, "row", e, 1),
        "row(k-2,k/2)": lambda: lowered(k, "row", k - 2, k // 2),
        "clean_col": lambda: graded(k, "col"),
        "parity_tail_valid": lambda: parity_tail_valid(k),
        "parity_then_lower(k/2)": lambda: parity_before_boundary_ods(k, k // 2),
        "parity_then_lower(k-1)": lambda: parity_before_boundary_ods(k, k - 1),
    }
    return m


_EXPECT = {}


def expect(oracle, key, make):
    """(status, row roots, column roots, DAH) of the whole-square oracle for the square
    make() builds, computed once per key."""
    if key not in _EXPECT:
        eds = oracle.extend(make())
        rc, rr, cr = oracle.roots(eds, check_order=True)
        _EXPECT[key] = (rc, rr, cr, oracle.dah_hash(rr, cr))
    return _EXPECT[key]


def assert_batch(st, rr, cr, dah, want, what):
    """Status of every square against the oracle's, roots and DAH of the accepted ones."""
    want_st = np.array([w[0] for w in want], np.int32)
    assert np.array_equal(st, want_st), f"{what}: status differs at squares {np.flatnonzero(st != want_st).tolist()}"
    for i, (rc, w_rr, w_cr, w_dah) in enumerate(want):
        if rc == 0:
            assert np.array_equal(rr[i], w_rr) and np.array_equal(cr[i], w_cr), f"{what}: square {i} roots"
            assert dah[i].tobytes() == w_dah, f"{what}: square {i} DAH"


# ------------------------------------------------------------------------------ entry points

def host_batch(ctx, odss, flags):
    """cel_extend_batch from pageable host memory, roots only. Returns (return code, status,
    row roots, column roots, DAHs)."""
    n, k = odss.shape[:2]
    rr = np.zeros((n, 2 * k, NODE), np.uint8)
    cr = np.zeros_like(rr)
    dah = np.zeros((n, 32), np.uint8)
    st = np.full(n, 0x7F7F7F7F, np.int32)
    rc = ctx.lib.cel_extend_batch(ctx.handle, _P(odss), n, k, SHARE, None, _P(rr), _P(cr), _P(dah), _P(st), flags)
    return rc, st, rr, cr, dah


class DevBatch:
    """n squares resident on the device (ODS placed in Q0 of each EDS buffer)."""

    def __init__(self, ctx, n, k):
        from hipmem import DeviceBuffer
        self.ctx, self.n, self.k, w = ctx, n, k, 2 * k
        self.eds_sq = w * w * SHARE
        self.eds = DeviceBuffer(n * self.eds_sq)
        self.rr, self.cr = DeviceBuffer(n * w * NODE), DeviceBuffer(n * w * NODE)
        self.dah, self.st = DeviceBuffer(n * 32), DeviceBuffer(n * 4)
        self.work = DeviceBuffer(ctx.lib.cel_dev_workspace_size(k, n))

    def load(self, odss):
        from hipmem import synchronize
        odss = np.ascontiguousarray(odss)
        assert odss.shape[:3] == (self.n, self.k, self.k)
        self.ctx.check(self.ctx.lib.cel_dev_place_ods(self.ctx.handle, _P(odss), self.n, self.k, self.eds.ptr, None))
        synchronize()

    def run(self, mode, flags, first=0, n=None):
        """mode "pipeline": cel_dev_extend_batch on the internal two-chunk pipeline;
        "caller": the same with CEL_FLAG_CALLER_STREAM (one chunk); "commit": cel_dev_extend_only
        then cel_dev_commit_only. Squares [first, first + n). Returns (status, rr, cr, dah)."""
        from celestia_eds import _lib
        from hipmem import synchronize
        c, k, w = self.ctx, self.k, 2 * self.k
        n = self.n - first if n is None else n
        at = lambda buf, per: ctypes.c_void_p(buf.ptr.value + first * per)
        self.st.upload(np.full(self.n, 0x7F7F7F7F, np.int32))
        eds, rr, cr = at(self.eds, self.eds_sq), at(self.rr, w * NODE), at(self.cr, w * NODE)
        dah, st = at(self.dah, 32), at(self.st, 4)
        if mode == "commit":
            c.check(c.lib.cel_dev_extend_only(c.handle, None, n, k, eds, None))
            c.check(c.lib.cel_dev_commit_only(c.handle, eds, n, k, rr, cr, dah, st, self.work.ptr, None, flags))
        else:
            fl = flags | (_lib.FLAG_CALLER_STREAM if mode == "caller" else 0)
            c.check(c.lib.cel_dev_extend_batch(c.handle, None, n, k, eds, rr, cr, dah, st, self.work.ptr, None, fl))
        synchronize()
        sl = slice(first, first + n)
        return (self.st.download((self.n,), np.int32)[sl], self.rr.download((self.n, w, NODE))[sl],
                self.cr.download((self.n, w, NODE))[sl], self.dah.download((self.n, 32))[sl])


# ------------------------------------------------------------- a. the byte sweep in one batch

SWEEP_CELLS = {(0, 1): "row", (1, 0): "col", (1, 1): "both"}


@pytest.fixture(scope="module")
def sweep(oracle):
    return build_sweep(oracle)


def build_sweep(oracle):
    """k = 2, the smallest square with a row pair and a column pair in Q0: random shares
    with every Q0 namespace byte 0x80, and one square per (cell, kind, byte b in 0..30):
      lower      byte b of the cell 0x7F
      decoy_bad  byte b 0x7F and byte b + 1 0xFF (the later, less significant byte is higher)
      decoy_ok   at (1, 1) only: byte b 0x81 and byte b + 1 0x00 (the later byte is lower)
    Byte 28 is the last namespace byte; 29 (the info byte) and 30 are not part of it. An
    unmodified square goes in after every 24. Returns (squares, their labels, the oracle's
    (status, rr, cr, dah) per square)."""
    k = 2
    base = np.random.default_rng(4202).integers(0, 256, (k, k, SHARE), dtype=np.uint8)
    base[:, :, :NS] = 0x80
    squares, labels = [], []

    def add(ods, label):
        if len(squares) % 25 == 24:
            squares.append(base.copy())
            labels.append(("clean", None, None))
        squares.append(ods)
        labels.append(label)

    for (r, c), kind in SWEEP_CELLS.items():
        for b in range(31):
            lo = base.copy()
            lo[r, c, b] = 0x7F
            add(lo, ("lower", (r, c), b))
            bad = lo.copy()
            bad[r, c, b + 1] = 0xFF
            add(bad, ("decoy_bad", (r, c), b))
            row, col = violations(lo)
            if b < NS:  # the kind of violation each cell makes
                assert (row.any(), col.any()) == (kind != "col", kind != "row")
                assert np.array_equal(violations(bad), (row, col))
    for b in range(31):
        ok = base.copy()
        ok[1, 1, b], ok[1, 1, b + 1] = 0x81, 0x00
        add(ok, ("decoy_ok", (1, 1), b))
    squares.append(base.copy())
    labels.append(("clean", None, None))
    odss = np.stack(squares)
    assert len(odss) > 4 * 21 and len(odss) % 4 != 0  # four host chunks, a short last one
    want = [expect(oracle, ("sweep", i), lambda i=i: odss[i]) for i in range(len(odss))]
    # what the oracle says, as this file's reader expects it
    for (kind, _, b), (rc, _, _, _) in zip(labels, want):
        assert rc == (EORDER if kind in ("lower", "decoy_bad") and b < NS else 0), (kind, b, rc)
    return odss, labels, want


def test_byte_sweep_host_batch(ctx, sweep):
    """One cel_extend_batch call over the whole sweep (four host chunks, the last one short):
    the status array is the oracle's square by square, the call returns CEL_EORDER, and the
    accepted squares carry the oracle's roots and DAH. The same batch without
    CEL_FLAG_ORDER_CHECK: every status is 0."""
    from celestia_eds import _lib
    odss, labels, want = sweep
    rc, st, rr, cr, dah = host_batch(ctx, odss, _lib.FLAG_ORDER_CHECK)
    bad = [labels[i] for i in np.flatnonzero(st != np.array([w[0] for w in want]))]
    assert not bad, f"status differs from the oracle's for {bad}"
    assert_batch(st, rr, cr, dah, want, "host batch")
    assert rc == _lib.EORDER
    rc, st, rr, cr, dah = host_batch(ctx, odss, 0)
    assert rc == _lib.OK and not st.any()
    for i, w in enumerate(want):  # without the check the accepted squares are unchanged
        if w[0] == 0:
            assert np.array_equal(rr[i], w[1]) and np.array_equal(cr[i], w[2]) and dah[i].tobytes() == w[3]


@pytest.mark.parametrize("mode", ["pipeline", "caller", "commit"])
def test_byte_sweep_device_resident(ctx, sweep, mode):
    """The same squares device-resident: cel_dev_extend_batch on the two-chunk pipeline
    (chunk 1 writes its status at d_status + first), with CEL_FLAG_CALLER_STREAM (one chunk),
    and cel_dev_commit_only over EDS buffers that cel_dev_extend_only filled. Status per
    square against the oracle; without the flag every status is 0."""
    from celestia_eds import _lib
    odss, labels, want = sweep
    dev = DevBatch(ctx, len(odss), 2)
    dev.load(odss)
    st, rr, cr, dah = dev.run(mode, _lib.FLAG_ORDER_CHECK)
    bad = [labels[i] for i in np.flatnonzero(st != np.array([w[0] for w in want]))]
    assert not bad, f"{mode}: status differs from the oracle's for {bad}"
    assert_batch(st, rr, cr, dah, want, mode)
    st, _, _, _ = dev.run(mode, 0)
    assert not st.any()


# ----------------------------------------------------------------------------- c. positions

@pytest.mark.parametrize("k", [16, 32])
def test_positions_batched(ctx, oracle, k):
    """Row-only and column-only violations at the corners and edges of Q0 and across leaf
    workgroup edges (k = 16: four workgroups per square; k = 32: one workgroup is four rows),
    parity-namespace shares inside Q0, and valid squares between them, as one host batch and
    one device-resident batch on the two-chunk pipeline."""
    from celestia_eds import _lib
    cases = position_cases(k)
    names = list(cases)
    odss = np.stack([cases[nm]() for nm in names])
    want = [expect(oracle, (k, nm), lambda i=i: odss[i]) for i, nm in enumerate(names)]
    assert {w[0] for w in want} == {0, EORDER}
    rc, st, rr, cr, dah = host_batch(ctx, odss, _lib.FLAG_ORDER_CHECK)
    assert_batch(st, rr, cr, dah, want, f"host {names}")
    assert rc == _lib.EORDER
    dev = DevBatch(ctx, len(names), k)
    dev.load(odss)
    assert_batch(*dev.run("pipeline", _lib.FLAG_ORDER_CHECK), want, f"pipeline {names}")


def test_positions_k128(ctx, oracle):
    """k = 128: a leaf workgroup is one EDS row, so the compare with the row above always
    crosses workgroups. Three squares at a time as one chunk (CEL_FLAG_CALLER_STREAM): past
    the two-waves-per-SIMD bound, the plain leaf kernel k_leaf<true, false>; then every
    square alone (n = 1, the prefetching k_leaf<true, true>)."""
    from celestia_eds import _lib
    k = 128
    cases = position_cases(k)
    names = ["row(0,1)", "col(1,0)", "clean_row", "row(0,k-1)", "col(k-1,0)", "col(k-1,k-1)", "row(k-1,k-1)",
             "col(e,k-1)", "row(k-2,k/2)", "parity_then_lower(k/2)", "parity_tail_valid", "col(e-1,k/2)"]
    dev = DevBatch(ctx, 3, k)
    for g in range(0, len(names), 3):
        grp = names[g:g + 3]
        odss = np.stack([cases[nm]() for nm in grp])
        want = [expect(oracle, (k, nm), lambda i=i: odss[i]) for i, nm in enumerate(grp)]
        dev.load(odss)
        assert_batch(*dev.run("caller", _lib.FLAG_ORDER_CHECK), want, f"n=3 {grp}")
        for i in range(3):
            assert_batch(*dev.run("pipeline", _lib.FLAG_ORDER_CHECK, first=i, n=1), want[i:i + 1], f"n=1 {grp[i]}")


# -------------------------------------------------------------------- d. the one-square paths

def _pinned(ctx, shape):
    nbytes = int(np.prod(shape))
    p = ctx.lib.cel_host_alloc(nbytes)
    assert p, "cel_host_alloc failed"
    return p, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p)).reshape(shape)


def _one_square(ctx, ods, flags):
    """cel_extend_batch with n = 1, roots only: (return code, status, rr, cr, dah)."""
    k = ods.shape[0]
    rr, cr = np.zeros((2 * k, NODE), np.uint8), np.zeros((2 * k, NODE), np.uint8)
    dah, st = np.zeros(32, np.uint8), np.full(1, 0x7F7F7F7F, np.int32)
    rc = ctx.lib.cel_extend_batch(ctx.handle, ctypes.c_void_p(ods.ctypes.data), 1, k, SHARE, None, _P(rr), _P(cr),
                                  _P(dah), _P(st), flags)
    return rc, st, rr[None], cr[None], dah[None]


@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("k", [32, 128])
def test_one_square_paths(ctx, oracle, k, mem):
    """cel_extend_batch with n = 1 (api.cpp's one-square path): from pageable memory the ODS
    is copied up first; from cel_host_alloc memory the row pass reads the mapped host pages.
    A column-only violation in the last Q0 row, a row-only one in row 0, then a valid square."""
    from celestia_eds import _lib
    cases = position_cases(k)
    p, buf = _pinned(ctx, (k, k, SHARE)) if mem == "pinned" else (None, np.zeros((k, k, SHARE), np.uint8))
    try:
        for nm in ("col(k-1,k-1)", "row(0,1)", "clean_col"):
            buf[...] = cases[nm]()
            want = expect(oracle, (k, nm), lambda: np.array(buf))
            rc, st, rr, cr, dah = _one_square(ctx, buf, _lib.FLAG_ORDER_CHECK)
            assert_batch(st, rr, cr, dah, [want], f"{mem} {nm}")
            assert rc == want[0] == (0 if nm == "clean_col" else EORDER)
    finally:
        if p:
            ctx.lib.cel_host_free(p)


def test_one_square_k512_chunk_boundaries(ctx):
    """k = 512 from page-locked memory: the ODS crosses PCIe in four row chunks, and the
    push-order check of a chunk's first row reads the row the chunk before brought
    (test_gpu_square.test_pinned_single_square breaks rows 127 / 128). Here: column order
    broken only across rows 255 / 256, only across 383 / 384, and a row-only violation inside
    the last chunk. Three calls. The expectation is by construction, asserted with numpy byte
    compares (`violations`), not by the oracle, whose k = 512 run takes seconds."""
    from celestia_eds import _lib
    k = 512
    p, buf = _pinned(ctx, (k, k, SHARE))
    try:
        buf[...] = graded(k, "row")
        assert not any(v.any() for v in violations(buf))
        for b in (256, 384):
            # row b takes row 0's namespaces: still constant along the row, below row b - 1 in every column
            keep = buf[b, :, :NS].copy()
            buf[b, :, :NS] = buf[0, :, :NS]
            row, col = violations(buf)
            assert not row.any() and col[b].all() and not np.delete(col, b, axis=0).any()
            rc, st, _, _, _ = _one_square(ctx, buf, _lib.FLAG_ORDER_CHECK)
            assert rc == _lib.EORDER and st[0] == _lib.EORDER, f"rows {b - 1} / {b}"
            buf[b, :, :NS] = keep
        r, c = 400, 300  # the cell takes the grade of the row above: below its left neighbour only
        buf[r, c, :NS] = buf[r - 1, c, :NS]
        row, col = violations(buf)
        assert row.sum() == 1 and row[r, c] and not col.any()
        rc, st, _, _, _ = _one_square(ctx, buf, _lib.FLAG_ORDER_CHECK)
        assert rc == _lib.EORDER and st[0] == _lib.EORDER, "row-only violation in the last chunk"
    finally:
        ctx.lib.cel_host_free(p)


# -------------------------------------------------------------------------------- e. sharded

@pytest.fixture(scope="module")
def ctxs():
    """Eight contexts on device 0 (ctx[0] is the session's default one)."""
    from celestia_eds import Context, default_context
    cs = [default_context(0)] + [Context(0) for _ in range(7)]
    yield cs
    for c in cs[1:]:
        c.close()


SHARD_K = 256  # the smallest sharded width
SHARD_CASES = {
    # inside a slab at every n: the slab's own leaf compare
    "row_in_slab": lambda k: lowered(k, "row", 5, 3),
    "col_first_slab": lambda k: lowered(k, "col", 7, 1),
    "col_last_q0_slab": lambda k: lowered(k, "col", 9, k - 1),
    # a cell below its left neighbour at every column that can be a slab boundary inside Q0
    # (n = 4: k/2; n = 8: k/4, k/2, 3k/4): the finish's compare of gathered records
    "row_at_k/4": lambda k: lowered(k, "row", 11, k // 4),
    "row_at_k/2": lambda k: lowered(k, "row", 11, k // 2),
    "row_at_3k/4": lambda k: lowered(k, "row", 11, 3 * k // 4),
    # 0xFF*29 just before the boundary, a lower namespace after it: IgnoreMaxNamespace keeps
    # 0xFF*29 out of the left slab's maxNs
    "parity_before_k/4": lambda k: parity_before_boundary_ods(k, k // 4),
    "parity_before_k/2": lambda k: parity_before_boundary_ods(k, k // 2),
    "parity_before_3k/4": lambda k: parity_before_boundary_ods(k, 3 * k // 4),
    "parity_tail_valid": parity_tail_valid,
}


@pytest.mark.parametrize("n,case", [(n, c) for n in (1, 2, 4, 8) for c in SHARD_CASES])
def test_sharded(ctxs, oracle, n, case):
    """cel_extend_sharded over n ranks, k = 256: the oracle's status for the case, then a
    valid square (namespaces equal across every slab boundary; at n = 2 the only boundary is
    column k, where Q1 begins and nothing is compared) succeeds on the same ctxs with the
    oracle's roots and DAH."""
    from celestia_eds import CelError
    from celestia_eds.multi import extend_sharded
    k = SHARD_K
    ods = SHARD_CASES[case](k)
    rc, w_rr, w_cr, w_dah = expect(oracle, (k, "shard", case), lambda: ods)
    assert rc == (0 if case == "parity_tail_valid" else EORDER)
    if rc:
        with pytest.raises(CelError) as e:
            extend_sharded(ctxs[:n], ods, want_eds=False)
        assert e.value.status == rc
    else:
        _, rr, cr, dah = extend_sharded(ctxs[:n], ods, want_eds=False)
        assert np.array_equal(rr, w_rr) and np.array_equal(cr, w_cr) and dah == w_dah
    valid = graded(k, "row")
    rc, w_rr, w_cr, w_dah = expect(oracle, (k, "shard", "valid"), lambda: valid)
    assert rc == 0
    _, rr, cr, dah = extend_sharded(ctxs[:n], valid, want_eds=False)
    assert np.array_equal(rr, w_rr) and np.array_equal(cr, w_cr) and dah == w_dah
