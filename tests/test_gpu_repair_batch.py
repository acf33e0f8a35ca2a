"""GPU: the repair of many squares in one call (cel_dev_repair_batch, cel_repair_batch,
rsmt2d.RepairBatch). For k = 32, 64, 128 the squares' crossword passes are merged (one decode
and one check launch per pass over every square, one commit, one copy back); any other k, and
n = 1, runs the single repair square after square. Every square of every batch must come out
as the oracle's rsmt2d restatement and as cel_dev_repair on that square alone: status, mask,
failing axis and index, ErrByzantineData.Shares with their mask, and every cell the mask
vouches for. Outcomes are exact bytes."""
import ctypes

import numpy as np
import pytest

from hipmem import DeviceBuffer
from test_gpu_repair import _byz_case, _crossword_passes, _dev_repair, _oracle_repair, _stack, setup

pytestmark = pytest.mark.gpu

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
_setups = {}


def _setup(oracle, k, seed):
    """(eds, row roots, column roots) of a random ODS, extended once per (k, seed); never written."""
    if (k, seed) not in _setups:
        _setups[k, seed] = setup(oracle, k, seed=seed)
    return _setups[k, seed]


def _random(w, seed, p):
    return (np.random.default_rng(seed).random((w, w)) < p).astype(np.uint8)


def _q0(w):
    m = np.zeros((w, w), np.uint8)
    m[:w // 2, :w // 2] = 1
    return m


class Result:
    """One square's outcome: status, cells, (bad axis, bad index), Shares, their mask, the mask."""

    def __init__(self, st, cells, bad, bs, bp, pres):
        self.st, self.cells, self.bad, self.bs, self.bp, self.pres = int(st), cells, bad, bs, bp, pres


class Results(list):
    """The squares' outcomes; `error`: cel_last_error after the call, where a test reads it."""
    error = None


def _inputs(cases, rng=None):
    """cases: (eds, present, rr, cr) each. The damaged squares (absent cells zero, or random
    bytes from rng), masks and roots as the batch call takes them."""
    eds = np.stack([np.where(p[..., None] == 1, e, 0 if rng is None else rng.integers(0, 256, e.shape, dtype=np.uint8))
                    for e, p, _, _ in cases]).astype(np.uint8)
    pres = np.ascontiguousarray(np.stack([p for _, p, _, _ in cases]), np.uint8).copy()
    rr = np.ascontiguousarray(np.stack([_stack(r) for _, _, r, _ in cases]))
    cr = np.ascontiguousarray(np.stack([_stack(c) for _, _, _, c in cases]))
    return np.ascontiguousarray(eds), pres, rr, cr


def _results(n, w, status, cells, ba, bi, bs, bp, pres):
    return Results(Result(status[i], cells[i], (int(ba[i]), int(bi[i])), bs[i], bp[i], pres[i]) for i in range(n))


def _dev_repair_batch(ctx, cases, rng=None, host=False):
    """cel_dev_repair_batch over device-resident damaged copies (host: cel_repair_batch over
    host squares); one Result per square."""
    from celestia_eds import _lib
    n, w = len(cases), cases[0][0].shape[0]
    eds, pres, rr, cr = _inputs(cases, rng)
    status = np.full(n, -7, np.int32)
    ba, bi = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    bs = np.zeros((n, w, 512), np.uint8)
    bp = np.zeros((n, w), np.uint8)
    if host:
        st = ctx.lib.cel_repair_batch(ctx.handle, P(eds), P(pres), n, w // 2, 512, P(rr), P(cr), P(status), P(ba), P(bi),
                                      P(bs), P(bp))
        cells = eds
    else:
        d = DeviceBuffer(eds.nbytes)
        d.upload(eds)
        st = ctx.lib.cel_dev_repair_batch(ctx.handle, d.ptr, P(pres), n, w // 2, P(rr), P(cr), P(status), P(ba), P(bi),
                                          P(bs), P(bp))
        cells = d.download(eds.shape)
        d.free()
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle)
    return _results(n, w, status, cells, ba, bi, bs, bp, pres)


def _single(ctx, case):
    st, cells, bad, (bs, bp, pres) = _dev_repair(ctx, *case, want_shares=True)
    return Result(st, cells, bad, bs, bp, pres)


def _assert_same(got, ref, what):
    """Two device outcomes of one square: everything the ABI defines is equal."""
    from celestia_eds import _lib
    assert got.st == ref.st, (what, got.st, ref.st)
    assert np.array_equal(got.pres, ref.pres), what
    if ref.st in (_lib.EBYZANTINE, _lib.EBADROOT):
        assert got.bad == ref.bad, (what, got.bad, ref.bad)
    else:
        assert got.bad == (-1, -1), (what, got.bad)
    if ref.st == _lib.EBYZANTINE:
        assert np.array_equal(got.bp, ref.bp), what
        assert np.array_equal(got.bs[got.bp == 1], ref.bs[ref.bp == 1]), what
    assert np.array_equal(got.cells[got.pres == 1], ref.cells[ref.pres == 1]), what


def _assert_oracle(oracle, got, case, what):
    """_assert_same_outcome of test_gpu_repair.py for one square of a batch; the oracle's status."""
    from celestia_eds import _lib
    eds = case[0]
    rc, ocells, opres, obad, (obs, obp) = _oracle_repair(oracle, *case)
    assert got.st == rc, (what, got.st, rc)
    if rc in (_lib.EBYZANTINE, _lib.EBADROOT):
        assert got.bad == obad, (what, got.bad, obad)
    if rc == _lib.EBYZANTINE:
        assert np.array_equal(got.bp, obp), what
        assert np.array_equal(got.bs[got.bp == 1], obs[obp == 1]), what
    assert np.array_equal(got.pres, opres), what
    if rc == _lib.OK:
        assert np.array_equal(got.cells, eds), what
    else:
        assert np.array_equal(got.cells[got.pres == 1], ocells[opres == 1]), what
    return rc


def _check_batch(ctx, oracle, cases):
    """The batch against the oracle and against cel_dev_repair square by square; the statuses."""
    got = _dev_repair_batch(ctx, cases)
    got.error = ctx.lib.cel_last_error(ctx.handle).decode()  # before the single repairs leave theirs
    rcs = []
    for i, case in enumerate(cases):
        rcs.append(_assert_oracle(oracle, got[i], case, f"square {i} vs oracle"))
        _assert_same(got[i], _single(ctx, case), f"square {i} vs cel_dev_repair")
    return rcs, got


def _mixed_cases(oracle):
    """k = 32, n = 7: all present, Q0 only, nine passes, stuck after three, stuck at once, and
    two byzantine squares (in the second rsmt2d's sweep order differs from the pass order)."""
    k, w = 32, 64
    block = np.ones((w, w), np.uint8)
    block[:k + 1, :k + 1] = 0  # (k+1) x (k+1) missing: no axis through it keeps k cells
    masks = [np.ones((w, w), np.uint8), _q0(w), _random(w, 13, 0.40), _random(w, 15, 0.40), block]
    assert _crossword_passes(masks[1], k) == (2, True)
    assert _crossword_passes(masks[2], k) == (9, True)
    assert _crossword_passes(masks[3], k) == (3, False)
    assert _crossword_passes(masks[4], k) == (0, False)
    cases = [_setup(oracle, k, 3 + i)[:1] + (m,) + _setup(oracle, k, 3 + i)[1:] for i, m in enumerate(masks)]
    return cases + [_byz_case(oracle, k, 0), _byz_case(oracle, k, 2)]


def test_mixed_batch_k32(ctx, oracle):
    from celestia_eds import _lib
    cases = _mixed_cases(oracle)
    rcs, got = _check_batch(ctx, oracle, cases)
    assert {_lib.OK, _lib.EUNREPAIRABLE, _lib.EBYZANTINE} <= set(rcs)  # no branch lost to a change of inputs
    assert rcs[:5] == [_lib.OK, _lib.OK, _lib.OK, _lib.EUNREPAIRABLE, _lib.EUNREPAIRABLE]
    # the first failing square's message, with its index
    assert got.error == "square 3: failed to solve data square"


def test_schedule_fuzz_k32(ctx, oracle):
    """Random idle kernels (0..60 us) in front of every operation the batch enqueues on its
    two streams: a missing cross-stream dependency would change an outcome."""
    from celestia_eds import _lib
    cases = _mixed_cases(oracle)
    ref = _dev_repair_batch(ctx, cases)
    try:
        for fseed in range(4):
            assert ctx.lib.cel_debug_schedule_fuzz(ctx.handle, 2000 + fseed, 60) == _lib.OK
            got = _dev_repair_batch(ctx, cases)
            for i in range(len(cases)):
                _assert_same(got[i], ref[i], f"fuzz seed {fseed}, square {i}")
    finally:
        ctx.lib.cel_debug_schedule_fuzz(ctx.handle, 0, 0)


def test_bad_root_is_isolated_k32(ctx, oracle):
    """The middle square has a complete row whose expected root has one byte flipped: it alone
    returns EBADROOT (row 5); its neighbours are repaired to their original squares."""
    from celestia_eds import _lib
    k, w = 32, 64
    a, b, c = (_setup(oracle, k, s) for s in (3, 4, 5))
    rr = list(b[1])
    rr[5] = rr[5][:17] + bytes([rr[5][17] ^ 0x04]) + rr[5][18:]
    mid = np.ones((w, w), np.uint8)
    mid[0, 9] = 0
    cases = [(a[0], _q0(w), a[1], a[2]), (b[0], mid, rr, b[2]), (c[0], _random(w, 8, 0.6), c[1], c[2])]
    rcs, got = _check_batch(ctx, oracle, cases)
    assert rcs == [_lib.OK, _lib.EBADROOT, _lib.OK] and got[1].bad == (0, 5)
    assert np.array_equal(got[0].cells, a[0]) and np.array_equal(got[2].cells, c[0])


def test_entry_limits_k32(ctx, oracle):
    """The highest square index with the highest axis index of the entry format: only the last
    of four squares is damaged, missing its last column and its last row (the rows solve, then
    every column, column 2k-1 among them). The undamaged squares hold their true bytes on the
    device and must come back whole: no store strays into another square."""
    from celestia_eds import _lib
    k, w = 32, 64
    sq = [_setup(oracle, k, 3 + i) for i in range(4)]
    last = np.ones((w, w), np.uint8)
    last[:, w - 1] = 0
    last[w - 1, :] = 0
    assert _crossword_passes(last, k) == (2, True)
    cases = [(s[0], np.ones((w, w), np.uint8), s[1], s[2]) for s in sq[:3]] + [(sq[3][0], last, sq[3][1], sq[3][2])]
    rcs, got = _check_batch(ctx, oracle, cases)
    assert rcs == [_lib.OK] * 4
    for i in range(4):
        assert np.array_equal(got[i].cells, sq[i][0]), i


def test_batch_k128(ctx, oracle):
    """The <8> decode instantiation (W = 256): five passes, a p = 0.55 mask, a byzantine square."""
    from celestia_eds import _lib
    k, w = 128, 256
    eds, rr, cr = _setup(oracle, k, 3)
    m = _random(w, 1, 0.44)
    assert _crossword_passes(m, k) == (5, True)
    cases = [(eds, m, rr, cr), (eds, _random(w, 7, 0.55), rr, cr), _byz_case(oracle, k, 0)]
    rcs, _ = _check_batch(ctx, oracle, cases)
    assert rcs == [_lib.OK, _lib.OK, _lib.EBYZANTINE]


def test_batch_k64(ctx, oracle):
    from celestia_eds import _lib
    k, w = 64, 128
    cases = [_setup(oracle, k, 3 + i)[:1] + (_random(w, 20 + i, 0.55),) + _setup(oracle, k, 3 + i)[1:] for i in range(2)]
    rcs, _ = _check_batch(ctx, oracle, cases)
    assert rcs == [_lib.OK, _lib.OK]


@pytest.mark.parametrize("k", [8, 16])
def test_fallback_small_k(ctx, oracle, k):
    """A k outside the in-square kernels runs the single repair square after square."""
    w = 2 * k
    a, b = _setup(oracle, k, 3), _setup(oracle, k, 4)
    cases = [(a[0], _random(w, 5, 0.6), a[1], a[2]), _byz_case(oracle, k, 0), (b[0], _q0(w), b[1], b[2])]
    got = _dev_repair_batch(ctx, cases)
    for i, case in enumerate(cases):
        _assert_same(got[i], _single(ctx, case), f"square {i}")


def test_n1_and_n0(ctx, oracle):
    from celestia_eds import _lib
    k, w = 32, 64
    case = _byz_case(oracle, k, 2)
    got = _dev_repair_batch(ctx, [case])
    _assert_same(got[0], _single(ctx, case), "n = 1")
    eds, pres, rr, cr = _inputs([case])
    d = DeviceBuffer(eds.nbytes)
    d.upload(eds)
    before = pres.copy()
    status, ba, bi = (np.full(1, -7, np.int32) for _ in range(3))
    assert ctx.lib.cel_dev_repair_batch(ctx.handle, d.ptr, P(pres), 0, k, P(rr), P(cr), P(status), P(ba), P(bi),
                                        None, None) == _lib.OK
    assert status[0] == ba[0] == bi[0] == -7 and np.array_equal(pres, before)
    assert np.array_equal(d.download(eds.shape), eds)
    d.free()


def test_bad_arguments(ctx, oracle):
    from celestia_eds import _lib
    k = 32
    eds, pres, rr, cr = _inputs([_byz_case(oracle, k, 0)] * 2)
    d = DeviceBuffer(eds.nbytes)
    d.upload(eds)
    status, ba, bi = (np.full(2, -7, np.int32) for _ in range(3))
    call = lambda present, kk, st: ctx.lib.cel_dev_repair_batch(ctx.handle, d.ptr, present, 2, kk, P(rr), P(cr), st,
                                                                P(ba), P(bi), None, None)
    assert call(P(pres), k, None) == _lib.EINVAL
    assert call(None, k, P(status)) == _lib.EINVAL
    assert call(P(pres), 24, P(status)) == _lib.EINVAL
    # refused before any device work: nothing written anywhere
    assert (status == -7).all() and (ba == -7).all() and np.array_equal(d.download(eds.shape), eds)
    d.free()


def test_host_entry_k32(ctx, oracle):
    k, w = 32, 64
    a = _setup(oracle, k, 4)
    cases = [(a[0], _random(w, 13, 0.40), a[1], a[2]), _byz_case(oracle, k, 0), (a[0], _random(w, 15, 0.40), a[1], a[2])]
    dev, host = _dev_repair_batch(ctx, cases), _dev_repair_batch(ctx, cases, host=True)
    for i in range(3):
        _assert_same(host[i], dev[i], f"square {i}")


def test_missing_cells_hold_garbage_k32(ctx, oracle):
    """Absent cells may hold anything: random bytes there change no outcome."""
    k, w = 32, 64
    a = _setup(oracle, k, 5)
    cases = [(a[0], _random(w, 32, 0.6), a[1], a[2]), (a[0], _random(w, 15, 0.40), a[1], a[2]), _byz_case(oracle, k, 0)]
    zeros, junk = _dev_repair_batch(ctx, cases), _dev_repair_batch(ctx, cases, rng=np.random.default_rng(9))
    for i in range(3):
        _assert_same(junk[i], zeros[i], f"square {i}")
    from celestia_eds import _lib
    assert [r.st for r in zeros] == [_lib.OK, _lib.EUNREPAIRABLE, _lib.EBYZANTINE]
    assert np.array_equal(junk[0].cells, a[0])


def test_python_repair_batch(ctx, oracle):
    from celestia_eds import CelError, _lib
    from celestia_eds.rsmt2d import (ErrByzantineData, ErrUnrepairableDataSquare, ExtendedDataSquare, RepairBatch)
    cases = _mixed_cases(oracle)
    damaged = [np.where(p[..., None] == 1, e, 0).astype(np.uint8) for e, p, _, _ in cases]
    out = RepairBatch([ExtendedDataSquare(d, ctx=ctx) for d in damaged], [c[2] for c in cases], [c[3] for c in cases],
                      presents=[c[1] for c in cases], ctx=ctx)
    kinds = [ExtendedDataSquare] * 3 + [ErrUnrepairableDataSquare] * 2 + [ErrByzantineData] * 2
    assert [type(o) for o in out] == kinds
    for i in range(3):
        assert np.array_equal(out[i].cells, cases[i][0]) and out[i]._mask.all()
    for i in (5, 6):
        sq = ExtendedDataSquare(damaged[i].copy(), ctx=ctx)
        with pytest.raises(ErrByzantineData) as ei:
            sq.Repair(cases[i][2], cases[i][3], present=cases[i][1])
        e = ei.value
        assert (out[i].Axis, out[i].Index, out[i].Shares) == (e.Axis, e.Index, e.Shares)
        assert str(out[i]) == str(e)
        # the most-repaired square and its mask, as Repair leaves them on self
        assert np.array_equal(out[i].square._mask, sq._mask)
        assert np.array_equal(out[i].square.cells[sq._mask == 1], sq.cells[sq._mask == 1])
    # a bad root comes back as CelError(EBADROOT), not raised
    eds, rr, cr = _setup(oracle, 32, 4)
    rr = [bytes(90)] + list(rr[1:])
    out = RepairBatch([eds, eds], [rr, _setup(oracle, 32, 4)[1]], [cr, cr], ctx=ctx)
    assert type(out[0]) is CelError and out[0].status == _lib.EBADROOT and "bad root input: row 0" in str(out[0])
    assert isinstance(out[1], ExtendedDataSquare)
    assert RepairBatch([], [], [], ctx=ctx) == []
