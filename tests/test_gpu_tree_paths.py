"""GPU: the tree paths that share one level step and one reducer, at the shapes where a shared
reducer can go wrong.

Every NMT root of a square can be had four ways: the EDS commit (k_leaf, k_level, the root
level packs the roots), cel_axis_root (one tree, k_reduce_pass), cel_axis_trees (every level
kept, the strided level kernel level by level) and the repair's roots of gathered axes (the
strided level kernel through the reducer's ping / pong buffers). At k = 1 the first level is
the root level and nothing goes through ping or pong, k = 2 is one ping, k = 4 ping and pong.

The row-sharded finish reduces the ranks' row subtrees through the same reducer: one rank
copies, two ranks are one level, four ranks two levels. The device steps admit k = 256 and 512
and at most k ranks (cel_dev_shard_*: validate_shard), so a slab is at least two cells wide and
k = 256 is the smallest square this path can be run at; launch_slab_trees' one-cell-wide copy
(w == 1) cannot be reached through the C ABI.
"""
import numpy as np
import pytest

from eds_inputs import random_ods

pytestmark = pytest.mark.gpu

_SQUARES = {}


def square(ctx, oracle, k):
    """(oracle eds, oracle row roots, oracle column roots, the device commit) of one random
    square with sorted Q0 namespaces per width, computed once and never written."""
    if k not in _SQUARES:
        from celestia_eds import da
        ods = random_ods(k, 4100 + k)
        eds, rr, cr, dah = oracle.extend_and_commit(ods)
        for a in (eds, rr, cr):
            a.setflags(write=False)
        _SQUARES[k] = (eds, rr, cr, dah, da._extend(ods.reshape(-1, 512), ctx=ctx))
    return _SQUARES[k]


@pytest.mark.parametrize("k", [1, 2, 4])
def test_commit_roots_equal_oracle(ctx, oracle, k):
    eds, rr, cr, dah, dev = square(ctx, oracle, k)
    assert np.array_equal(dev.cells, eds)
    assert np.array_equal(dev._row_roots, rr) and np.array_equal(dev._col_roots, cr)
    assert dev._dah == dah


@pytest.mark.parametrize("k", [1, 2, 4])
def test_axis_root_equals_commit_and_oracle(ctx, oracle, k):
    import ctypes
    from celestia_eds import _lib
    eds, rr, cr, _, dev = square(ctx, oracle, k)
    for axis, want, got_commit in ((0, rr, dev._row_roots), (1, cr, dev._col_roots)):
        for i in range(2 * k):
            cells = np.ascontiguousarray(eds[i] if axis == 0 else eds[:, i])
            out = np.zeros(_lib.NMT_NODE_SIZE, np.uint8)
            ctx.check(ctx.lib.cel_axis_root(ctx.handle, cells.ctypes.data_as(ctypes.c_void_p), k, i, _lib.SHARE_SIZE,
                                            out.ctypes.data_as(ctypes.c_void_p), 0))
            assert np.array_equal(out, want[i]), (axis, i)
            assert np.array_equal(out, got_commit[i]), (axis, i)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_axis_trees_top_equals_commit_and_oracle(ctx, oracle, k):
    """The last record of every exported tree is its root: one tree per call (count = 1, every
    first) and all 2k trees in one call."""
    from celestia_eds.proof import axis_trees
    _, rr, cr, _, dev = square(ctx, oracle, k)
    w = 2 * k
    for axis, want, got_commit in ((0, rr, dev._row_roots), (1, cr, dev._col_roots)):
        every = axis_trees(dev, axis, 0, w, ctx=ctx)
        assert every.shape == (w, 2 * w - 1, 90)
        assert np.array_equal(every[:, -1], want) and np.array_equal(every[:, -1], got_commit), axis
        for i in range(w):
            one = axis_trees(dev, axis, i, 1, ctx=ctx)
            assert np.array_equal(one[0], every[i]), (axis, i)


@pytest.mark.parametrize("k", [2, 4])
def test_byzantine_repair_small_width(ctx, oracle, k):
    """Below 2k = 32 the repair decodes gathered axes, and a byzantine square is replayed in
    sweep order (repair_exact): gather, encoding check, the roots of the gathered axes through
    the reducer, their records (rows, then columns) kept after the axes-roots workspace.

    Rows 0, 1 and 2k - 1 and column 1 are incomplete; rows 0 and 1 are clean and the corrupt
    cell (2k - 1, 1) is present. The sweep solves row 0 and row 1, whose computed roots must
    equal the given ones, before row 1's solve completes column 1, whose re-encoding fails:
    the answer is column 1 only if both earlier root records are right and the column pass
    left the row records alone. A wrong record would name row 0 or row 1 instead, which is
    what the same square does when the given root of row 0 or row 1 is the stale one. Status,
    axis and index, the shares and the mask equal the oracle's rsmt2d restatement."""
    from celestia_eds import _lib
    from test_gpu_repair import _assert_same_outcome
    eds, rr, cr, _, _ = square(ctx, oracle, k)
    w = 2 * k
    present = np.ones((w, w), np.uint8)
    present[0, 1] = present[1, 1] = present[w - 1, w - 1] = 0
    bad = eds.copy()
    bad[w - 1, 1, 200] ^= 0x40
    cols = [c.tobytes() for c in cr]
    for stale, want in ((None, (1, 1)), (0, (0, 0)), (1, (0, 1))):
        rows = rr.copy()
        if stale is not None:
            rows[stale, 60] ^= 1
        st, axis, _, _ = _assert_same_outcome(ctx, oracle, bad, present, [r.tobytes() for r in rows], cols)
        assert st == _lib.EBYZANTINE and axis == want, (stale, st, axis)


@pytest.mark.parametrize("nranks", [1, 2, 4])
def test_sharded_finish_equals_unsharded_commit(ctx, oracle, nranks):
    """The finish's reduce of the ranks' row subtrees: one rank (copy), two (one level into the
    roots), four (ping, then the roots), all ranks in one process. Roots and DAH of every rank
    equal the unsharded commit's."""
    import torch
    from celestia_eds import da
    from celestia_eds.sharded import DeviceSteps, LocalComm, ShardedSquare
    k = 256
    if "sharded" not in _SQUARES:
        ods = random_ods(k, 4100 + k)
        _SQUARES["sharded"] = (ods, da._extend(ods.reshape(-1, 512), ctx=ctx))
    ods, whole = _SQUARES["sharded"]
    steps = DeviceSteps(ctx)
    squares = [ShardedSquare(k, r, nranks, steps) for r in range(nranks)]
    for s in squares:
        a, b = s.row_range()
        s.ods_rows.copy_(torch.from_numpy(np.ascontiguousarray(ods[a:b])))
    LocalComm.run(squares)
    steps.stream.synchronize()
    for s in squares:
        assert int(s.status.item()) == 0
        assert np.array_equal(s.row_roots.cpu().numpy(), whole._row_roots)
        assert np.array_equal(s.col_roots.cpu().numpy(), whole._col_roots)
        assert s.dah.cpu().numpy().tobytes() == whole._dah
