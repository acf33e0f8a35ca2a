"""CPU: the merged pass schedule of a batch repair (cel_debug_repair_batch_plan, host-only).
cel_dev_repair_batch runs every square's crossword passes together: global pass (round r, rows)
is every square's row list of round r, then the columns. Five mixed masks per width (the
splitmix masks of test_repair_plan_check.py at p = 0.5, 0.55 and 0.3, all present, one
quadrant), W = 4, 64, 256:
  - each square's projection of the merged passes is its own pass list, worked out here in
    numpy by the pass rule (an axis with k <= known cells < 2k gets all of them);
  - every entry names a square below n and an axis below W, and no axis of a square is listed
    twice in a direction;
  - a complete square, and one stuck at the start, are in no pass."""
import ctypes

import numpy as np
import pytest

from test_repair_plan_check import _random_mask


def _batch_plan(masks, k):
    from celestia_eds import _lib
    lib = _lib.load()
    n = len(masks)
    m = np.ascontiguousarray(np.stack(masks), np.uint8)
    dirs = np.full(8 * k, -1, np.int32)
    off = np.zeros(8 * k + 1, np.uint32)
    sq = np.full(n * 4 * k, 0xFFFFFFFF, np.uint32)
    ax = np.full(n * 4 * k, -1, np.int32)
    npass = ctypes.c_uint32(0)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.cel_debug_repair_batch_plan(P(m), n, k, P(dirs), P(off), ctypes.byref(npass), P(sq), P(ax)) == _lib.OK
    np_ = npass.value
    return [(int(dirs[p]), [(int(s), int(a)) for s, a in zip(sq[off[p]:off[p + 1]], ax[off[p]:off[p + 1]])])
            for p in range(np_)], int(off[np_])


def _own_passes(mask):
    """(direction, axes) of every pass of one square: rows, then columns, until none is solvable."""
    m = mask.astype(bool).copy()
    w = m.shape[0]
    out = []
    while True:
        progress = False
        for d in (0, 1):
            cnt = m.sum(axis=1 - d)
            sel = np.flatnonzero((cnt >= w // 2) & (cnt < w))
            if sel.size == 0:
                continue
            if d == 0:
                m[sel, :] = True
            else:
                m[:, sel] = True
            out.append((d, sel.tolist()))
            progress = True
        if not progress:
            return out


def _masks(w):
    k = w // 2
    quad = np.zeros((w, w), bool)
    quad[:k, :k] = True
    seed = 0xC0FFEE + w * 1000
    return [_random_mask(w, seed + 10, 0.5), np.ones((w, w), bool), _random_mask(w, seed + 21, 0.55),
            _random_mask(w, seed + 2, 0.3), quad]


@pytest.mark.parametrize("w", [4, 64, 256])
def test_merged_schedule_projects_onto_each_square(w):
    masks = _masks(w)
    n, k = len(masks), w // 2
    passes, nent = _batch_plan(masks, k)
    assert nent == sum(len(e) for _, e in passes)
    proj = [[] for _ in range(n)]
    seen = set()
    for d, entries in passes:
        assert d in (0, 1) and entries
        assert entries == sorted(entries)  # squares ascending, a square's axes ascending
        for s, a in entries:
            assert 0 <= s < n and 0 <= a < w
            assert (s, d, a) not in seen
            seen.add((s, d, a))
        for s in sorted({s for s, _ in entries}):
            proj[s].append((d, [a for t, a in entries if t == s]))
    own = [_own_passes(m) for m in masks]
    assert proj == own
    assert own[1] == []  # complete
    if w >= 64:  # p = 0.3: no axis holds k cells; the others do solve
        assert own[3] == [] and all(own[i] for i in (0, 2, 4))
    assert len(own[4]) == 2  # one quadrant: its rows, then every column


def test_rejects_bad_arguments():
    from celestia_eds import _lib
    lib = _lib.load()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    m = np.ones((2, 4, 4), np.uint8)
    a = np.zeros(64, np.int32)
    u = np.zeros(64, np.uint32)
    npass = ctypes.c_uint32(0)
    assert lib.cel_debug_repair_batch_plan(None, 2, 2, P(a), P(u), ctypes.byref(npass), P(u), P(a)) == _lib.EINVAL
    assert lib.cel_debug_repair_batch_plan(P(m), 2, 3, P(a), P(u), ctypes.byref(npass), P(u), P(a)) == _lib.EINVAL
    assert lib.cel_debug_repair_batch_plan(P(m), 0, 2, P(a), P(u), ctypes.byref(npass), P(u), P(a)) == _lib.EINVAL
    assert lib.cel_dev_repair_batch_scratch_size(3, 4) == 0 and lib.cel_dev_repair_batch_scratch_size(32, 0) == 0
    # the batch's scratch grows with n; one square, or a k outside the merged path, is the single repair's
    s1, s2, s8 = (lib.cel_dev_repair_batch_scratch_size(32, n) for n in (1, 2, 8))
    assert 0 < s1 < s2 < s8
    assert lib.cel_dev_repair_batch_scratch_size(16, 8) == lib.cel_dev_repair_batch_scratch_size(16, 1)
