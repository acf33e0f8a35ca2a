"""GPU: sampled cells with single-leaf NMT proofs, verified on the device and placed into a
resident square (cel_dev_place_samples), and the repair from them (cel_repair_samples through
rsmt2d.RepairFromSamples). The verdicts are checked against the host mirror in
celestia_eds/proof.py, the cells and roots against the oracle."""
import numpy as np
import pytest

import nmt_ref
import verify_cases as vc
from eds_inputs import random_ods

pytestmark = pytest.mark.gpu

PARITY = b"\xff" * 29
ROW, COL = 0, 1


class Square:
    """An EDS (any cells, codeword or not) with the device-exported trees of all its rows
    and columns; sample(r, c, axis) = (r, c, axis, share, proof nodes)."""

    def __init__(self, ctx, cells):
        from celestia_eds import proof
        from celestia_eds.rsmt2d import ExtendedDataSquare
        self.cells = cells
        self.w = cells.shape[0]
        self.k = self.w // 2
        sq = ExtendedDataSquare(cells, ctx=ctx)
        self.trees = [proof.axis_trees(sq, axis, 0, self.w) for axis in (ROW, COL)]
        self.roots = [[t[-1].tobytes() for t in self.trees[axis]] for axis in (ROW, COL)]

    def sample(self, r, c, axis):
        from celestia_eds import proof
        index, leaf = (r, c) if axis == ROW else (c, r)
        return (r, c, axis, self.cells[r, c].tobytes(), proof.nmt_prove_range(self.trees[axis][index], leaf, leaf + 1))

    def mirror(self, s):
        """The mirror's verdict of sample s under cel_dev_place_samples' rules."""
        r, c, axis, share, nodes = s
        if r >= self.w or c >= self.w or axis > 1:
            return False
        ns = share[:29] if r < self.k and c < self.k else PARITY
        index, leaf = (r, c) if axis == ROW else (c, r)
        return nmt_ref.mirror_verify(leaf, leaf + 1, ns, [share], nodes, self.roots[axis][index])


def _sample_set(sq, present, rng):
    """One sample per present cell with alternating axes, then the troublemakers, shuffled;
    also returns the absent cell that only a tampered sample names."""
    w = sq.w
    cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(present))]
    samples = [sq.sample(r, c, i % 2) for i, (r, c) in enumerate(cells)]
    good = list(samples)
    pick = lambda: good[int(rng.integers(0, len(good)))]
    for i in range(20):  # a flipped share or node bit
        r, c, axis, share, nodes = pick()
        if i % 2 == 0 or not nodes:
            share = vc.flip(share, int(rng.integers(0, 512)))
        else:
            j = int(rng.integers(0, len(nodes)))
            nodes = nodes[:j] + [vc.flip(nodes[j], int(rng.integers(0, 90)))] + nodes[j + 1:]
        samples.append((r, c, axis, share, nodes))
    for _ in range(5):  # row and column swapped
        r, c, axis, share, nodes = pick()
        samples.append((c, r, axis, share, nodes))
    for _ in range(5):  # duplicates
        samples.append(pick())
    for r, c in ((w, 0), (1, w + 3), (2 ** 31, 2 ** 31)):  # outside the square
        samples.append((r, c) + pick()[2:])
    r, c, _, share, nodes = pick()
    samples.append((r, c, 2, share, nodes))  # neither a row nor a column proof
    absent = [(int(r), int(c)) for r, c in zip(*np.nonzero(present == 0))]
    ur, uc = absent[len(absent) // 2]
    r, c, axis, share, nodes = sq.sample(ur, uc, ROW)
    samples.append((r, c, axis, vc.flip(share, 77), nodes))
    order = rng.permutation(len(samples))
    return [samples[i] for i in order], (ur, uc)


def _flat(samples):
    buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return dict(rows=np.array([s[0] for s in samples], np.uint32), cols=np.array([s[1] for s in samples], np.uint32),
                axes=np.array([s[2] for s in samples], np.uint8), shares=buf(s[3] for s in samples),
                nodes=buf(x for s in samples for x in s[4]),
                node_off=np.cumsum([0] + [len(s[4]) for s in samples]).astype(np.uint64))


@pytest.mark.parametrize("k", [8, 32])
def test_samples_to_repair(ctx, oracle, k):
    from celestia_eds import _lib
    from celestia_eds.rsmt2d import RepairFromSamples
    from hipmem import DeviceBuffer
    eds, rr, cr, _ = oracle.extend_and_commit(random_ods(k, 7))
    w = 2 * k
    present = (np.random.default_rng(7).random((w, w)) < 0.55).astype(np.uint8)
    damaged = eds.copy()
    damaged[present == 0] = 0
    assert oracle.repair(damaged, present, rr, cr)[0] == 0, "the oracle must repair this mask"
    sq = Square(ctx, eds)
    assert sq.roots[ROW] == [r.tobytes() for r in rr] and sq.roots[COL] == [c.tobytes() for c in cr]
    samples, (ur, uc) = _sample_set(sq, present, np.random.default_rng(k))
    want = [sq.mirror(s) for s in samples]
    assert sum(want) >= int(present.sum()) + 5 and want.count(False) >= 25
    covered = np.zeros((w, w), np.uint8)
    for s, v in zip(samples, want):
        if v:
            covered[s[0], s[1]] = 1
    assert np.array_equal(covered, present) and not covered[ur, uc]

    # cel_dev_place_samples into a zeroed device square; one absent cell is marked present
    # beforehand and must be left as it is
    f = _flat(samples)
    P = vc._p
    d_eds = DeviceBuffer(eds.nbytes, fill=0)
    pr, pc = [(int(r), int(c)) for r, c in zip(*np.nonzero(present))][3]
    d_eds.upload_at((pr * w + pc) * 512, np.full(512, 0xAB, np.uint8))
    mask = np.zeros((w, w), np.uint8)
    mask[pr, pc] = 1
    ok = np.full(len(samples), 9, np.uint8)
    rra, cra = np.ascontiguousarray(rr), np.ascontiguousarray(cr)
    st = ctx.lib.cel_dev_place_samples(ctx.handle, d_eds.ptr, P(mask), k, P(rra), P(cra), len(samples), P(f["rows"]),
                                       P(f["cols"]), P(f["axes"]), P(f["shares"]), P(f["nodes"]), P(f["node_off"]),
                                       P(ok))
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    assert ok.tolist() == [int(v) for v in want]
    assert np.array_equal(mask, present) and not mask[ur, uc]
    got = d_eds.download(eds.shape)
    expect = damaged.copy()
    expect[pr, pc] = 0xAB
    assert np.array_equal(got, expect)

    # the whole path: verify, place, repair
    out, ok2 = RepairFromSamples(k, samples, [r.tobytes() for r in rr], [c.tobytes() for c in cr], ctx=ctx)
    assert ok2 == want
    assert np.array_equal(out.cells, eds)
    assert out.RowRoots() == [r.tobytes() for r in rr] and out.ColRoots() == [c.tobytes() for c in cr]


def test_byzantine_passes_through(ctx, oracle):
    """A square with one corrupt Q0 cell and roots recomputed over it: every sample verifies,
    so the bad cell reaches the crossword, which reports the axis cel_repair reports."""
    from celestia_eds.rsmt2d import ErrByzantineData, ExtendedDataSquare, RepairFromSamples
    k = 8
    eds, _, _, _ = oracle.extend_and_commit(random_ods(k, 7))
    w = 2 * k
    bad = eds.copy()
    bad[0, 1, 200] ^= 0x40
    present = np.ones((w, w), np.uint8)
    for r, c in ((3, 5), (0, 7), (9, 1)):  # row 0 and column 1 incomplete: their decode meets the bad cell
        present[r, c] = 0
    sq = Square(ctx, bad)
    rr, cr = sq.roots
    samples = [sq.sample(int(r), int(c), i % 2) for i, (r, c) in enumerate(zip(*np.nonzero(present)))]
    assert all(sq.mirror(s) for s in samples)
    ref = ExtendedDataSquare(np.where(present[..., None] == 1, bad, 0).astype(np.uint8), ctx=ctx)
    with pytest.raises(ErrByzantineData) as want:
        ref.Repair(rr, cr, present=present)
    with pytest.raises(ErrByzantineData) as got:
        RepairFromSamples(k, samples, rr, cr, ctx=ctx)
    assert (got.value.Axis, got.value.Index) == (want.value.Axis, want.value.Index)
    assert got.value.Shares == want.value.Shares


def test_sample_call_errors(ctx):
    from celestia_eds import _lib
    from hipmem import DeviceBuffer
    k, w = 2, 4
    d_eds = DeviceBuffer(w * w * 512, fill=0)
    mask = np.zeros((w, w), np.uint8)
    roots = np.zeros((w, 90), np.uint8)
    one = np.zeros(512, np.uint8)
    z32, z8, off, ok = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(2, np.uint64), np.full(1, 9, np.uint8)
    P = vc._p

    def place(d=d_eds.ptr, k=k, n=1, shares=P(one)):
        return ctx.lib.cel_dev_place_samples(ctx.handle, d, P(mask), k, P(roots), P(roots), n, P(z32), P(z32), P(z8),
                                             shares, P(one), P(off), P(ok))

    assert place(d=None) == _lib.EINVAL and place(shares=None) == _lib.EINVAL
    assert place(k=3) == _lib.ENOTPOW2 and place(k=1024) == _lib.ETOOBIG
    assert place(n=0) == _lib.OK
    # a proof without nodes against an all-zero root: verdict 0, nothing written
    assert place() == _lib.OK and ok[0] == 0 and not mask.any()
    assert not d_eds.download((w, w, 512)).any()
    out = np.zeros((w, w, 512), np.uint8)
    args = (P(roots), P(roots), 1, P(z32), P(z32), P(z8), P(one), P(one), P(off), P(ok))
    assert ctx.lib.cel_repair_samples(ctx.handle, k, *args, None, P(mask), None, None, None, None) == _lib.EINVAL
    assert ctx.lib.cel_repair_samples(ctx.handle, 3, *args, P(out), P(mask), None, None, None, None) == _lib.ENOTPOW2
    # no sample accepted: nothing to repair from
    assert ctx.lib.cel_repair_samples(ctx.handle, k, *args, P(out), P(mask), None, None, None,
                                      None) == _lib.EUNREPAIRABLE
