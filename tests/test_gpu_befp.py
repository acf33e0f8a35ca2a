"""GPU: bad-encoding fraud proofs. The verifier (cel_befp_verify_batch through
fraud.ValidateBatch) against tests/befp_ref.py over honest and malicious squares, tampered
entries, short and malformed proofs, in one batch, reversed and one by one; the producer
(cel_befp_build through fraud.CreateBadEncodingProof) after a byzantine repair.

Shapes: k = 1 (two-cell axes, one entry suffices), 2, 4 (the bit-sliced encoder), 16, 32 (the
register decoder's lower bound, 64 points), 128, 256 (GF(2^16)). The entries' proofs come from
ExtendedDataSquare.SampleProofs (the batched prover, tested on its own); the reference checks
every one of them again with the recursive mirror. Rebuilt roots are compared byte for byte
where the entries agree with one codeword or are exactly k; where more than k entries agree with
no codeword, what a decoder returns is not defined, and only the verdict is compared."""
import ctypes
import functools

import numpy as np
import pytest

import befp_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [1, 2, 4, 16, 32, 128, 256]


def _flip(b, i):
    return b[:i] + bytes([b[i] ^ 0x21]) + b[i + 1:]


@functools.lru_cache(maxsize=None)
def _batch(k):
    """Every case at width k, built once: (names, proofs, roots per proof, expected verdict or
    None, compare-root flags, reference (verdict, root))."""
    import celestia_eds
    from celestia_eds import fraud
    from celestia_eds.rsmt2d import ExtendedDataSquare
    ctx = celestia_eds.default_context(0)
    w = 2 * k
    squares = {"honest": R.honest_square(k), "data": R.malicious_square(k, (0, 0)),
               "parity": R.malicious_square(k, (w - 1, w - 1))}
    data, parity, everything = list(range(k)), list(range(k, w)), list(range(w))
    straddle = list(range(k // 2, k // 2 + k))
    specs = []  # (name, square, axis, index, positions, entry axis of position p, expected, compare root)

    def add(name, sq, axis, index, positions, ea, want, cmp_root=True):
        specs.append((name, sq, axis, index, list(positions), ea, want, cmp_root))

    orth = lambda axis: (lambda p: 1 - axis)
    same = lambda axis: (lambda p: axis)
    mixed = lambda p: p & 1
    add("honest row, data half, orthogonal", "honest", 0, 0, data, orth(0), R.NOT_FRAUD)
    add("honest row, parity half, same axis", "honest", 0, w - 1, parity, same(0), R.NOT_FRAUD)
    add("honest column, straddling, orthogonal", "honest", 1, w - 1, straddle, orth(1), R.NOT_FRAUD)
    add("honest column, parity half, same axis", "honest", 1, k, parity, same(1), R.NOT_FRAUD)
    add("honest column, all 2k, mixed", "honest", 1, 0, everything, mixed, R.NOT_FRAUD)
    add("honest row, all 2k, same axis", "honest", 0, k, everything, same(0), R.NOT_FRAUD)
    for sq, cell in (("data", (0, 0)), ("parity", (w - 1, w - 1))):
        for axis in (0, 1):
            index, at = (cell[1], cell[0]) if axis else cell
            near, far = (data, parity) if at < k else (parity, data)
            tag = f"{sq} flip, {'column' if axis else 'row'} through it"
            add(f"{tag}, k entries with the cell", sq, axis, index, near, orth(axis), R.FRAUD)
            add(f"{tag}, k entries without it", sq, axis, index, far, same(axis), R.FRAUD)
            add(f"{tag}, all but the cell", sq, axis, index, [p for p in everything if p != at], mixed, R.FRAUD)
            add(f"{tag}, all 2k", sq, axis, index, everything, orth(axis), R.FRAUD, cmp_root=False)
            add(f"{tag}, k + 1 with the cell", sq, axis, index, near + far[:1], mixed, R.FRAUD, cmp_root=False)
        other = (cell[0] + k) % w
        add(f"{sq} flip, a row off it", sq, 0, other, data, orth(0), R.NOT_FRAUD)
        add(f"{sq} flip, a row off it, all 2k", sq, 0, other, everything, mixed, R.NOT_FRAUD)
    add("k - 1 entries", "data", 0, 0, data[:k - 1], orth(0), R.TOO_FEW)
    add("empty", "honest", 1, 0, [], orth(1), R.TOO_FEW)
    # one SampleProofs call per square for every entry used
    table = {}
    for name, (eds, rr, cr) in squares.items():
        coords = sorted({((p, index, ea(p)) if axis else (index, p, ea(p)))
                         for _, sq, axis, index, positions, ea, _, _ in specs if sq == name for p in positions})
        got = ExtendedDataSquare(eds, ctx=ctx).SampleProofs(coords)
        table[name] = {(r, c, a): (sh, nd) for r, c, a, sh, nd in got}

    def entries(sq, axis, index, positions, ea):
        out = []
        for p in positions:
            sh, nd = table[sq][(p, index, ea(p)) if axis else (index, p, ea(p))]
            out.append((p, sh, list(nd), ea(p)))
        return out

    cases = []  # (name, square, axis, index, entries, expected, compare root)
    for name, sq, axis, index, positions, ea, want, cmp_root in specs:
        cases.append((name, sq, axis, index, entries(sq, axis, index, positions, ea), want, cmp_root))
    # one tampered entry in k good ones (the data-flip square's row 0, orthogonal proofs)
    good = entries("data", 0, 0, data, orth(0))
    t = k // 2
    p, sh, nd, ea = good[t]
    tampered = [("share byte", (p, _flip(sh, 300), nd, ea)), ("node byte", (p, sh, [_flip(nd[0], 40)] + nd[1:], ea)),
                ("position", (p + k, sh, nd, ea)), ("node dropped", (p, sh, nd[:-1], ea)),
                ("node added", (p, sh, nd + nd[:1], ea))]
    if k > 1:  # at k = 1 the three parity cells are one share: a proof holds in either direction
        tampered.append(("proving direction", (p, sh, nd, 1 - ea)))
    for name, bad in tampered:
        cases.append((f"tampered {name}", "data", 0, 0, good[:t] + [bad] + good[t + 1:], R.BAD_SHARE, True))
    # every malformed cause, each in an otherwise good proof
    cases.append(("malformed: axis", "data", 2, 0, good, R.MALFORMED, True))
    cases.append(("malformed: index", "data", 0, w, good, R.MALFORMED, True))
    cases.append(("malformed: position", "data", 0, 0, good[:t] + [(w, sh, nd, ea)] + good[t + 1:], R.MALFORMED, True))
    cases.append(("malformed: entry axis", "data", 0, 0, good[:t] + [(p, sh, nd, 2)] + good[t + 1:], R.MALFORMED, True))
    cases.append(("malformed: repeated position", "data", 0, 0, good + [good[t]], R.MALFORMED, True))
    cases.append(("malformed before too few", "data", 3, 0, [], R.MALFORMED, True))
    proofs = [fraud.BadEncodingProof(1, axis, index, [fraud.ShareWithProof(*e) for e in ents])
              for _, _, axis, index, ents, _, _ in cases]
    rrs = [squares[sq][1] for _, sq, *_ in cases]
    crs = [squares[sq][2] for _, sq, *_ in cases]
    ref = [R.verdict(k, axis, index, ents, squares[sq][1], squares[sq][2]) for _, sq, axis, index, ents, _, _ in cases]
    verdicts, roots = fraud.ValidateBatch(proofs, rrs, crs, k, ctx=ctx, rebuilt=True)
    return dict(names=[c[0] for c in cases], want=[c[5] for c in cases], cmp_root=[c[6] for c in cases], proofs=proofs,
                rrs=rrs, crs=crs, ref=ref, verdicts=verdicts, roots=roots, ctx=ctx)


@pytest.mark.parametrize("k", SHAPES)
def test_batch_matches_reference(ctx, oracle, k):
    b = _batch(k)
    for name, want, (rv, rroot), got, root, cmp_root in zip(b["names"], b["want"], b["ref"], b["verdicts"], b["roots"],
                                                             b["cmp_root"]):
        assert rv == want, f"k = {k}, {name}: the reference says {rv}, the rule promises {want}"
        assert got == rv, f"k = {k}, {name}: verdict {got}, reference {rv}"
        if cmp_root:
            assert root == rroot, f"k = {k}, {name}: rebuilt root differs from the reference's"
        else:
            assert root is not None and len(root) == 90


@pytest.mark.parametrize("k", SHAPES)
def test_verdicts_do_not_depend_on_the_batch(ctx, oracle, k):
    from celestia_eds import fraud
    b = _batch(k)
    rev = fraud.ValidateBatch(b["proofs"][::-1], b["rrs"][::-1], b["crs"][::-1], k, ctx=ctx, rebuilt=True)
    assert rev[0][::-1] == b["verdicts"]
    for name, root, other, cmp_root in zip(b["names"], b["roots"], rev[1][::-1], b["cmp_root"]):
        if cmp_root:
            assert root == other, name
    # alone: every case at the small widths, one of each kind at the large ones
    step = 1 if k <= 32 else 5
    for i in list(range(0, len(b["proofs"]), step)):
        alone = fraud.ValidateBatch([b["proofs"][i]], [b["rrs"][i]], [b["crs"][i]], k, ctx=ctx, rebuilt=True)
        assert alone[0] == [b["verdicts"][i]], b["names"][i]
        if b["cmp_root"][i]:
            assert alone[1] == [b["roots"][i]], b["names"][i]
        assert b["proofs"][i].Validate(b["rrs"][i], b["crs"][i], ctx=ctx) == b["verdicts"][i]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_call_errors(ctx, oracle):
    """The call's own errors, and the nullable output."""
    from celestia_eds import _lib
    k = 2
    b = _batch(k)
    lib, h = ctx.lib, ctx.handle
    i = b["names"].index("honest row, data half, orthogonal")
    pr = b["proofs"][i]
    node = _lib.NMT_NODE_SIZE
    axes, index = np.array([pr.Axis], np.uint8), np.array([pr.Index], np.uint32)
    ent_off = np.array([0, len(pr.Shares)], np.uint64)
    pos = np.array([s.Position for s in pr.Shares], np.uint32)
    ea = np.array([s.Axis for s in pr.Shares], np.uint8)
    shares = np.frombuffer(b"".join(s.Share for s in pr.Shares), np.uint8).copy()
    nodes = np.frombuffer(b"".join(x for s in pr.Shares for x in s.Nodes), np.uint8).copy()
    node_off = np.cumsum([0] + [len(s.Nodes) for s in pr.Shares]).astype(np.uint64)
    rr = np.frombuffer(b"".join(b["rrs"][i]), np.uint8).copy()
    cr = np.frombuffer(b"".join(b["crs"][i]), np.uint8).copy()
    out = np.full(1, 0xEE, np.uint8)
    args = lambda **kw: [kw.get(n, v) for n, v in (("axes", _p(axes)), ("index", _p(index)), ("ent_off", _p(ent_off)),
                                                   ("pos", _p(pos)), ("ea", _p(ea)), ("shares", _p(shares)),
                                                   ("nodes", _p(nodes)), ("node_off", _p(node_off)), ("rr", _p(rr)),
                                                   ("cr", _p(cr)), ("out", _p(out)), ("reb", None))]
    assert lib.cel_befp_verify_batch(h, 1, k, *args()) == _lib.OK and out[0] == _lib.BEFP_NOT_FRAUD
    reb = np.zeros(node, np.uint8)
    assert lib.cel_befp_verify_batch(h, 1, k, *args(reb=_p(reb))) == _lib.OK
    assert reb.tobytes() == b["rrs"][i][pr.Index]
    assert lib.cel_befp_verify_batch(h, 0, k, *([None] * 12)) == _lib.OK
    for name in ("axes", "index", "ent_off", "pos", "ea", "shares", "nodes", "node_off", "rr", "cr", "out"):
        assert lib.cel_befp_verify_batch(h, 1, k, *args(**{name: None})) == _lib.EINVAL, name
    for bad_k in (0, 3, 1024):
        assert lib.cel_befp_verify_batch(h, 1, bad_k, *args()) == _lib.EINVAL
    dec = np.array([2, 0], np.uint64)
    assert lib.cel_befp_verify_batch(h, 1, k, *args(ent_off=_p(dec))) == _lib.EINVAL
    decn = node_off.copy()
    decn[1] = 0
    decn[0] = 1
    assert lib.cel_befp_verify_batch(h, 1, k, *args(node_off=_p(decn))) == _lib.EINVAL
    # the same proof once more after the refusals
    assert lib.cel_befp_verify_batch(h, 1, k, *args()) == _lib.OK and out[0] == _lib.BEFP_NOT_FRAUD


# ------------------------------------------------------------------ round trip


def _mask(k):
    """The shape of test_corrupt_cell_byzantine: row 0 and column 1 are incomplete, so their
    decode meets cell (0, 1)."""
    w = 2 * k
    present = np.ones((w, w), np.uint8)
    present[3 % w, 5 % w] = 0
    present[0, 7 % w] = 0
    present[9 % w, 1] = 0
    return present


def _repair_raises(ctx, eds, present, rr, cr):
    from celestia_eds.rsmt2d import ErrByzantineData, ExtendedDataSquare
    sq = ExtendedDataSquare(np.where(present[..., None] == 1, eds, 0).astype(np.uint8), ctx=ctx)
    with pytest.raises(ErrByzantineData) as ei:
        sq.Repair(rr, cr, present=present)
    return sq, ei.value


def _as_entries(proof):
    return [(s.Position, s.Share, s.Nodes, s.Axis) for s in proof.Shares]


@pytest.mark.parametrize("k", [2, 16, 32])
def test_round_trip_malicious_square(ctx, oracle, k):
    """Roots made over the flipped square: repair -> proof -> FRAUD."""
    from celestia_eds import _lib, fraud
    eds, rr, cr = R.malicious_square(k, (0, 1), byte=200)
    sq, err = _repair_raises(ctx, eds, _mask(k), rr, cr)
    assert (err.Axis, err.Index) in ((0, 0), (1, 1))
    proof = fraud.CreateBadEncodingProof(5, err, sq, rr, cr)
    assert (proof.Height, proof.Axis, proof.Index) == (5, err.Axis, err.Index)
    assert len(proof.Shares) >= k
    assert [s.Position for s in proof.Shares] == sorted({s.Position for s in proof.Shares})
    assert all(s.Axis == 1 - err.Axis for s in proof.Shares)
    assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_FRAUD
    assert R.verdict(k, proof.Axis, proof.Index, _as_entries(proof), rr, cr)[0] == R.FRAUD
    # each entry's nodes: cel_nmt_prove_range on cel_axis_tree of its orthogonal axis
    w, node = 2 * k, _lib.NMT_NODE_SIZE
    for s in proof.Shares:
        cells = np.ascontiguousarray(sq.cells[s.Position] if err.Axis else sq.cells[:, s.Position])
        tree = np.zeros((2 * w - 1, node), np.uint8)
        ctx.check(ctx.lib.cel_axis_tree(ctx.handle, _p(cells), k, s.Position, _lib.SHARE_SIZE, _p(tree)))
        out, nn = np.zeros((w.bit_length(), node), np.uint8), ctypes.c_uint32()
        assert ctx.lib.cel_nmt_prove_range(_p(tree), w, err.Index, err.Index + 1, _p(out), ctypes.byref(nn)) == _lib.OK
        assert [out[j].tobytes() for j in range(nn.value)] == s.Nodes, s.Position
        cell = (s.Position, err.Index) if err.Axis else (err.Index, s.Position)
        assert s.Share == eds[cell].tobytes()


@pytest.mark.parametrize("k", [4, 32])
def test_resident_square_repair_to_proof(ctx, oracle, k):
    """cel_dev_repair leaves the square in device memory; cel_dev_befp_build reads it there and
    gives what cel_befp_build gives over the downloaded square."""
    from celestia_eds import _lib, fraud
    from hipmem import DeviceBuffer
    w, share, node, per = 2 * k, _lib.SHARE_SIZE, _lib.NMT_NODE_SIZE, (2 * k).bit_length() - 1
    eds, rr, cr = R.malicious_square(k, (0, 1), byte=200)
    present = _mask(k)
    d_eds = DeviceBuffer(eds.nbytes)
    d_eds.upload(np.where(present[..., None] == 1, eds, 0).astype(np.uint8))
    rra, cra = np.frombuffer(b"".join(rr), np.uint8).copy(), np.frombuffer(b"".join(cr), np.uint8).copy()
    ba, bi = ctypes.c_int32(-1), ctypes.c_int32(-1)
    st = ctx.lib.cel_dev_repair(ctx.handle, d_eds.ptr, _p(present), k, _p(rra), _p(cra), ctypes.byref(ba),
                                ctypes.byref(bi), None, None)
    assert st == _lib.EBYZANTINE and (ba.value, bi.value) in ((0, 0), (1, 1))

    def build(fn, square):
        pos, ea = np.full(w, 0xEEEEEEEE, np.uint32), np.full(w, 0xEE, np.uint8)
        sh, nd, cnt = np.zeros((w, share), np.uint8), np.zeros((w, per, node), np.uint8), ctypes.c_uint32(99)
        ctx.check(fn(ctx.handle, square, _p(present), k, _p(rra), _p(cra), ba.value, bi.value, _p(pos), _p(ea), _p(sh),
                     _p(nd), ctypes.byref(cnt)))
        m = cnt.value
        return pos[:m].tolist(), ea[:m].tolist(), sh[:m].copy(), nd[:m].copy()

    dev = build(ctx.lib.cel_dev_befp_build, d_eds.ptr)
    cells = d_eds.download((w, w, share))
    host = build(ctx.lib.cel_befp_build, _p(cells))
    assert dev[0] == host[0] and dev[1] == host[1] and len(dev[0]) >= k
    assert np.array_equal(dev[2], host[2]) and np.array_equal(dev[3], host[3])
    proof = fraud.BadEncodingProof(9, ba.value, bi.value,
                                   [fraud.ShareWithProof(p, dev[2][e].tobytes(), [x.tobytes() for x in dev[3][e]], a)
                                    for e, (p, a) in enumerate(zip(dev[0], dev[1]))])
    assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_FRAUD
    # the producer's own errors
    z = ctypes.c_uint32()
    args = [_p(present), k, _p(rra), _p(cra)]
    pos_out, ea_out = np.zeros(w, np.uint32), np.zeros(w, np.uint8)
    outs = [_p(pos_out), _p(ea_out), _p(dev[2]), _p(dev[3]), ctypes.byref(z)]
    assert ctx.lib.cel_dev_befp_build(ctx.handle, d_eds.ptr, *args, 2, 0, *outs) == _lib.EINVAL
    assert ctx.lib.cel_dev_befp_build(ctx.handle, d_eds.ptr, *args, 0, w, *outs) == _lib.EINVAL
    assert ctx.lib.cel_dev_befp_build(ctx.handle, None, *args, 0, 0, *outs) == _lib.EINVAL
    assert ctx.lib.cel_befp_build(ctx.handle, _p(cells), _p(present), 3, _p(rra), _p(cra), 0, 0, *outs) == _lib.EINVAL
    d_eds.free()


@pytest.mark.parametrize("k", [1, 2, 16, 32, 128])
def test_same_accusation_on_the_honest_square(ctx, oracle, k):
    from celestia_eds import _lib, fraud
    from celestia_eds.rsmt2d import ErrByzantineData, ExtendedDataSquare
    eds, rr, cr = R.honest_square(k)
    sq = ExtendedDataSquare(eds, ctx=ctx)
    sq._mask = np.ones((2 * k, 2 * k), np.uint8)
    for axis, index in ((0, 0), (1, 1)):
        proof = fraud.CreateBadEncodingProof(5, ErrByzantineData(axis, index, "claimed"), sq, rr, cr)
        assert len(proof.Shares) == 2 * k
        assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_NOT_FRAUD
    # under the repair's mask fewer positions qualify, and the verdict stays
    sq._mask = _mask(k)
    proof = fraud.CreateBadEncodingProof(5, ErrByzantineData(0, 0, "claimed"), sq, rr, cr)
    want = [j for j in range(2 * k) if sq._mask[0, j] and sq._mask[:, j].all()]
    assert [s.Position for s in proof.Shares] == want and len(want) >= k
    assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_NOT_FRAUD


@pytest.mark.parametrize("k", [2, 16, 32])
def test_flip_after_the_roots(ctx, oracle, k):
    """The existing repair test's case: honest roots, one cell corrupted afterwards. The
    producer gives no entry for the corrupt cell, and every entry it gives verifies; the rule
    then cannot prove fraud: the accused root is honest."""
    from celestia_eds import _lib, fraud
    from celestia_eds.rsmt2d import ErrByzantineData, ExtendedDataSquare
    eds, rr, cr = R.honest_square(k)
    bad = eds.copy()
    bad[0, 1, 200] ^= 0x40
    sq, err = _repair_raises(ctx, bad, _mask(k), rr, cr)
    proof = fraud.CreateBadEncodingProof(5, err, sq, rr, cr)
    corrupt = 1 if err.Axis == 0 else 0
    assert (err.Axis, err.Index) in ((0, 0), (1, 1))
    assert corrupt not in [s.Position for s in proof.Shares]
    assert all(R.entry_ok(k, err.Axis, err.Index, e, rr, cr) for e in _as_entries(proof))
    # a complete orthogonal axis that holds the corrupt cell: only its root can rule it out
    full = ExtendedDataSquare(bad, ctx=ctx)
    full._mask = np.ones((2 * k, 2 * k), np.uint8)
    proof = fraud.CreateBadEncodingProof(5, ErrByzantineData(0, 0, "claimed"), full, rr, cr)
    assert [s.Position for s in proof.Shares] == [j for j in range(2 * k) if j != 1]
    assert all(R.entry_ok(k, 0, 0, e, rr, cr) for e in _as_entries(proof))
    assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_NOT_FRAUD
    # a sample of the corrupt cell fills the position, and its proof fails
    sample = full.SampleProofs([(0, 1, 1)])
    proof = fraud.CreateBadEncodingProof(5, ErrByzantineData(0, 0, "claimed"), full, rr, cr, samples=sample)
    assert [s.Position for s in proof.Shares] == list(range(2 * k))
    assert proof.Validate(rr, cr, ctx=ctx) == _lib.BEFP_BAD_SHARE
