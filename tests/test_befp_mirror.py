"""CPU: the fraud-proof rule without a device, on a k = 2 square. tests/befp_ref.py (the
reference verdict the GPU tests compare with) gives the outcomes the rule promises, and
celestia_eds.fraud's structural checks agree with it; proofs that cannot be marshalled get their
verdict in Python."""
import itertools

import pytest

import befp_ref as R

K, W = 2, 4


@pytest.fixture(scope="module")
def squares(oracle):
    return {"honest": R.honest_square(K), "data": R.malicious_square(K, (0, 1)), "parity": R.malicious_square(K, (3, 2))}


def _entries(eds, axis, index, positions, entry_axis):
    return [R.host_entry(eds, K, axis, index, p, entry_axis) for p in positions]


def test_honest_axes_are_not_fraud(squares):
    eds, rr, cr = squares["honest"]
    for axis, index, ea in itertools.product((0, 1), (0, 3), (0, 1)):
        accused = (cr if axis else rr)[index]
        for pos in list(itertools.combinations(range(W), K)) + [tuple(range(W))]:
            v, root = R.verdict(K, axis, index, _entries(eds, axis, index, pos, ea), rr, cr)
            assert (v, root) == (R.NOT_FRAUD, accused), (axis, index, ea, pos)


@pytest.mark.parametrize("name,cell", [("data", (0, 1)), ("parity", (3, 2))])
def test_malicious_axes_are_fraud(squares, name, cell):
    eds, rr, cr = squares[name]
    for axis, ea in itertools.product((0, 1), (0, 1)):
        index, at = (cell[1], cell[0]) if axis else cell
        for pos in list(itertools.combinations(range(W), K)) + [(0, 1, 2), tuple(range(W))]:
            v, root = R.verdict(K, axis, index, _entries(eds, axis, index, pos, ea), rr, cr)
            assert v == R.FRAUD and root != (cr if axis else rr)[index], (axis, ea, pos, at in pos)
    other = (cell[0] + 1) % W
    v, _ = R.verdict(K, 0, other, _entries(eds, 0, other, (1, 3), 1), rr, cr)
    assert v == R.NOT_FRAUD


def test_bad_share_too_few_malformed(squares):
    eds, rr, cr = squares["data"]
    good = _entries(eds, 0, 0, (0, 1, 3), 1)
    assert R.verdict(K, 0, 0, good, rr, cr)[0] == R.FRAUD
    p, sh, nd, ea = good[1]
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    for bad in ((p, flip(sh, 300), nd, ea), (p, sh, [flip(nd[0], 50)] + nd[1:], ea), (2, sh, nd, ea),
                (p, sh, nd[:-1], ea), (p, sh, nd, 0)):
        assert R.verdict(K, 0, 0, [good[0], bad, good[2]], rr, cr) == (R.BAD_SHARE, None)
    assert R.verdict(K, 0, 0, good[:1], rr, cr) == (R.TOO_FEW, None)
    assert R.verdict(K, 0, 0, [], rr, cr) == (R.TOO_FEW, None)
    for axis, index, ents in ((2, 0, good), (0, W, good), (0, 0, [good[0], (W, sh, nd, ea)]),
                              (0, 0, [good[0], (p, sh, nd, 2)]), (0, 0, [good[0], good[0]]), (2, 0, [])):
        assert R.verdict(K, axis, index, ents, rr, cr) == (R.MALFORMED, None)


def test_fraud_module_structure(squares):
    from celestia_eds import _lib, fraud
    assert [_lib.BEFP_NOT_FRAUD, _lib.BEFP_FRAUD, _lib.BEFP_BAD_SHARE, _lib.BEFP_TOO_FEW, _lib.BEFP_MALFORMED] == \
        [R.NOT_FRAUD, R.FRAUD, R.BAD_SHARE, R.TOO_FEW, R.MALFORMED]
    eds, rr, cr = squares["data"]
    good = _entries(eds, 0, 0, (0, 1, 3), 1)
    swp = lambda es: [fraud.ShareWithProof(*e) for e in es]
    p, sh, nd, ea = good[1]
    cases = [(0, 0, good), (0, 0, good[:1]), (0, 0, []), (2, 0, good), (0, W, good), (1, W - 1, good),
             (0, 0, [good[0], (W, sh, nd, ea)]), (0, 0, [good[0], (p, sh, nd, 2)]), (0, 0, [good[0], good[0]]),
             (-1, 0, good), (0, -1, good), (0, 0, [good[0], (-1, sh, nd, ea)])]
    for axis, index, ents in cases:
        proof = fraud.BadEncodingProof(7, axis, index, swp(ents))
        want = R.MALFORMED if min([axis, index] + [e[0] for e in ents]) < 0 else R.structural(K, axis, index, ents)
        assert fraud.structural_verdict(proof, K) == want, (axis, index)
    # what cannot be marshalled never reaches the library: no device is needed for these
    short = fraud.BadEncodingProof(7, 0, 0, swp([good[0], (p, sh[:-1], nd, ea), good[2]]))
    node = fraud.BadEncodingProof(7, 0, 0, swp([good[0], (p, sh, [nd[0][:-1]] + nd[1:], ea), good[2]]))
    neg = fraud.BadEncodingProof(7, 0, 0, swp([good[0], (-1, sh, nd, ea)]))
    few = fraud.BadEncodingProof(7, 0, 0, swp([(p, sh[:-1], nd, ea)]))
    got = fraud.ValidateBatch([short, node, neg, few], [rr] * 4, [cr] * 4, K)
    assert got == [R.BAD_SHARE, R.BAD_SHARE, R.MALFORMED, R.TOO_FEW]
    assert fraud.ValidateBatch([short], [rr], [cr], K, rebuilt=True) == ([R.BAD_SHARE], [None])
    assert short.Validate(rr, cr) == R.BAD_SHARE
    assert fraud.ValidateBatch([], [], [], K) == []
