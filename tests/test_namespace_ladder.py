"""CPU: the inputs of tests/test_gpu_namespace_bytes.py cover what they are for.
namespace_inputs.byte_ladder must decide a transition at every one of the 29 bytes, with a later
byte that points the other way, on row ends, across 0x80, and hold the near-parity namespaces;
the queries built from it, run through the host mirror over hashlib trees, must give inclusion
and absence entries decided at every byte. No device: if the ladder stops covering a byte, this
fails before any GPU test can pass for the wrong reason."""
import numpy as np
import pytest

import namespace_inputs as ni

NS = ni.NS
SEEDS = {8: 8, 32: 32}
_ladders = {}


def _ladder(k):
    if k not in _ladders:
        _ladders[k] = ni.byte_ladder(k, SEEDS[k])
    return _ladders[k]


def _contrary(b, x, y):
    return b + 1 < NS and x[b + 1] > y[b + 1]


@pytest.mark.parametrize("k", [8, 32])
def test_ladder_is_sorted_in_short_runs(k):
    nss, trans = _ladder(k)
    assert len(nss) == k * k and nss == sorted(nss) and ni.PARITY not in nss
    runs = {}
    for x in nss:
        runs[x] = runs.get(x, 0) + 1
    assert set(runs.values()) == {1, 2, 3}
    assert len(trans) == len(runs) - 1
    for pos, b, x, y in trans:
        assert nss[pos - 1] == x and nss[pos] == y and x < y
        assert x[:b] == y[:b] and x[b] < y[b]  # b is the deciding byte
    assert ni.byte_ladder(k, SEEDS[k]) == (nss, trans)  # seeded


@pytest.mark.parametrize("k", [8, 32])
def test_every_byte_decides_with_a_contrary_next_byte(k):
    nss, trans = _ladder(k)
    assert {b for _, b, _, _ in trans} == set(range(NS))
    # inside a dword this fails a compare with the bytes in the wrong order; at b % 4 == 3 one
    # with the words in the wrong order
    assert {b for _, b, x, y in trans if _contrary(b, x, y)} == set(range(NS - 1))


def test_k32_row_ends_and_sign_crossings():
    k = 32
    nss, trans = _ladder(k)
    # the last namespace of a row and the first of the next: a root's max and the next root's min
    at_end = [(b, x, y) for pos, b, x, y in trans if pos % k == 0]
    assert len(at_end) == k - 1
    assert {b for b, x, y in at_end if _contrary(b, x, y) or b == NS - 1} == set(range(NS))
    # x[b] < 0x80 <= y[b] in the top byte of a compare word fails a signed compare
    crossed = {b for _, b, x, y in trans if x[b] < 0x80 <= y[b]}
    assert crossed >= {b for b in range(NS) if b % 4 == 0} | {NS - 1}


def test_k32_near_parity_rows():
    k = 32
    nss, trans = _ladder(k)
    tail = nss[(k - 2) * k:]
    want = [ni.near_parity(b) for b in range(NS)]
    assert sorted(set(tail)) == want == sorted(want) and tail == sorted(tail)
    assert all(x not in want for x in nss[:(k - 2) * k])
    assert tail[k - 1] != tail[k]  # the runs fill the two rows exactly
    assert want[NS - 1] == b"\xff" * 28 + b"\xfe"  # the tail-padding namespace
    for b, n in enumerate(want):
        # one word apart from the parity namespace: word b // 4 of the 8 compare words
        words = [i for i in range(8) if (n + bytes(3))[4 * i:4 * i + 4] != (ni.PARITY + bytes(3))[4 * i:4 * i + 4]]
        assert words == [b // 4]
    assert nss[(k - 2) * k - 1] < ni.ABOVE_LADDER < want[0]


@pytest.mark.parametrize("k", [8, 32])
def test_absentees_lie_between_their_neighbours(k):
    nss, trans = _ladder(k)
    present = set(nss)
    for pos, b, x, y in trans:
        qs = ni.absentees(x, y, b)
        if b < NS - 1 and x not in [ni.near_parity(i) for i in range(NS)] and any(y[b + 1:]):
            assert len(qs) == 2
            hi, lo = qs  # late bytes alone against one neighbour, byte b against the other
            assert hi[:b + 1] == x[:b + 1] and hi[b] < y[b] and all(c == 0xFF for c in hi[b + 1:])
            assert lo[:b + 1] == y[:b + 1] and x[b] < lo[b] and all(c == 0 for c in lo[b + 1:])
        for q in qs:
            assert x < q < y and q not in present and q != ni.PARITY
    assert all(any(ni.absentees(x, y, b)) for _, b, x, y in trans if b == NS - 1)


def test_k8_mirror_entries_decided_at_every_byte():
    """The part B queries over hashlib trees alone: for every byte an inclusion entry and an
    absence entry whose namespace is decided against a neighbour at that byte, and a query that
    no row answers because it falls between two rows' ranges."""
    k = 8
    cells, nss, trans = ni.ladder_square(k, SEEDS[k])
    assert (nss, trans) == _ladder(k)
    queries, notes = ni.ladder_queries(nss, trans)
    want = ni.mirror_flat(ni.square_row_tables(cells), cells, queries)
    assert (want["rows"] < k).all()
    by_kind = {0: set(), 1: set()}
    answered = set()
    for i, kind in zip(want["ns_idx"].tolist(), want["kinds"].tolist()):
        what, decided, pos = notes[i]
        assert (what, kind) in (("present", 0), ("absent", 1))
        by_kind[kind] |= decided
        answered.add(i)
    assert by_kind[0] == set(range(NS)) and by_kind[1] == set(range(NS))
    silent = [i for i in range(len(queries)) if i not in answered]
    assert [notes[i][0] for i in silent[-2:]] == ["outside", "outside"]
    between = [i for i in silent[:-2]]
    assert between and all(notes[i][0] == "absent" and notes[i][2] % k == 0 for i in between)
    # the plan's totals follow from the entries
    assert want["leaf_off"][-1] == sum(1 for x in nss) and len(want["nodes"]) == want["node_off"][-1]
    # the mirror's entries are the counting rule's
    rows = [nss[r * k:(r + 1) * k] for r in range(k)]
    flat = [(i, r) + ni.pair_rule(rows[r], q, 2 * k) for i, q in enumerate(queries) for r in range(k)
            if ni.pair_rule(rows[r], q, 2 * k)]
    got = list(zip(want["ns_idx"].tolist(), want["rows"].tolist(), want["starts"].tolist(), want["ends"].tolist(),
                   want["kinds"].tolist()))
    assert got == flat
