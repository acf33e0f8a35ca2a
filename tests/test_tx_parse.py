"""CPU: celestia_eds.square's compact share parser (parse_compact_shares, ParseTxs, compact_walk),
the host statement of go-square v1.1.0 parseCompactShares and the checker of the device path
(tests/test_gpu_txs.py), and square.Deconstruct, the inverse of square.Construct. The parser is
pinned from three sides: it inverts the oracle's compact share writer on unit lists chosen by
byte, every rule of the definition has a hand-made share whose result is written out in
tx_cases.py, and mainnet block 408's original data square deconstructs into exactly its txs."""
import hashlib

import numpy as np
import pytest

import square_inputs as SI
import tx_cases as T
from celestia_eds import _lib, square


@pytest.mark.parametrize("name", list(T.HONEST))
@pytest.mark.parametrize("ns", [T.TX_NS, T.PFB_NS], ids=["tx", "pfb"])
def test_inverse_of_the_compact_share_writer(name, ns):
    units = T.HONEST[name]
    shares = T.honest(ns, units)
    assert square.parse_compact_shares(shares) == units
    status, flags, got = square.compact_walk(T.as_array(shares))
    assert (status, flags) == (0, 0), "an honest builder's reserved bytes agree with the parse"
    # the shares a unit and its prefix touch, from the lengths alone
    at = 0
    share_of = lambda b: 0 if b < 474 else 1 + (b - 474) // 478
    for (data, first, off, n), u in zip(got, units):
        end = at + len(T.uvarint(len(u))) + len(u)
        assert (first, n) == (share_of(at), share_of(end - 1) - share_of(at) + 1)
        assert off == (38 + at if first == 0 else 34 + (at - 474) % 478)
        at = end


def test_honest_cases_are_what_their_names_say():
    sh = T.honest(T.TX_NS, T.HONEST["2-byte varint split across two shares"])
    assert sh[0][511] & 0x80 and not sh[1][34] & 0x80
    sh = T.honest(T.TX_NS, T.HONEST["239 one-byte units in one share"])
    assert len(sh) == 2 and sh[1][510:] == b"\x01\xee"
    sh = T.honest(T.TX_NS, T.HONEST["ends on a share's last byte"])
    assert sh[0][511] == T.FULL[-1] and int.from_bytes(sh[1][30:34], "big") == 34
    assert len(T.honest(T.TX_NS, T.HONEST["a unit over more than 3 shares"])) == 4


@pytest.mark.parametrize("case", T.HAND, ids=[c[0] for c in T.HAND])
def test_rule_by_hand(case):
    _, shares, status, units = case
    if status:
        with pytest.raises(square.TxParseError) as e:
            square.parse_compact_shares(shares)
        assert e.value.kind == status and e.value.status == _lib.EINVAL
        assert square.compact_walk(shares)[0::2] == (status, [])
    else:
        assert square.parse_compact_shares(shares) == units
        assert square.parse_compact_shares(T.as_array(shares)) == units


def test_parse_txs_reads_the_tx_namespace_alone():
    shares = T.honest(T.TX_NS, [b"one", b"two"]) + T.honest(T.PFB_NS, [b"wrapper"])
    assert square.ParseTxs(shares) == [b"one", b"two"]
    assert square.ParseTxs(shares[1:]) == []


def test_hint_flag_by_hand():
    """Three continuation shares behind a start share; unit starts at stream bytes 0, 500 (share
    1, byte 60) and 1500 (share 3, byte 104): share 2 holds no start."""
    units = [T.pattern(498, 1), T.pattern(998, 2), T.pattern(40, 3)]
    shares = T.honest(T.TX_NS, units)
    assert [int.from_bytes(s[30:34], "big") for s in shares[1:]] == [60, 0, 104]

    def with_hint(j, r):
        out = list(shares)
        out[j] = out[j][:30] + r.to_bytes(4, "big") + out[j][34:]
        return square.compact_walk(out)

    for j, r, flag in [(1, 60, 0), (1, 61, 1), (1, 59, 1), (1, 0, 1), (1, 33, 1), (1, 512, 1), (2, 40, 1), (2, 511, 1),
                       (2, 5, 0), (2, 600, 0), (3, 104, 0), (3, 105, 1), (3, 0, 1)]:
        status, flags, got = with_hint(j, r)
        assert (status, flags, [g[0] for g in got]) == (0, flag, units), (j, r)
    # behind the share in which the last unit begins nothing is looked at
    assert square.compact_walk(shares + [T.share(T.TX_NS, 0, 77)])[1] == 0


def test_index_wrapper_and_blob_tx_round_trip():
    import square_layout as SL
    w = SL.index_wrapper(b"inner tx", [7, 300, 70000]) if hasattr(SL, "index_wrapper") else None
    mine = b"\x0a\x08inner tx\x12\x06\x07\xac\x02\xf0\xa2\x04\x1a\x04INDX"
    assert w is None or w == mine
    assert square.unwrap_index_wrapper(mine) == (b"inner tx", [7, 300, 70000])
    assert square.unwrap_index_wrapper(b"\x1a\x04INDX") == (b"", [])
    assert square.unwrap_index_wrapper(b"\x0a\x08inner tx\x1a\x04BLOB") is None
    assert square.unwrap_index_wrapper(b"\x0a\x08inner") is None
    assert square.unwrap_index_wrapper(b"not a proto") is None
    blobs = [(bytes(18) + b"\x05" * 10, b"data one"), (bytes(18) + b"\x06" * 10, b"x" * 700)]
    assert square.marshal_blob_tx(b"inner", [(bytes(1) + i, d) for i, d in blobs]) == SI.blob_tx(b"inner", blobs)


def _round_trip(txs):
    ods = square.Construct(txs)
    assert square.Deconstruct(ods) == [bytes(t) for t in txs]
    return ods


def test_block408_deconstructs_into_its_txs(block408_ods):
    txs = SI.block408_txs()
    ods = _round_trip(txs)
    golden = np.asarray(block408_ods).reshape(-1, 512)
    assert np.array_equal(ods, golden)
    got = square.Deconstruct(golden)
    assert got == txs
    assert [hashlib.sha256(t).digest() for t in got] == [hashlib.sha256(t).digest() for t in txs]


@pytest.mark.parametrize("seed", range(1, 21))
def test_random_blocks_round_trip(seed):
    _round_trip(SI.random_block(seed, seed % 7 + 1, seed % 4 + 1))


def test_edge_blocks_round_trip():
    assert square.Deconstruct(square.Construct([])) == []
    _round_trip(SI.random_block(31, 9, 0))
    _round_trip(SI.random_block(32, 0, 5))


def test_deconstruct_rejects_what_does_not_fit():
    txs = SI.random_block(33, 2, 2)
    ods = square.Construct(txs)
    runs = square._compact_runs(ods)
    # a PayForBlob unit that is no index wrapper
    bad = ods.copy()
    bad[runs[1][0]] = np.frombuffer(T.share(T.PFB_NS, 1, 38, T.unit(b"no wrapper")), np.uint8)
    bad[runs[1][0] + 1:runs[1][1]] = np.frombuffer(T.share(T.PFB_NS, 0, 0), np.uint8)
    with pytest.raises(_lib.CelError, match="not an index wrapper"):
        square.Deconstruct(bad)
    # a share index at which no blob starts
    w = b"\x0a\x02tx\x12\x01\x00\x1a\x04INDX"  # share 0 is a tx share
    bad[runs[1][0]] = np.frombuffer(T.share(T.PFB_NS, 1, 38, T.unit(w)), np.uint8)
    with pytest.raises(_lib.CelError, match="no blob starts at share"):
        square.Deconstruct(bad)
