"""GPU: txs out of a resident square (cel_dev_txs_plan / cel_dev_txs_emit, cel_txs_by_range,
TreeIndex.txs_flat, ExtendedDataSquare.Txs, square.Deconstruct over a TreeIndex). The checker is
the host parser square.compact_walk (pinned in test_tx_parse.py) and hashlib: records, status,
flags, bytes, padding zeros and hashes must equal it for every range."""
import ctypes
import hashlib

import numpy as np
import pytest

import square_inputs as SI
import tx_cases as T
from celestia_eds import _lib, block, proof, square
from celestia_eds.rsmt2d import ExtendedDataSquare

pytestmark = pytest.mark.gpu

FILLER = T.share(T.BLOB_NS, 1, 0)  # what lies between the cases: no range covers it


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def eds_of(ods, k, fill=0):
    """A (2k, 2k, 512) square with Q0 = ods ([k*k][512]) and `fill` everywhere else."""
    eds = np.full((2 * k, 2 * k, T.SHARE), fill, np.uint8)
    eds[:k, :k] = np.asarray(ods, np.uint8).reshape(k, k, T.SHARE)
    return eds


def packed(k, runs, gap=0):
    """A k*k ODS of filler with the runs of shares one behind the other, `gap` shares between
    them, and the range of each."""
    ods = np.tile(np.frombuffer(FILLER, np.uint8), (k * k, 1))
    ranges, at = [], 0
    for sh in runs:
        assert at + len(sh) <= k * k
        ods[at:at + len(sh)] = T.as_array(sh)
        ranges.append((at, at + len(sh)))
        at += len(sh) + gap
    return ods, ranges


def mirror(ods, ranges):
    """Per range (status, flags, [(bytes, ODS share, share_off, shares)]) by the host parser."""
    out = []
    for a, b in ranges:
        status, flags, units = square.compact_walk(ods[a:b])
        out.append((status, flags, [(d, s + a, off, n) for d, s, off, n in units]))
    return out


def by_range(ctx, eds, k, ranges, hashes=True):
    """cel_txs_by_range: count, then fetch."""
    n = len(ranges)
    starts = np.array([a for a, _ in ranges] or [0], np.uint32)
    ends = np.array([b for _, b in ranges] or [0], np.uint32)
    status, flags = np.full(max(n, 1), 77, np.uint32), np.full(max(n, 1), 77, np.uint32)
    nu, tb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    cells = np.ascontiguousarray(eds)
    ctx.check(ctx.lib.cel_txs_by_range(ctx.handle, p(cells), k, n, p(starts), p(ends), 0, 0, None, p(status), p(flags),
                                       None, None, ctypes.byref(nu), ctypes.byref(tb)))
    cap, nbytes = nu.value, tb.value
    recs = (square.TxRec * max(cap, 1))()
    data, hs = np.zeros(max(nbytes, 1), np.uint8), np.zeros((max(cap, 1), 32), np.uint8)
    ctx.check(ctx.lib.cel_txs_by_range(ctx.handle, p(cells), k, n, p(starts), p(ends), cap, nbytes, recs, p(status),
                                       p(flags), p(data), p(hs) if hashes else None, ctypes.byref(nu), ctypes.byref(tb)))
    assert (nu.value, tb.value) == (cap, nbytes)
    return list(recs[:cap]), status[:n], flags[:n], data[:nbytes], hs[:cap]


def check_result(got, want):
    recs, status, flags, data, hs = got
    assert [int(s) for s in status] == [w[0] for w in want]
    assert [int(f) for f in flags] == [w[1] for w in want]
    flat = [(r, u) for r, w in enumerate(want) for u in w[2]]
    assert len(recs) == len(flat)
    at = 0
    for i, (rec, (r, (d, share, off, n))) in enumerate(zip(recs, flat)):
        assert (rec.range, rec.share, rec.share_off, rec.shares, rec.len) == (r, share, off, n, len(d)), i
        assert rec.data_off == at and at % 16 == 0
        assert data[at:at + len(d)].tobytes() == d, i
        at += (len(d) + 15) // 16 * 16
        assert not data[rec.data_off + len(d):at].any(), "the bytes up to the next multiple of 16 are zero"
        assert hs[i].tobytes() == hashlib.sha256(d).digest(), i
    assert len(data) == at


def check_against_mirror(ctx, ods, k, ranges, host_form=True, index=None):
    want = mirror(ods, ranges)
    eds = eds_of(ods, k)
    index = index or proof.TreeIndex(eds, ctx=ctx)
    check_result(index.txs_flat(ranges), want)
    if host_form:
        check_result(by_range(ctx, eds, k, ranges), want)
    return index, want


def groups(runs, room):
    """The runs in order, split into groups of at most `room` shares."""
    out, cur = [], []
    for sh in runs:
        if sum(len(s) for s in cur) + len(sh) > room:
            out.append(cur)
            cur = []
        cur.append(sh)
    return out + [cur]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_rules_by_hand(ctx, k):
    at = 0
    for group in groups([c[1] for c in T.HAND], k * k):
        ods, ranges = packed(k, group)
        _, want = check_against_mirror(ctx, ods, k, ranges, host_form=(k == 8 or at == 0))
        for w, case in zip(want, T.HAND[at:at + len(group)]):
            assert (w[0], [u[0] for u in w[2]]) == (case[2], case[3]), case[0]
        at += len(group)
    assert at == len(T.HAND)


@pytest.mark.parametrize("k", [4, 8])
def test_honest_streams(ctx, k):
    runs = [T.honest(ns, units) for units in T.HONEST.values() for ns in (T.TX_NS, T.PFB_NS)]
    runs = [sh for sh in runs if len(sh) <= k * k]
    assert len(runs) >= 24
    for group in groups(runs, k * k):
        ods, ranges = packed(k, group)
        _, want = check_against_mirror(ctx, ods, k, ranges, host_form=False)
        assert all(w[:2] == (0, 0) and w[2] for w in want)


def test_damaged_hints(ctx):
    k = 8
    runs = []
    for _, units, j, r in T.DAMAGED_HINTS:
        sh = T.honest(T.TX_NS, units)
        runs += [T.with_reserved(sh, j, r), sh]  # each damaged range beside the honest one
    ods, ranges = packed(k, runs)
    _, want = check_against_mirror(ctx, ods, k, ranges)
    for i, (name, units, j, r) in enumerate(T.DAMAGED_HINTS):
        bad, good = want[2 * i], want[2 * i + 1]
        assert bad[:2] == (0, _lib.TX_FHINTS) and good[:2] == (0, 0), name
        assert [u[0] for u in good[2]] == units
        if j:
            assert [u[0] for u in bad[2]] == units, name
        else:
            assert len(bad[2]) == 201, name


@pytest.fixture(scope="module")
def long_stream():
    """A k = 32 ODS: 300 shares of one tx stream whose units cross 256 within two shares and in
    all, then the edge lengths as a PFB stream."""
    rng = np.random.default_rng(5)
    units = [bytes([i]) for i in range(239)] * 2 + [rng.integers(0, 256, int(n), np.uint8).tobytes()
                                                    for n in rng.integers(1, 900, 330)]
    tx = T.honest(T.TX_NS, units)
    assert len(tx) >= 300
    pfb = T.honest(T.PFB_NS, T.HONEST["edge lengths"])
    ods, ranges = packed(32, [tx[:300], pfb])
    return ods, ranges


def test_scan_block_edges(ctx, long_stream):
    ods, (tx, pfb) = long_stream
    ranges = [(0, 255), (0, 256), (0, 257), (1, 257), tx, pfb, (tx[0], pfb[1])]
    index, want = check_against_mirror(ctx, ods, 32, ranges)
    assert [w[:2] for w in want[:6]] == [(0, 0)] * 6
    for total in (255, 256, 257):  # plans of one scan block less one share, one block, one block and a share
        check_against_mirror(ctx, ods, 32, [(0, total)], host_form=False, index=index)
        check_against_mirror(ctx, ods, 32, [(3, 100), (100, total + 3)], host_form=False, index=index)  # 97 + the rest
    assert len(want[0][2]) > 256 and [len(u[0]) for u in want[5][2]] == T.EDGE_LENGTHS
    assert want[3][2], "a range that begins inside a stream begins at the unit its first share names"


def test_range_geometry(ctx, long_stream):
    ods, (tx, pfb) = long_stream
    k = 32
    ranges = [(0, 40), (40, 90), (90, 300),   # ordered
              (20, 60), (0, 300),             # overlapping
              (40, 90), (40, 90),             # repeated
              (7, 7), (0, 0), (k * k, k * k),  # empty
              (pfb[0] - 2, pfb[1] + 1),       # runs into the filler: a namespace error
              (295, pfb[0] + 3)]              # two namespaces in one range
    index, want = check_against_mirror(ctx, ods, k, ranges)
    assert want[10][0] == T.ENAMESPACE and want[5] == want[6] == want[1]
    assert [w[2] for w in want[7:10]] == [[], [], []]
    recs, status, flags, data, hs = index.txs_flat([])
    assert (len(recs), len(status), len(flags), len(data), len(hs)) == (0, 0, 0, 0, 0)
    assert index.txs([]) == [] and index.txs([(3, 3), (0, 0)]) == [[], []]
    got = index.txs(ranges[:2] + [ranges[10]])
    assert got[:2] == [[u[0] for u in w[2]] for w in want[:2]]
    assert isinstance(got[2], square.TxParseError) and got[2].kind == T.ENAMESPACE
    check_result(by_range(ctx, eds_of(ods, k), k, []), [])


def test_only_q0_is_read(ctx):
    k = 8
    ods, ranges = packed(k, [T.honest(T.TX_NS, T.HINT_UNITS), T.honest(T.PFB_NS, T.NESTED_UNITS)])
    outs = []
    for fill in (0, 0xA5):
        recs, status, flags, data, hs = proof.TreeIndex(eds_of(ods, k, fill), ctx=ctx).txs_flat(ranges)
        outs.append(([bytes(r) for r in recs], status.tobytes(), flags.tobytes(), data.tobytes(), hs.tobytes()))
    assert outs[0] == outs[1] and len(outs[0][0]) == 6


def test_byte_damage_corpus(ctx):
    cases = T.corpus(T.CORPUS_SEED)
    assert len(cases) == 300
    host = [square.compact_walk(c) for c in cases]
    assert {h[0] for h in host} == {0, T.EVERSION, T.ENAMESPACE, T.ERESERVED, T.EVARINT}
    assert any(h[1] == _lib.TX_FHINTS for h in host)
    assert sum(1 for h in host if h[2]) * 2 >= len(cases)
    ods, ranges = packed(32, cases)
    check_against_mirror(ctx, ods, 32, ranges, host_form=False)


def _plan(index, starts, ends, status=None, flags=None):
    import torch
    c = index.ctx
    n = len(starts)
    s, e = np.array(starts or [0], np.uint32), np.array(ends or [0], np.uint32)
    total = int(sum(b - a for a, b in zip(starts, ends)))
    d_work = torch.empty((max(c.lib.cel_dev_txs_workspace_size(total, n), 16),), dtype=torch.uint8, device=index._dev)
    cnt, tb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    st = c.lib.cel_dev_txs_plan(c.handle, index._ptr(index.d_eds), index.k, n, p(s), p(e),
                                p(status) if status is not None else None, p(flags) if flags is not None else None,
                                ctypes.byref(cnt), ctypes.byref(tb), index._ptr(d_work), index._stream_ptr())
    return st, cnt.value, tb.value, d_work


def test_abi_conventions(ctx):
    import torch
    k = 8
    ods, ranges = packed(k, [T.honest(T.TX_NS, T.HINT_UNITS)])
    eds = eds_of(ods, k)
    index = proof.TreeIndex(eds, ctx=ctx)
    c, lib = index.ctx, index.ctx.lib
    lengths = [len(u) for u in T.HINT_UNITS]
    nbytes = sum((n + 15) // 16 * 16 for n in lengths)
    a, b = ranges[0]
    # the plan call counts; status and flags are optional
    status, flags = np.full(1, 77, np.uint32), np.full(1, 77, np.uint32)
    assert _plan(index, [a], [b])[:3] == (_lib.OK, 3, nbytes)
    assert _plan(index, [a], [b], status, flags)[:3] == (_lib.OK, 3, nbytes) and (status[0], flags[0]) == (0, 0)
    # n_ranges = 0; bad ranges and widths; nil and misaligned arguments
    assert _plan(index, [], [])[:3] == (_lib.OK, 0, 0)
    assert _plan(index, [5], [4])[0] == _lib.EINVAL
    assert _plan(index, [0], [k * k + 1])[0] == _lib.EINVAL
    s = np.zeros(1, np.uint32)
    cnt, tb = ctypes.c_uint64(), ctypes.c_uint64()
    d_work = torch.empty((1 << 16,), dtype=torch.uint8, device=index._dev)
    plan = lambda kk, d_eds, work, nu=ctypes.byref(cnt), se=(p(s), p(s)): lib.cel_dev_txs_plan(
        c.handle, d_eds, kk, 1, se[0], se[1], None, None, nu, ctypes.byref(tb), work, index._stream_ptr())
    assert plan(3, index._ptr(index.d_eds), index._ptr(d_work)) == _lib.EINVAL
    assert plan(1024, index._ptr(index.d_eds), index._ptr(d_work)) == _lib.EINVAL
    assert plan(k, None, index._ptr(d_work)) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), None) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), index._ptr(d_work), None) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), index._ptr(d_work), se=(None, p(s))) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), ctypes.c_void_p(d_work.data_ptr() + 4)) == _lib.EINVAL
    assert plan(k, index._ptr(index.d_eds), index._ptr(d_work)) == _lib.OK
    assert lib.cel_dev_txs_workspace_size(1 << 31, 1) == 0 and lib.cel_dev_txs_workspace_size(0, 0) > 0
    # the workspace is linear in the shares, whatever they hold
    assert lib.cel_dev_txs_workspace_size(1 << 18, 1) <= 128 * (1 << 18) + (1 << 14)
    # the emit call: a NULL d_hashes gives records and bytes alone; it runs over no more units
    # than the plan holds, whatever it is passed
    st, n_units, tb_, d_work = _plan(index, [a], [b])
    assert st == _lib.OK
    d_recs = torch.full((32 * 8,), 0xCC, dtype=torch.uint8, device=index._dev)
    d_data = torch.full((nbytes + 64,), 0xCC, dtype=torch.uint8, device=index._dev)
    emit = lambda n, recs, data, work, hs=None: lib.cel_dev_txs_emit(c.handle, index._ptr(index.d_eds), k, n, recs, data,
                                                                     hs, work, index._stream_ptr())
    assert emit(1000, index._ptr(d_recs), index._ptr(d_data), index._ptr(d_work)) == _lib.OK
    index._stream.synchronize()
    got, raw = d_data.cpu().numpy(), d_recs.cpu().numpy()
    assert (got[nbytes:] == 0xCC).all() and (raw[32 * 3:] == 0xCC).all(), "nothing is written past the plan"
    recs = (square.TxRec * 3).from_buffer_copy(raw[:96].tobytes())
    for r, u in zip(recs, T.HINT_UNITS):
        assert r.len == len(u) and got[r.data_off:r.data_off + r.len].tobytes() == u
    # the first unit alone
    d_data.fill_(0xCC)
    d_recs.fill_(0xCC)
    assert emit(1, index._ptr(d_recs), index._ptr(d_data), index._ptr(d_work)) == _lib.OK
    index._stream.synchronize()
    assert (d_data.cpu().numpy()[512:] == 0xCC).all() and (d_recs.cpu().numpy()[32:] == 0xCC).all()
    assert d_data.cpu().numpy()[:498].tobytes() == T.HINT_UNITS[0]
    # a workspace that holds no plan of this context, nil and misaligned buffers
    other = torch.empty((1 << 16,), dtype=torch.uint8, device=index._dev)
    assert emit(3, index._ptr(d_recs), index._ptr(d_data), index._ptr(other)) == _lib.EINVAL
    assert emit(3, None, index._ptr(d_data), index._ptr(d_work)) == _lib.EINVAL
    assert emit(3, index._ptr(d_recs), None, index._ptr(d_work)) == _lib.EINVAL
    assert emit(3, index._ptr(d_recs), ctypes.c_void_p(d_data.data_ptr() + 8), index._ptr(d_work)) == _lib.EINVAL
    assert emit(3, index._ptr(d_recs), index._ptr(d_data), index._ptr(d_work),
                ctypes.c_void_p(d_data.data_ptr() + 8)) == _lib.EINVAL
    assert emit(0, None, None, None) == _lib.OK
    # the host-memory form: count only, caps that are too small, nil arguments
    cells = np.ascontiguousarray(eds)
    s, e = np.array([a], np.uint32), np.array([b], np.uint32)
    nu, tb = ctypes.c_uint64(99), ctypes.c_uint64(99)
    recs = (square.TxRec * 3)()
    data = np.zeros(nbytes, np.uint8)
    call = lambda cap, data_cap, r, d, cl=p(cells), kk=k: lib.cel_txs_by_range(
        c.handle, cl, kk, 1, p(s), p(e), cap, data_cap, r, p(status), p(flags), d, None, ctypes.byref(nu), ctypes.byref(tb))
    assert call(0, 0, None, None) == _lib.OK and (nu.value, tb.value) == (3, nbytes)
    for cap, data_cap in ((2, nbytes), (3, nbytes - 16)):
        status[0] = 77
        assert call(cap, data_cap, recs, p(data)) == _lib.EINVAL
        assert (nu.value, tb.value, status[0]) == (3, nbytes, 0)
        msg = lib.cel_last_error(c.handle).decode()
        assert str(cap) in msg and "3 units" in msg, msg
    assert call(3, nbytes, recs, p(data)) == _lib.OK and data[:498].tobytes() == T.HINT_UNITS[0]
    assert call(3, nbytes, None, p(data)) == _lib.EINVAL
    assert call(3, nbytes, recs, None) == _lib.EINVAL
    assert call(3, nbytes, recs, p(data), cl=None) == _lib.EINVAL
    assert call(3, nbytes, recs, p(data), kk=12) == _lib.EINVAL
    e[0] = k * k + 1
    assert call(3, nbytes, recs, p(data)) == _lib.EINVAL
    assert lib.cel_txs_by_range(c.handle, p(cells), k, 1, p(s), p(s), 0, 0, None, None, None, None, None, None,
                                ctypes.byref(tb)) == _lib.EINVAL


@pytest.fixture(scope="module")
def blocks(ctx):
    out = []
    for txs in (SI.block408_txs(), SI.random_block(41, 12, 4), SI.random_block(42, 3, 7, max_blob=3000)):
        b = block.block_extend(ctx, txs, want_eds=True)
        out.append((txs, b, proof.TreeIndex(b.eds, ctx=ctx)))
    return out


def test_share_ranges_equal_tx_share_range(ctx, blocks):
    from celestia_eds import blob
    for txs, b, index in blocks:
        runs = blob.ods_ranges(index.k, 2, index.namespace_flat([square.TX_NAMESPACE, square.PFB_NAMESPACE]))
        recs, status, flags, data, hs = index.txs_flat(runs)
        assert list(status) == [0, 0] and list(flags) == [0, 0] and len(recs) == len(txs)
        for i, r in enumerate(recs):
            assert (r.share, r.share + r.shares) == square.TxShareRange(txs, i), i
        n_normal = sum(1 for r in recs if r.range == 0)
        assert [data[r.data_off:r.data_off + r.len].tobytes() for r in recs[:n_normal]] == txs[:n_normal]
        assert [h.tobytes() for h in hs[:n_normal]] == [hashlib.sha256(t).digest() for t in txs[:n_normal]]


def test_deconstruct_from_the_device(ctx, blocks):
    for txs, b, index in blocks:
        assert square.Deconstruct(index) == txs
    empty = block.block_extend(ctx, [], want_eds=True)
    assert square.Deconstruct(proof.TreeIndex(empty.eds, ctx=ctx)) == []


def test_host_memory_form_equals_the_device_form(ctx, blocks):
    from celestia_eds import blob
    for txs, b, index in blocks:
        eds = ExtendedDataSquare(b.eds, b.row_roots, b.col_roots, ctx=ctx)
        runs = blob.ods_ranges(index.k, 2, index.namespace_flat([square.TX_NAMESPACE, square.PFB_NAMESPACE]))
        assert list(eds.Txs()) == index.txs(runs)
        (normal, h_normal), (wrappers, h_wrappers) = eds.Txs(hashes=True)
        assert h_normal == [hashlib.sha256(t).digest() for t in normal]
        assert h_wrappers == [hashlib.sha256(t).digest() for t in wrappers]
        assert square.Deconstruct(eds) == txs
