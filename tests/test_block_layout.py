"""CPU: cel_square_layout (the square without its blob bytes) against cel_square_construct:
the layout's segments and compact shares, expanded into bytes with numpy, equal the byte
builder's square, with the same k, included[], status and error string; the segments are
ascending, disjoint and cover [0, k*k). And the block entry points reject nil arguments
before any device call."""
import ctypes

import numpy as np
import pytest

import block_inputs as B

BLOCKS = B.layout_blocks()


def _check(txs, max_square_size, greedy):
    st_c, err_c, k_c, inc_c, shares = B.construct(txs, max_square_size, 64, greedy)
    st_l, err_l, k_l, inc_l, segs, compact = B.layout(txs, max_square_size, 64, greedy)
    assert (st_l, err_l, k_l, inc_l) == (st_c, err_c, k_c, inc_c)
    if st_c != 0:
        return st_c, err_c, 0, inc_c, []
    at = 0
    for s in segs:  # ascending, disjoint, no empty segment, covering [0, k*k)
        assert s.start == at and s.count > 0 and s.kind in (B.SEG_COMPACT, B.SEG_BLOB, B.SEG_PAD)
        at += s.count
    assert at == k_l * k_l
    got = B.expand(b"".join(txs), k_l, segs, compact)
    assert np.array_equal(got, shares)
    # a blob segment names the tx that carries it: its bytes lie inside that tx
    bounds = np.cumsum([0] + [len(t) for t in txs])
    for s in segs:
        if s.kind == B.SEG_BLOB:
            assert bounds[s.tx_index] <= s.off and s.off + s.len <= bounds[s.tx_index + 1]
            assert inc_l[s.tx_index] == 2
    return st_c, err_c, k_l, inc_c, segs


@pytest.mark.parametrize("name,txs,max_square_size,k", BLOCKS, ids=[b[0] for b in BLOCKS])
@pytest.mark.parametrize("greedy", [0, 1])
def test_layout_expands_to_the_constructed_square(name, txs, max_square_size, k, greedy):
    import celestia_eds._lib as L
    st, err, got_k, included, segs = _check(txs, max_square_size, greedy)
    if k is not None:
        assert st == 0 and got_k == k
    pads = [bytes(s.ns)[:B.NS] for s in segs if s.kind == B.SEG_PAD]
    blob_ns = {bytes(s.ns)[:B.NS] for s in segs if s.kind == B.SEG_BLOB}
    if name == "block408":
        assert B.PRIMARY_PAD_NS in pads and B.TAIL_PAD_NS in pads
    elif name == "empty":
        assert len(segs) == 1 and segs[0].kind == B.SEG_PAD and segs[0].count == 1 and pads == [B.TAIL_PAD_NS]
    elif name == "no_blobs":
        assert not blob_ns and segs[0].kind == B.SEG_COMPACT
    elif name == "no_normal":
        assert blob_ns and all(i == 2 for i in included)
    elif name == "ns_padding":
        assert any(p in blob_ns for p in pads), "no namespace padding between blobs"
    elif name == "dropping":
        if greedy:
            assert st == 0 and got_k == 8 and included == [1] * 4 + [2] * 8 + [0] * 22
        else:
            assert (st, err) == (L.ETOOBIG, "not enough space to append blob tx at index 12")
    elif name == "misordered":
        if greedy:
            assert st == 0 and included == [1, 2, 1]
        else:
            assert (st, err) == (L.EINVAL, "normal transaction at index 2 can not be appended after blob tx")


def test_edge_block_shape():
    """The GPU share-edge block: k = 32, a namespace-padding share, every offset residue."""
    txs, segs = B.edge_block()
    st, _, k, _, _ = _check(txs, 128, 0)
    assert st == 0 and k == 32
    blobs = [s for s in segs if s.kind == B.SEG_BLOB]
    assert sorted(s.len for s in blobs) == sorted(B.EDGE_LENGTHS)
    assert {s.off % 4 for s in blobs} == {0, 1, 2, 3}
    blob_ns = {bytes(s.ns)[:B.NS] for s in blobs}
    assert any(s.kind == B.SEG_PAD and bytes(s.ns)[:B.NS] in blob_ns for s in segs)


def test_mib_block_shape():
    import celestia_eds._lib as L
    txs = B.mib_block()
    st, err, k, _, _, _ = B.layout(txs, 256)
    assert st == 0 and k == 256
    st, err, _, _, _, _ = B.layout(txs, 128)
    assert (st, err) == (L.ETOOBIG, "not enough space to append blob tx at index 7")


def test_layout_sizing_and_argument_errors():
    import celestia_eds._lib as L
    l = L.load()
    buf, lens, ntx, _ = B.pack(B.block408_txs())
    k, nseg, ncomp = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    args = (buf, lens, ntx, 128, 64, 0)
    assert l.cel_square_layout(*args, ctypes.byref(k), None, None, 0, ctypes.byref(nseg), None, 0,
                               ctypes.byref(ncomp)) == L.OK
    assert k.value == 32 and nseg.value >= 4 and ncomp.value >= 1
    segs = (B.Segment * nseg.value)()
    comp = (ctypes.c_uint8 * (ncomp.value * 512))()
    n2, c2 = ctypes.c_uint32(), ctypes.c_uint32()
    # a segment array or a compact buffer below the counts
    assert l.cel_square_layout(*args, ctypes.byref(k), None, segs, nseg.value - 1, ctypes.byref(n2), comp, ncomp.value,
                               ctypes.byref(c2)) == L.EINVAL
    assert (n2.value, c2.value) == (nseg.value, ncomp.value)
    assert l.cel_square_layout(*args, ctypes.byref(k), None, segs, nseg.value, ctypes.byref(n2), comp, ncomp.value - 1,
                               ctypes.byref(c2)) == L.EINVAL
    assert l.cel_square_layout(*args, None, None, None, 0, ctypes.byref(n2), None, 0, ctypes.byref(c2)) == L.EINVAL
    assert l.cel_square_layout(buf, lens, ntx, 100, 64, 0, ctypes.byref(k), None, None, 0, ctypes.byref(n2), None, 0,
                               ctypes.byref(c2)) == L.EINVAL
    assert l.cel_square_last_error().decode() == "invalid argument"


def test_block_entry_points_validate_without_a_device():
    import celestia_eds._lib as L
    l = L.load()
    buf, lens, ntx, _ = B.pack(B.block408_txs())
    k, n = ctypes.c_uint32(), ctypes.c_uint32()
    rr = (ctypes.c_uint8 * (256 * 90))()
    dah = (ctypes.c_uint8 * 32)()
    seg = (B.Segment * 1)()
    assert l.cel_block_extend(None, buf, lens, ntx, 128, 64, 0, ctypes.byref(k), None, rr, rr, dah, None, 0, None, None,
                              0, ctypes.byref(n), 0) == L.EINVAL
    assert l.cel_dev_square_build(None, None, seg, 1, None, 0, 1, rr, None) == L.EINVAL
    assert l.cel_dev_square_build(None, None, None, 0, None, 0, 0, None, None) == L.EINVAL
