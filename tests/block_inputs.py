"""Shared inputs and host-side helpers of the block tests (test_block_layout.py,
test_gpu_block.py): ctypes views of cel_square_construct / cel_square_layout, a numpy
expansion of a layout into share bytes, and the blocks the tests run."""
import ctypes

import numpy as np

from square_inputs import blob_msg, blob_tx, block408_txs, field_bytes, random_block

SHARE, NS = 512, 29
FIRST, CONT = 478, 482
SEG_COMPACT, SEG_BLOB, SEG_PAD = 0, 1, 2
PRIMARY_PAD_NS = bytes(28) + b"\xff"
TAIL_PAD_NS = b"\xff" * 28 + b"\xfe"


class Segment(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("start", ctypes.c_uint32), ("count", ctypes.c_uint32),
                ("share_version", ctypes.c_uint32), ("off", ctypes.c_uint64), ("len", ctypes.c_uint32),
                ("tx_index", ctypes.c_uint32), ("ns", ctypes.c_uint8 * 32)]


assert ctypes.sizeof(Segment) == 64


def lib():
    import celestia_eds._lib as L
    return L.load()


def pack(txs):
    """-> (buffer, lens, ntx, raw): the concatenated txs as the C ABI takes them."""
    txs = [bytes(t) for t in txs]
    raw = b"".join(txs)
    lens = (ctypes.c_uint32 * max(len(txs), 1))(*[len(t) for t in txs])
    return ctypes.create_string_buffer(raw, max(len(raw), 1)), lens, len(txs), raw


def construct(txs, max_square_size=128, threshold=64, greedy=0):
    """cel_square_construct -> (status, error text, k, included, shares [k*k][512] or None)."""
    l = lib()
    buf, lens, ntx, _ = pack(txs)
    k = ctypes.c_uint32()
    inc = (ctypes.c_uint8 * max(ntx, 1))()
    st = l.cel_square_construct(buf, lens, ntx, max_square_size, threshold, greedy, None, 0, ctypes.byref(k), inc)
    err = l.cel_square_last_error().decode()
    included = [int(inc[i]) for i in range(ntx)]
    if st != 0:
        return st, err, 0, included, None
    out = np.zeros((k.value * k.value, SHARE), np.uint8)
    st = l.cel_square_construct(buf, lens, ntx, max_square_size, threshold, greedy,
                                out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(k), inc)
    assert st == 0
    return st, err, k.value, included, out


def layout(txs, max_square_size=128, threshold=64, greedy=0):
    """cel_square_layout -> (status, error text, k, included, [Segment], compact [n][512])."""
    l = lib()
    buf, lens, ntx, _ = pack(txs)
    k, nseg, ncomp = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    inc = (ctypes.c_uint8 * max(ntx, 1))()
    st = l.cel_square_layout(buf, lens, ntx, max_square_size, threshold, greedy, ctypes.byref(k), inc, None, 0,
                             ctypes.byref(nseg), None, 0, ctypes.byref(ncomp))
    err = l.cel_square_last_error().decode()
    included = [int(inc[i]) for i in range(ntx)]
    if st != 0:
        return st, err, 0, included, [], None
    segs = (Segment * max(nseg.value, 1))()
    compact = np.zeros((max(ncomp.value, 1), SHARE), np.uint8)
    st = l.cel_square_layout(buf, lens, ntx, max_square_size, threshold, greedy, ctypes.byref(k), inc, segs,
                             nseg.value, ctypes.byref(nseg), compact.ctypes.data_as(ctypes.c_void_p), ncomp.value,
                             ctypes.byref(ncomp))
    assert st == 0
    return st, err, k.value, included, list(segs[:nseg.value]), compact[:ncomp.value]


def sparse_shares(n):
    return 0 if n == 0 else 1 if n <= FIRST else 1 + (n - FIRST + CONT - 1) // CONT


def expand(raw, k, segs, compact):
    """The bytes of a layout, restated with numpy: [k*k][512]."""
    out = np.full((k * k, SHARE), 0xEE, np.uint8)  # a share no segment covers keeps 0xEE
    for s in segs:
        a, b = s.start, s.start + s.count
        ns = np.frombuffer(bytes(s.ns)[:NS], np.uint8)
        if s.kind == SEG_COMPACT:
            out[a:b] = compact[s.off:s.off + s.count]
        elif s.kind == SEG_PAD:
            out[a:b] = 0
            out[a:b, :NS] = ns
            out[a:b, NS] = 1
        else:
            assert s.kind == SEG_BLOB and s.count == sparse_shares(s.len)
            payload = np.zeros(FIRST + CONT * (s.count - 1), np.uint8)
            payload[:s.len] = np.frombuffer(raw[s.off:s.off + s.len], np.uint8)
            out[a:b] = 0
            out[a:b, :NS] = ns
            out[a:b, NS] = (s.share_version << 1) & 0xFF
            out[a, NS] |= 1
            out[a, NS + 1:NS + 5] = np.frombuffer(int(s.len).to_bytes(4, "big"), np.uint8)
            out[a, NS + 5:] = payload[:FIRST]
            if s.count > 1:
                out[a + 1:b, NS + 1:] = payload[FIRST:].reshape(-1, CONT)
    return out


def segment(kind, start, count, ns29, off=0, length=0, share_version=0, tx_index=0):
    return Segment(kind, start, count, share_version, off, length, tx_index, (ctypes.c_uint8 * 32)(*bytes(ns29)))


def blob_layout(lengths, k, seed, version1=()):
    """A hand-made layout without txs: one random blob per length, back to back in the byte
    buffer and in the square (share version 1 for the blobs listed in version1), then tail
    padding to the end of the k x k square. -> (raw bytes, [Segment])"""
    rng = np.random.default_rng(seed)
    raw = rng.bytes(int(sum(lengths)))
    segs, off, start = [], 0, 0
    for i, n in enumerate(lengths):
        ns = bytes(19) + rng.integers(0, 256, 10, np.uint8).tobytes()
        segs.append(segment(SEG_BLOB, start, sparse_shares(n), ns, off, n, 1 if i in version1 else 0))
        off += n
        start += sparse_shares(n)
    assert start <= k * k
    if start < k * k:
        segs.append(segment(SEG_PAD, start, k * k - start, TAIL_PAD_NS))
    return raw, segs


def dropping_block():
    """30 blob txs after 4 normal ones: at max_square_size 8 Construct fails at tx 12 and
    Build keeps the first 12."""
    return random_block(4, 4, 30, max_blob=3000)


def misordered_block():
    """A normal tx after a blob tx: square.Construct's ordering error."""
    t = random_block(9, 2, 1)
    return [t[0], t[2], t[1]]


# (name, txs, max_square_size, expected k or None where Construct fails)
def layout_blocks():
    return [("block408", block408_txs(), 128, 32),
            ("empty", [], 128, 1),
            ("no_blobs", random_block(3, 5, 0), 128, 4),
            ("no_normal", random_block(2, 0, 6), 128, 16),
            ("ns_padding", random_block(1, 3, 4, max_blob=60000), 128, 32),
            ("dropping", dropping_block(), 8, None),
            ("misordered", misordered_block(), 128, None)]


EDGE_LENGTHS = [1, 477, 478, 479, 959, 960, 961, 1442, 1443, 6000, 40000, 31000, 2, 70000]


def _edge_txs(inner0):
    rng = np.random.default_rng(2024)
    txs = [rng.integers(0, 256, n, np.uint8).tobytes() for n in (90, 333, 601)]
    groups = [EDGE_LENGTHS[0:4], EDGE_LENGTHS[4:8], EDGE_LENGTHS[8:11], EDGE_LENGTHS[11:14]]
    for g, lens in enumerate(groups):
        blobs = [(bytes(18) + rng.integers(0, 256, 10, np.uint8).tobytes(),
                  rng.integers(0, 256, n, np.uint8).tobytes()) for n in lens]
        txs.append(blob_tx(rng.integers(0, 256, inner0 + g, np.uint8).tobytes(), blobs))
    return txs


def edge_block():
    """Blobs at every share boundary (EDGE_LENGTHS) over four blob txs after three normal
    txs, with the inner-tx length raised from 200 until the blobs' data offsets in the
    concatenated txs take every value mod 4. -> (txs, layout segments)."""
    for inner0 in range(200, 240):
        txs = _edge_txs(inner0)
        st, _, k, _, segs, _ = layout(txs)
        assert st == 0
        if {s.off % 4 for s in segs if s.kind == SEG_BLOB} == {0, 1, 2, 3}:
            return txs, segs
    raise AssertionError("no inner-tx length gives all four offset residues")


def version1_block():
    """One blob tx whose blob has share version 1, after one normal tx."""
    rng = np.random.default_rng(77)
    ns_id = bytes(18) + rng.integers(0, 256, 10, np.uint8).tobytes()
    data = rng.integers(0, 256, 1500, np.uint8).tobytes()
    tx = field_bytes(1, rng.integers(0, 256, 180, np.uint8).tobytes()) + \
        field_bytes(2, blob_msg(ns_id, data, share_version=1)) + field_bytes(3, b"BLOB")
    return [rng.integers(0, 256, 120, np.uint8).tobytes(), tx]


def mib_block():
    """Nine blob txs of one 1 MiB blob each: k = 256 at max_square_size 256."""
    rng = np.random.default_rng(256)
    txs = []
    for i in range(9):
        ns_id = bytes(18) + rng.integers(0, 256, 10, np.uint8).tobytes()
        txs.append(blob_tx(rng.integers(0, 256, 200 + i, np.uint8).tobytes(),
                           [(ns_id, rng.integers(0, 256, 1 << 20, np.uint8).tobytes())]))
    return txs
