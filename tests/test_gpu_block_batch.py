"""GPU: the batched block path (cel_block_extend_batch, cel_dev_square_build_batch,
celestia_eds.block's ExtendBlocks / ProcessProposals), bit-exact against the single calls it
batches: cel_block_extend per block and cel_dev_square_build per layout, themselves checked
against the three-call path in test_gpu_block.py."""
import ctypes

import numpy as np
import pytest

import block_inputs as B
from test_gpu_block import block_extend

pytestmark = pytest.mark.gpu

MISORDERED = "normal transaction at index 2 can not be appended after blob tx"


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Result:
    pass


def batch_extend(ctx, blocks, max_square_size=128, greedy=0, cap=None, host_threads=1, max_eds_bytes=0,
                 roots_cap=None, threshold=64):
    """cel_block_extend_batch through the raw ABI. cap: commitment capacity (None = every blob of
    every block, 0 = skip); roots_cap: nodes (None = n * 2 * max_square_size). Outputs are
    pre-filled, so what is written shows."""
    l = ctx.lib
    flat = [bytes(t) for b in blocks for t in b]
    buf, lens, ntx, _ = B.pack(flat)
    n = len(blocks)
    nt = np.array([len(b) for b in blocks] + [0], np.uint32)
    r = Result()
    ncom = ctypes.c_uint32(0xFFFFFFFF)
    if cap is None:
        c = ctypes.c_uint32()
        assert l.cel_blob_tx_commitments(ctx.handle, buf, lens, ntx, 64, None, None, 0, ctypes.byref(c)) == 0
        cap = c.value
    if roots_cap is None:
        roots_cap = n * 2 * max_square_size
    r.k = np.full(max(n, 1), 0xABCD, np.uint32)
    r.st = np.full(max(n, 1), 0x1234, np.int32)
    r.inc = np.full(max(ntx, 1), 0x99, np.uint8)
    r.rr = np.full((max(roots_cap, 1), 90), 0xC3, np.uint8)
    r.cr = np.full((max(roots_cap, 1), 90), 0xC3, np.uint8)
    r.root_off = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    r.dah = np.full((max(n, 1), 32), 0x77, np.uint8)
    com = np.full((max(cap, 1), 32), 0x55, np.uint8)
    cb = np.full(max(cap, 1), 0xEEEEEEEE, np.uint32)
    ct = np.full(max(cap, 1), 0xEEEEEEEE, np.uint32)
    r.status = l.cel_block_extend_batch(ctx.handle, buf, lens, _p(nt), n, max_square_size, threshold, greedy,
                                        host_threads, max_eds_bytes, _p(r.k), _p(r.st), _p(r.inc), _p(r.rr), _p(r.cr),
                                        _p(r.root_off), roots_cap, _p(r.dah), _p(com) if cap else None,
                                        _p(cb) if cap else None, _p(ct) if cap else None, cap, ctypes.byref(ncom),
                                        None, 1)
    r.error = l.cel_last_error(ctx.handle).decode() if r.status else ""
    r.errors = [l.cel_block_batch_error(ctx.handle, i).decode() for i in range(n)]
    r.n_commit, r.cap, r.com, r.cb, r.ct = ncom.value, cap, com, cb, ct
    r.tx0 = np.concatenate([[0], np.cumsum(nt[:n])]).astype(int)
    return r


def untouched(r):
    return ((r.k == 0xABCD).all() and (r.st == 0x1234).all() and (r.inc == 0x99).all() and (r.rr == 0xC3).all() and
            (r.cr == 0xC3).all() and (r.root_off == 0xFFFFFFFF).all() and (r.dah == 0x77).all() and
            (r.com == 0x55).all() and (r.cb == 0xEEEEEEEE).all())


def block_of(r, i):
    """Block i's outputs of a batch result, shaped like a single call's."""
    o = Result()
    o.status, o.error, o.k = int(r.st[i]), r.errors[i], int(r.k[i])
    o.included = [int(x) for x in r.inc[r.tx0[i]:r.tx0[i + 1]]]
    a, b = int(r.root_off[i]), int(r.root_off[i + 1])
    o.row_roots, o.col_roots, o.dah = r.rr[a:b], r.cr[a:b], r.dah[i].tobytes()
    o.commitments = [(int(r.ct[j]), r.com[j].tobytes()) for j in range(min(r.n_commit, r.cap)) if r.cb[j] == i]
    return o


def assert_block(got, want, commitments=True):
    """got: a batch's block; want: cel_block_extend's result for the same txs."""
    assert (got.status, got.error) == (want.status, want.error)
    if want.status:
        assert got.k == 0 and len(got.row_roots) == 0 and got.dah == bytes(32) and not any(got.included)
        assert got.commitments == []
        return
    k = want.k
    assert got.k == k and got.included == want.included
    assert len(got.row_roots) == 2 * k
    assert np.array_equal(got.row_roots, want.row_roots[:2 * k]) and np.array_equal(got.col_roots, want.col_roots[:2 * k])
    assert got.dah == want.dah
    if commitments:
        assert got.commitments == want.commitments


def assert_batch(r, singles, commitments=True):
    n = len(singles)
    for i, want in enumerate(singles):
        assert_block(block_of(r, i), want, commitments)
    total = int(r.root_off[n])
    assert total == sum(2 * s.k for s in singles if not s.status)
    assert (r.rr[total:] == 0xC3).all() and (r.cr[total:] == 0xC3).all()  # the packed roots, no more
    first = next((i for i, s in enumerate(singles) if s.status), None)
    if first is None:
        assert (r.status, r.error) == (0, "")
    else:
        assert (r.status, r.error) == (singles[first].status, f"block {first}: {singles[first].error}")
    if commitments:
        assert r.n_commit == sum(len(s.commitments) for s in singles if not s.status)
        blocks = [int(b) for b in r.cb[:r.n_commit]]
        assert blocks == sorted(blocks)  # flat, in block order


def same_outputs(a, b):
    return (a.status == b.status and a.error == b.error and a.errors == b.errors and a.n_commit == b.n_commit and
            all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("k", "st", "inc", "rr", "cr", "root_off", "dah",
                                                                       "com", "cb", "ct")))


@pytest.fixture(scope="module")
def kinds(ctx):
    """layout_blocks() at max_square_size 128, greedy 0 and 1 (the dropping block, which needs 8,
    has a case of its own), with each block's single call. -> {greedy: ([name], [txs], [single])}"""
    out = {}
    for greedy in (0, 1):
        names, blocks, singles = [], [], []
        for name, txs, max_sq, _ in B.layout_blocks():
            if max_sq != 128:
                continue
            names.append(name)
            blocks.append(txs)
            singles.append(block_extend(ctx, txs, 128, greedy))
        out[greedy] = (names, blocks, singles)
    return out


def test_symbols_exported(ctx):
    import celestia_eds._lib as L
    for name in ("cel_dev_square_build_batch", "cel_block_extend_batch", "cel_block_batch_error"):
        assert name in L.EXPORTS and hasattr(ctx.lib, name)


# ---------------------------------------------------------------- 1. the kernel's bytes

@pytest.fixture(scope="module")
def kernel_blocks():
    """(k, raw bytes, segments, compact shares) of the mixed-width layouts."""
    out = []
    for i, n in enumerate((1, 477, 478)):  # k = 1: a one-share blob
        raw, segs = B.blob_layout([n], 1, 100 + i)
        out.append((1, raw, segs, np.zeros((0, 512), np.uint8)))
    raw, segs = B.blob_layout([478 + 482 + 1], 2, 110)  # k = 2: three shares and a pad
    assert [s.count for s in segs] == [3, 1]
    out.append((2, raw, segs, np.zeros((0, 512), np.uint8)))
    for txs, want_k in ((B.layout_blocks()[2][1], 4), (B.layout_blocks()[3][1], 16), (B.edge_block()[0], 32)):
        st, _, k, _, segs, compact = B.layout(txs)
        assert st == 0 and k == want_k
        out.append((k, b"".join(txs), segs, compact))
    assert all(s.kind != B.SEG_BLOB for s in out[4][2])  # k = 4: compact shares and padding only
    raw, segs = B.blob_layout(list(range(1, 1444)), 64, 120)
    out.append((64, raw, segs, np.zeros((0, 512), np.uint8)))
    return out


@pytest.mark.parametrize("order", [(0, 3, 1, 4, 2, 5, 6, 7), (7, 6, 5, 2, 4, 1, 3, 0)], ids=["rising", "falling"])
def test_kernel_bytes_mixed_widths(ctx, kernel_blocks, order):
    """Every block's Q0 is the layout's bytes and what cel_dev_square_build writes for it alone;
    every other byte of the buffer keeps its fill. k = 1 blocks sit beside the k = 2 block, so a
    wave's two shares lie in different blocks."""
    from hipmem import DeviceBuffer, synchronize
    blocks = [kernel_blocks[i] for i in order]
    n = len(blocks)
    tx_base, at = [], 0
    for b, (_, raw, _, _) in enumerate(blocks):  # block b's bytes start at an address that is b mod 4
        at += (b - at) % 4
        tx_base.append(at)
        at += len(raw)
    host = np.zeros(at + 8, np.uint8)
    for base, (_, raw, _, _) in zip(tx_base, blocks):
        host[base:base + len(raw)] = np.frombuffer(raw, np.uint8)
    d_txs = DeviceBuffer(len(host))
    d_txs.upload(host)
    eds_off, end = [], 0
    for b, (k, _, _, _) in enumerate(blocks):  # gaps of 16 bytes and more between the EDSs
        end += 16 * (1 + 37 * b)
        eds_off.append(end)
        end += 4 * k * k * 512
    end += 4096
    d_eds = DeviceBuffer(end, fill=0xA5)
    segs = [s for _, _, ss, _ in blocks for s in ss]
    arr = (B.Segment * len(segs))(*segs)
    compact = np.ascontiguousarray(np.concatenate([c for _, _, _, c in blocks]))
    u32 = lambda v: np.array(v, np.uint32)
    ctx.check(ctx.lib.cel_dev_square_build_batch(
        ctx.handle, d_txs.ptr, _p(np.array(tx_base, np.uint64)), n, arr, _p(u32([len(ss) for _, _, ss, _ in blocks])),
        _p(compact), _p(u32([len(c) for _, _, _, c in blocks])), _p(u32([k for k, _, _, _ in blocks])), d_eds.ptr,
        _p(np.array(eds_off, np.uint64)), None))
    synchronize()
    got = d_eds.download(end)
    rest = np.ones(end, bool)
    alone = DeviceBuffer(4 * 64 * 64 * 512)
    for (k, raw, ss, c), base, off in zip(blocks, tx_base, eds_off):
        eds = got[off:off + 4 * k * k * 512].reshape(2 * k, 2 * k, 512)
        want = B.expand(raw, k, ss, c)
        assert np.array_equal(eds[:k, :k].reshape(k * k, 512), want), f"k = {k}"
        a = (B.Segment * len(ss))(*ss)
        ctx.check(ctx.lib.cel_dev_square_build(ctx.handle, ctypes.c_void_p(d_txs.ptr.value + base), a, len(ss),
                                               _p(c) if len(c) else None, len(c), k, alone.ptr, None))
        synchronize()
        single = alone.download((2 * k, 2 * k, 512))
        assert np.array_equal(eds[:k, :k], single[:k, :k]), f"k = {k}"
        q0 = np.zeros((2 * k, 2 * k, 512), bool)
        q0[:k, :k] = True
        rest[off:off + 4 * k * k * 512] = ~q0.reshape(-1)
    assert (got[rest] == 0xA5).all(), "a byte outside every Q0 was written"


def test_device_entry_rejections(ctx, kernel_blocks):
    import celestia_eds._lib as L
    from hipmem import DeviceBuffer
    k, raw, ss, c = kernel_blocks[3]
    d = DeviceBuffer(4096 + 2 * 4 * k * k * 512)
    arr = (B.Segment * (2 * len(ss)))(*(ss + ss))
    u32 = lambda v: np.array(v, np.uint32)
    u64 = lambda v: np.array(v, np.uint64)

    def call(nseg, ks, offs, n=2):
        return ctx.lib.cel_dev_square_build_batch(ctx.handle, d.ptr, _p(u64([0, 0])), n, arr, _p(u32(nseg)), None,
                                                  _p(u32([0, 0])), _p(u32(ks)), d.ptr, _p(u64(offs)), None)
    assert call([2, 2], [k, k], [0, 8192]) == L.OK
    assert call([2, 2], [k, k], [0, 8192], n=0) == L.EINVAL
    assert call([2, 2], [k, k], [0, 8200]) == L.EINVAL  # an EDS offset that is no multiple of 16
    assert call([2, 1], [k, k], [0, 8192]) == L.EINVAL  # the second layout does not cover its square
    assert ctx.lib.cel_last_error(ctx.handle).decode().startswith("block 1: ")
    assert call([2, 2], [k, 3], [0, 8192]) == L.ENOTPOW2
    from hipmem import synchronize
    synchronize()


# ---------------------------------------------------------------- 2. the batch equals the loop

@pytest.mark.parametrize("greedy", [0, 1])
def test_batch_equals_loop(ctx, golden, kinds, greedy):
    import celestia_eds._lib as L
    names, blocks, singles = kinds[greedy]
    assert set(names) >= {"block408", "empty", "no_blobs", "no_normal", "ns_padding", "misordered"}
    r = batch_extend(ctx, blocks, 128, greedy)
    assert_batch(r, singles)
    assert block_of(r, names.index("block408")).dah.hex() == golden["block408"]["data_hash"].lower()
    mis = names.index("misordered")
    if greedy == 0:
        assert (r.status, r.error) == (L.EINVAL, f"block {mis}: {MISORDERED}")
        assert (int(r.st[mis]), r.errors[mis]) == (L.EINVAL, MISORDERED)
    else:
        assert r.status == 0 and (r.st[:len(blocks)] == 0).all()


@pytest.mark.parametrize("greedy", [0, 1])
def test_too_big_between_good_blocks(ctx, greedy):
    import celestia_eds._lib as L
    from square_inputs import random_block
    blocks = [random_block(3, 5, 0), B.dropping_block(), random_block(11, 2, 3, max_blob=2000)]
    singles = [block_extend(ctx, txs, 8, greedy) for txs in blocks]
    assert [s.status for s in singles] == ([0, L.ETOOBIG, 0] if greedy == 0 else [0, 0, 0])
    r = batch_extend(ctx, blocks, 8, greedy)
    assert_batch(r, singles)
    if greedy == 0:
        assert (r.status, r.error) == (L.ETOOBIG, "block 1: not enough space to append blob tx at index 12")


# ---------------------------------------------------------------- 3. order

def test_shuffled_order(ctx, kinds):
    names, blocks, singles = kinds[0]
    perm = np.random.default_rng(3).permutation(len(blocks))
    assert (perm != np.arange(len(blocks))).any()
    r = batch_extend(ctx, [blocks[i] for i in perm], 128, 0)
    assert_batch(r, [singles[i] for i in perm])


# ---------------------------------------------------------------- 4. chunks

def test_chunks(ctx, kinds):
    """A budget of 1 MiB: the k = 1, 4 and 16 blocks share a chunk, and each k = 32 block (2 MiB
    of EDS, above the budget) is a chunk of its own."""
    names, blocks, singles = kinds[0]
    ks = sorted(s.k for s in singles if not s.status)
    assert ks == [1, 4, 16, 32, 32]
    whole = batch_extend(ctx, blocks, 128, 0)
    cut = batch_extend(ctx, blocks, 128, 0, max_eds_bytes=1 << 20)
    assert_batch(cut, singles)
    assert same_outputs(cut, whole)
    one_each = batch_extend(ctx, blocks, 128, 0, max_eds_bytes=1)
    assert same_outputs(one_each, whole)


# ---------------------------------------------------------------- 5. threads

def test_host_threads(ctx, kinds):
    import celestia_eds._lib as L
    names, blocks, singles = kinds[0]
    mis = names.index("misordered")
    # failing blocks among good ones, so that with 4 and 16 threads workers lay failing blocks out
    order = [mis, 0, mis, 1, 2, mis, 3, 4, mis]
    bl, si = [blocks[i] for i in order], [singles[i] for i in order]
    base = batch_extend(ctx, bl, 128, 0, host_threads=1)
    assert_batch(base, si)
    for t in (4, 16):
        r = batch_extend(ctx, bl, 128, 0, host_threads=t)
        assert same_outputs(r, base)
        assert (r.status, r.error) == (L.EINVAL, f"block 0: {MISORDERED}")
        assert [r.errors[i] for i, o in enumerate(order) if o == mis] == [MISORDERED] * 4


# ---------------------------------------------------------------- 6. stale scratch

def test_stale_scratch(ctx, kinds):
    """ctx scratch is reused: fewer and smaller blocks after more and larger ones must not see
    their bytes."""
    import celestia_eds
    names, blocks, singles = kinds[0]
    pick = lambda ns: ([blocks[names.index(x)] for x in ns], [singles[names.index(x)] for x in ns])
    calls = [pick(["ns_padding", "block408", "no_normal", "no_blobs"]), pick(["no_blobs", "empty"])]
    fresh = []
    for bl, _ in calls:
        c = celestia_eds.Context(ctx.device)
        fresh.append(batch_extend(c, bl, 128, 0))
        c.close()
    c = celestia_eds.Context(ctx.device)
    for (bl, si), f in zip(calls, fresh):
        r = batch_extend(c, bl, 128, 0)
        assert same_outputs(r, f)
        assert_batch(r, si)
    c.close()


# ---------------------------------------------------------------- 7. edges

def test_edges(ctx, kinds):
    import celestia_eds._lib as L
    names, blocks, singles = kinds[0]
    i = names.index("ns_padding")
    assert_batch(batch_extend(ctx, [blocks[i]], 128, 0), [singles[i]])  # n = 1
    r = batch_extend(ctx, [], 128, 0)
    assert (r.status, r.error) == (L.EINVAL, "nil argument") and untouched(r)
    good = [b for b, s in zip(blocks, singles) if not s.status]
    need = sum(2 * s.k for s in singles if not s.status)
    ncom = sum(len(s.commitments) for s in singles if not s.status)
    assert ncom > 1
    r = batch_extend(ctx, good, 128, 0, roots_cap=need - 1)
    assert r.status == L.EINVAL and untouched(r)
    r = batch_extend(ctx, good, 128, 0, cap=ncom - 1)
    assert r.status == L.EINVAL and untouched(r) and r.n_commit == ncom
    assert batch_extend(ctx, good, 128, 0, roots_cap=need, cap=ncom).status == 0
    for kw, msg in ((dict(max_square_size=0), "max square size must be a power of 2"),
                    (dict(max_square_size=48), "max square size must be a power of 2"),
                    (dict(threshold=0), "subtree root threshold must be positive")):
        r = batch_extend(ctx, good, **{"max_square_size": 128, "roots_cap": 4096, **kw})
        assert (r.status, r.error) == (L.EINVAL, msg) and untouched(r)
        s = block_extend(ctx, good[0], kw.get("max_square_size", 128)) if "threshold" not in kw else None
        assert s is None or (s.status, s.error) == (r.status, r.error)
    r = batch_extend(ctx, good, 1024, roots_cap=4096)
    s = block_extend(ctx, good[0], 1024)
    assert (r.status, r.error) == (s.status, s.error) == (L.ETOOBIG, "square width 1024 exceeds the device path (512)")
    # commit_cap == 0 skips the commitments and still counts them
    r = batch_extend(ctx, good, 128, 0, cap=0)
    assert r.status == 0 and r.n_commit == ncom and (r.com == 0x55).all()
    assert_batch(r, [s for s in singles if not s.status], commitments=False)


# ---------------------------------------------------------------- 8. the GF(2^16) class

def test_gf16_class(ctx):
    blocks = [B.mib_block(), B.edge_block()[0]]
    singles = [block_extend(ctx, txs, 256) for txs in blocks]
    assert [s.k for s in singles] == [256, 32] and [s.status for s in singles] == [0, 0]
    assert_batch(batch_extend(ctx, blocks, 256), singles)


# ---------------------------------------------------------------- 9. the Python mirror

def test_python_mirror(ctx, golden, kinds):
    import celestia_eds._lib as L
    from celestia_eds import CelError, ExtendBlock, ExtendBlocks, ProcessProposal, ProcessProposals
    names, blocks, singles = kinds[0]
    good = [b for b, s in zip(blocks, singles) if not s.status]
    dahs = ExtendBlocks(ctx, good, host_threads=4)
    for txs, dah in zip(good, dahs):
        _, want = ExtendBlock(ctx, txs)
        assert dah.Hash() == want.Hash() and dah.RowRoots == want.RowRoots and dah.ColumnRoots == want.ColumnRoots
    with pytest.raises(CelError) as e:
        ExtendBlocks(ctx, blocks)
    mis = names.index("misordered")
    assert (e.value.status, str(e.value)) == (L.EINVAL, f"block {mis}: {MISORDERED}")
    hashes = [s.dah if not s.status else bytes(32) for s in singles]
    wrong = names.index("block408")
    hashes[wrong] = bytes([hashes[wrong][0] ^ 1]) + hashes[wrong][1:]  # a reject by the data hash
    got = ProcessProposals(ctx, blocks, hashes)
    assert got == [ProcessProposal(ctx, txs, h) for txs, h in zip(blocks, hashes)]
    assert not got[wrong][0] and len(got[wrong][1]) == 1
    assert got[mis] == (False, [])  # a reject by construction
    assert all(ok for i, (ok, _) in enumerate(got) if i not in (wrong, mis))
