"""GPU: blob share commitments from blob bytes (cel_create_commitments,
cel_dev_create_commitments, cel_blob_tx_commitments; go-square inclusion.CreateCommitment),
bit-exact against the hashlib restatement in commitment_ref.py, the signed commitment of
block 408's blob tx, and the library's other device path (GetCommitment over an EDS)."""
import ctypes

import numpy as np
import pytest

import commitment_ref as ref
from square_inputs import block408_txs, random_block

pytestmark = pytest.mark.gpu

# every share count at which the layout changes shape: one share, the first / second share
# boundary, widths 1, 2, 8 and 32 with one-, two- and three-piece tails, a whole power of two
MIXED_SHARES = [63, 64, 65, 267, 352, 1031, 16384]
MIXED_LENGTHS = [1, 478, 479, 960, 961] + [ref.blob_len_for_shares(n) for n in MIXED_SHARES]


_ns, _data = ref.random_namespace, ref.random_bytes


def test_block408_signed_commitment(ctx):
    """The only vector the reference data holds (SHA-256 paths only, no GF arithmetic):
    the commitment signed in block 408's MsgPayForBlobs."""
    from celestia_eds import inclusion
    txs = block408_txs()
    got = inclusion.BlobTxCommitments(txs, ctx=ctx)
    assert len(got) == 1
    tx_index, commitment = got[0]
    blobs, signed = ref.blob_tx_parts(txs[tx_index])
    assert len(blobs) == 1 and commitment == signed[0]


@pytest.fixture(scope="module")
def mixed_blobs():
    rng = np.random.default_rng(408)
    # packed back to back, so the data offsets take every value mod 4 (checked below); the
    # last blob's last share is short of full
    blobs = [(_ns(rng), _data(rng, n)) for n in MIXED_LENGTHS[:-1]] + \
            [(_ns(rng), _data(rng, MIXED_LENGTHS[-1] - 100))]
    blobs[8] = (bytes(28) + b"\x07", blobs[8][1])   # 267 shares, all zeros but the last byte
    blobs[6] = (b"\xff" * 29, blobs[6][1])          # 64 shares in the parity namespace
    offsets = np.cumsum([0] + [len(d) for _, d in blobs])
    assert {int(o) % 4 for o in offsets[:-1]} == {0, 1, 2, 3}
    return blobs


@pytest.mark.parametrize("threshold", [64, 8])
def test_mixed_batch(ctx, mixed_blobs, threshold):
    from celestia_eds import inclusion
    got = inclusion.CreateCommitments(mixed_blobs, threshold, ctx=ctx)
    for i, (ns, data) in enumerate(mixed_blobs):
        assert got[i] == ref.create_commitment(ns, data, 0, threshold), (i, len(data), threshold)


def test_wide_subtrees(ctx):
    """70000 shares at threshold 64: width 512 (two tiles per subtree) and the tail
    256, 64, 32, 16."""
    from celestia_eds import inclusion
    rng = np.random.default_rng(70000)
    ns, data = _ns(rng), _data(rng, ref.blob_len_for_shares(70000) - 7)
    assert inclusion.blob_subtree_sizes(len(data), 64)[1] == 512
    assert inclusion.CreateCommitment(ns, data, ctx=ctx) == ref.create_commitment(ns, data)


def test_many_roots(ctx):
    """3000 shares at threshold 4096: width 1, so 3000 roots (more than one workgroup's
    LDS holds) and no NMT inner node."""
    from celestia_eds import inclusion
    rng = np.random.default_rng(3000)
    ns, data = _ns(rng), _data(rng, ref.blob_len_for_shares(3000) - 481)
    assert inclusion.blob_subtree_sizes(len(data), 4096) == (3000, 1, [1] * 3000)
    assert inclusion.CreateCommitment(ns, data, threshold=4096, ctx=ctx) == \
        ref.create_commitment(ns, data, 0, 4096)


def test_batch_consistency_and_device_entry(ctx):
    from celestia_eds import inclusion
    from hipmem import DeviceBuffer, synchronize
    rng = np.random.default_rng(300)
    blobs = [(_ns(rng), _data(rng, int(rng.integers(1, 6001)))) for _ in range(300)]
    batch = inclusion.CreateCommitments(blobs, ctx=ctx)
    for i in rng.choice(300, 20, replace=False):
        ns, data = blobs[i]
        assert inclusion.CreateCommitment(ns, data, ctx=ctx) == batch[i]
        assert batch[i] == ref.create_commitment(ns, data)
    # the same batch from device-resident bytes
    lib = ctx.lib
    data, offsets, ns, _ = inclusion._pack_blobs(blobs)
    shares = sum(ref.sparse_shares_needed(len(d)) for _, d in blobs)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d_data = DeviceBuffer(len(data))
    d_data.upload(data)
    d_out = DeviceBuffer(32 * len(blobs))
    d_work = DeviceBuffer(lib.cel_dev_commitments_workspace_size(shares, len(blobs)))
    ctx.check(lib.cel_dev_create_commitments(ctx.handle, d_data.ptr, P(offsets), len(blobs), P(ns), None, 64,
                                             d_out.ptr, d_work.ptr, None))
    synchronize()  # the call is asynchronous on the context's stream
    out = d_out.download((len(blobs), 32))
    assert [out[i].tobytes() for i in range(len(blobs))] == batch


def test_agrees_with_get_commitment(ctx):
    """Every blob of a constructed square: the commitment from its bytes equals the one
    GetCommitment reads from the extended square's row trees."""
    from celestia_eds import da, inclusion, square
    txs = random_block(21, 4, 25, max_blob=70000)
    got = inclusion.BlobTxCommitments(txs, ctx=ctx)
    ods = square.Construct(txs)
    eds = da.ExtendShares(list(ods))
    # where each blob starts in the square: its first share carries the sequence-start bit,
    # the blob's namespace and its length (namespace padding shares carry length 0)
    starts = {}
    for i, s in enumerate(ods):
        length = int.from_bytes(bytes(s[ref.NS + 1:ref.NS + 5]), "big")
        if s[ref.NS] & 1 and length > 0:
            starts.setdefault((bytes(s[:ref.NS]), length), []).append(i)
    # every blob in tx, then blob, order, as BlobTxCommitments reports them
    want = [(t, ns, data) for t, tx in enumerate(txs) if t >= 4 for ns, data, _ in ref.blob_tx_blobs(tx)]
    assert len(want) >= 25 and len(got) == len(want)
    for (tx_index, commitment), (t, ns, data) in zip(got, want):
        assert tx_index == t
        start = starts[(ns, len(data))].pop(0)
        assert commitment == inclusion.GetCommitment(eds, start, ref.sparse_shares_needed(len(data))), (t, start)


def test_errors(ctx):
    from celestia_eds import CelError, inclusion
    import celestia_eds._lib as L
    ns = bytes(28) + b"\x09"
    with pytest.raises(CelError, match="blob 1 has no data") as e:
        inclusion.CreateCommitments([(ns, b"abc"), (ns, b"")], ctx=ctx)
    assert e.value.status == L.EINVAL
    with pytest.raises(CelError, match="unsupported share version 1") as e:
        inclusion.CreateCommitment(ns, b"abc", share_version=1, ctx=ctx)
    assert e.value.status == L.EINVAL
    with pytest.raises(CelError, match="subtree root threshold must be positive") as e:
        inclusion.CreateCommitment(ns, b"abc", threshold=0, ctx=ctx)
    assert e.value.status == L.EINVAL
    out = (ctypes.c_uint8 * 64)()
    data = (ctypes.c_uint8 * 16)()
    off = (ctypes.c_uint64 * 3)(0, 10, 4)
    nss = (ctypes.c_uint8 * 58)()
    assert ctx.lib.cel_create_commitments(ctx.handle, data, off, 2, nss, None, 64, out) == L.EINVAL
    assert ctx.lib.cel_last_error(ctx.handle).decode() == "blob offsets must be non-decreasing"
