"""GPU: the blob commitment kernels (blob_commit.hip) and their host entry (api_commit.cpp)
at the lengths, alignments, root counts, subtree widths and batch sizes where their code
branches, bit for bit against the hashlib restatement in commitment_ref.py:

  every blob length 1..1443 at every byte alignment (blob_leaf_node's clamp and masks);
  the whole-wave fast path against the masked path, block by block;
  RFC-6962 root counts on both sides of the 64 / 256-lane block switch, of the LDS capacity
    (1024 digests) and with odd global-memory levels (k_blob_commit);
  subtree widths 256 and 1024 (k_blob_tile's own level-8 root, k_blob_top_level at L = 10);
  a host batch of three device chunks, from pageable and from page-locked memory (run_host);
  random batches in which blobs of unlike widths share a tile, at thresholds 1, 5, 64, 1000;
  the leaf stage's A/B partner (CEL_COMMIT_LEAF=expanded: k_blob_expand, k_blob_tile<true>).
"""
import ctypes

import numpy as np
import pytest

import commitment_ref as ref

pytestmark = pytest.mark.gpu

WIDE = 1 << 20  # a threshold at which every blob here has subtree width 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Batch:
    """Blobs packed back to back: .blobs [(ns, data)], .data (uint8), .offsets (uint64),
    .ns (uint8), .shares."""

    def __init__(self, blobs):
        from celestia_eds import inclusion
        self.blobs = blobs
        self.data, self.offsets, self.ns, _ = inclusion._pack_blobs(blobs)
        self.shares = sum(ref.sparse_shares_needed(len(d)) for _, d in blobs)
        self._want = {}

    def want(self, threshold=64):
        if threshold not in self._want:
            self._want[threshold] = [ref.create_commitment(ns, d, 0, threshold) for ns, d in self.blobs]
        return self._want[threshold]


def from_lengths(seed, lengths):
    """One random blob per length, cut out of a single random buffer."""
    rng = np.random.default_rng(seed)
    raw = rng.bytes(int(sum(lengths)))
    blobs, at = [], 0
    for n in lengths:
        blobs.append((ref.random_namespace(rng), raw[at:at + n]))
        at += n
    return blobs


def dev_commitments(ctx, batch, odd=0, threshold=64):
    """cel_dev_create_commitments with the batch's bytes `odd` bytes into a device buffer that
    is 0xA5 before them and 0xA5 straight after the last blob's last byte."""
    from hipmem import DeviceBuffer, hip, synchronize
    lib, n = ctx.lib, len(batch.blobs)
    d_data = DeviceBuffer(odd + len(batch.data) + 8, fill=0xA5)
    assert d_data.ptr.value % 4 == 0
    assert hip().hipMemcpy(ctypes.c_void_p(d_data.ptr.value + odd), _p(batch.data), len(batch.data), 1) == 0
    d_out = DeviceBuffer(32 * n, fill=0)
    d_work = DeviceBuffer(lib.cel_dev_commitments_workspace_size(batch.shares, n))
    ctx.check(lib.cel_dev_create_commitments(ctx.handle, ctypes.c_void_p(d_data.ptr.value + odd), _p(batch.offsets), n,
                                             _p(batch.ns), None, threshold, d_out.ptr, d_work.ptr, None))
    synchronize()  # the call is asynchronous on the context's stream
    out = d_out.download((n, 32))
    guard = d_data.download_at(odd + len(batch.data), (8,))
    assert (guard == 0xA5).all()
    for b in (d_data, d_out, d_work):
        b.free()
    return [out[i].tobytes() for i in range(n)]


def host_commitments(ctx, batch, threshold=64, data_ptr=None):
    """cel_create_commitments through the raw ABI; data_ptr: the batch's bytes elsewhere."""
    n = len(batch.blobs)
    out = np.zeros((n, 32), np.uint8)
    ctx.check(ctx.lib.cel_create_commitments(ctx.handle, data_ptr if data_ptr is not None else _p(batch.data),
                                             _p(batch.offsets), n, _p(batch.ns), None, threshold, _p(out)))
    return [out[i].tobytes() for i in range(n)]


def assert_equal(got, batch, threshold=64):
    want = batch.want(threshold)
    bad = [(i, len(batch.blobs[i][1])) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {len(want)} commitments differ, (blob, length): {bad[:12]}"


# --- 1. every length at every alignment ---------------------------------------------------

ALL_LENGTHS = list(range(1, 1444))  # one to four shares; every tail length of a 2nd and a 3rd share


@pytest.fixture(scope="module")
def every_length():
    blobs = from_lengths(1443, ALL_LENGTHS)
    blobs[700] = (ref.PARITY_NS, blobs[700][1])
    blobs[1200] = (bytes(28) + b"\x07", blobs[1200][1])
    b = Batch(blobs)
    assert b.shares == 2892
    # every tail length 1..482 of a second and of a third share, 1..478 of a first
    tails = {(ref.sparse_shares_needed(n), n - ref.blob_len_for_shares(ref.sparse_shares_needed(n) - 1))
             for n in ALL_LENGTHS if n > ref.FIRST}
    assert {t for s, t in tails if s == 2} == {t for s, t in tails if s == 3} == set(range(1, 483))
    # over the four shifts every length starts at every address mod 4
    for o in b.offsets[:-1]:
        assert {(int(o) + odd) % 4 for odd in range(4)} == {0, 1, 2, 3}
    return b


@pytest.mark.parametrize("odd", [0, 1, 2, 3])
def test_every_length_device_entry(ctx, every_length, odd):
    assert_equal(dev_commitments(ctx, every_length, odd), every_length)


def test_every_length_host_entry(ctx, every_length):
    assert_equal(host_commitments(ctx, every_length), every_length)


# --- 2. the whole-wave fast path and the masked path ----------------------------------------

# bytes in the last of 130 shares: block b of the leaf message takes plain loads iff
# 64 b + 8 <= those bytes, for every lane of the wave
LEFT = [1, 481, 482] + [64 * b + d for b in range(1, 8) for d in (7, 8, 9)]


@pytest.fixture(scope="module")
def tails_130():
    b = Batch(from_lengths(130, [ref.blob_len_for_shares(129) + left for left in LEFT]))
    assert all(ref.sparse_shares_needed(len(d)) == 130 for _, d in b.blobs)
    return b


@pytest.mark.parametrize("odd", [0, 1, 2, 3])
def test_fast_and_masked_path(ctx, tails_130, odd):
    """Each blob's short last share is one lane among the full shares of its neighbours."""
    assert_equal(dev_commitments(ctx, tails_130, odd), tails_130)


# --- 3. root counts at width 1 --------------------------------------------------------------

ROOTS_64_LANES = [1, 2, 3, 5, 7, 127, 128]
ROOTS_256_LANES = [129, 1023, 1024, 1025, 2049, 2051, 3000]


def _width1_batch(seed, counts):
    from celestia_eds import inclusion
    rng = np.random.default_rng(seed)
    lengths = [ref.blob_len_for_shares(n) - int(rng.integers(0, 482 if n > 1 else 478)) for n in counts]
    for n, length in zip(counts, lengths):
        assert inclusion.blob_subtree_sizes(length, WIDE) == (n, 1, [1] * n)
    return Batch(from_lengths(seed, lengths))


def test_root_counts_64_lane_block(ctx):
    """max_roots = 128: the last count that takes k_blob_commit's 64-lane block."""
    b = _width1_batch(128, ROOTS_64_LANES)
    assert_equal(host_commitments(ctx, b, WIDE), b, WIDE)


def test_root_counts_256_lane_block(ctx):
    """129 roots take the 256-lane block; 1024 is exactly the LDS capacity; 1025, 2049 and
    2051 reduce in global memory over levels of odd size, where the unpaired node moves up,
    with two such blobs side by side in the scratch."""
    assert ref.rfc_level_sizes(1024) == [1024]
    assert ref.rfc_level_sizes(1025) == [1025, 513]
    assert ref.rfc_level_sizes(2049) == [2049, 1025, 513]
    assert ref.rfc_level_sizes(2051) == [2051, 1026, 513]
    assert ref.rfc_level_sizes(3000) == [3000, 1500, 750]
    b = _width1_batch(129, ROOTS_256_LANES)
    assert_equal(host_commitments(ctx, b, WIDE), b, WIDE)


# --- 4. widths 256 and 1024, several chunks, page-locked input ------------------------------

@pytest.fixture(scope="module")
def chunked():
    """[1000 B], [264001 shares less 7 bytes = 121 MiB], [5000 B, 3 MiB, 20037 shares]: three
    device chunks of the host entry (64 MiB each at most, whole blobs). The reference is
    computed once for both runs."""
    from celestia_eds import inclusion
    lengths = [1000, ref.blob_len_for_shares(264001) - 7, 5000, 3 << 20, ref.blob_len_for_shares(20037) - 3]
    assert inclusion.blob_subtree_sizes(lengths[1], 64) == (264001, 1024, [1024] * 257 + [512, 256, 64, 1])
    assert inclusion.blob_subtree_sizes(lengths[4], 64) == (20037, 256, [256] * 78 + [64, 4, 1])
    chunk = 64 << 20
    assert lengths[0] + lengths[1] > chunk and lengths[1] > chunk and sum(lengths[2:]) <= chunk
    b = Batch(from_lengths(264001, lengths))
    b.want(64)
    return b


def test_chunks_and_wide_subtrees(ctx, chunked):
    """Pageable memory: every chunk goes through the page-locked staging buffer, which the
    second chunk regrows and the third reuses; results land at blob index * 32."""
    assert_equal(host_commitments(ctx, chunked), chunked)


def test_chunks_from_page_locked_memory(ctx, chunked):
    """cel_host_alloc memory: each chunk is uploaded straight from the caller's bytes."""
    n = len(chunked.data)
    p = ctx.lib.cel_host_alloc(n)
    assert p, "cel_host_alloc failed"
    try:
        ctypes.memmove(p, _p(chunked.data), n)
        assert_equal(host_commitments(ctx, chunked, data_ptr=ctypes.c_void_p(p)), chunked)
    finally:
        ctx.lib.cel_host_free(p)


# --- 5. mixed random batches ----------------------------------------------------------------

MIXED_SEED = 0  # the first seed at which the widths at threshold 1 are every power of two up to 256


def mixed_lengths(seed=MIXED_SEED):
    """About 120 blobs with share counts log-uniform in 1..3000, three of 5000..20000 shares
    (one above 16384), each one's last share cut at a random byte, in random order."""
    rng = np.random.default_rng(seed)
    counts = [int(np.exp(rng.uniform(0, np.log(3001)))) for _ in range(120)]
    counts += [int(rng.integers(5000, 16385)), int(rng.integers(5000, 16385)), int(rng.integers(16385, 20001))]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    return [ref.blob_len_for_shares(n) - int(rng.integers(0, 478)) for n in counts]


@pytest.fixture(scope="module")
def mixed():
    return Batch(from_lengths(MIXED_SEED, mixed_lengths()))


@pytest.mark.parametrize("threshold", [1, 5, 64, 1000])
def test_mixed_batch(ctx, mixed, threshold):
    """Blobs of unlike widths and the alignment gaps between them in the same 256-slot tile
    (k_blob_tile's meta and top_level), at thresholds that are no power of two as well."""
    from celestia_eds import inclusion
    widths = {inclusion.blob_subtree_sizes(len(d), threshold)[1] for _, d in mixed.blobs}
    if threshold == 1:
        assert widths == {1 << i for i in range(9)}
    assert_equal(host_commitments(ctx, mixed, threshold), mixed, threshold)


# --- 6. the expanded leaf stage -------------------------------------------------------------

def test_expanded_leaf_stage(ctx, every_length, mixed, monkeypatch):
    """k_blob_expand + k_blob_tile<true>: an independent, byte-by-byte cut of the same shares.
    The library reads the variable on every call."""
    monkeypatch.setenv("CEL_COMMIT_LEAF", "expanded")
    assert_equal(dev_commitments(ctx, every_length, 1), every_length)
    assert_equal(host_commitments(ctx, mixed, 64), mixed, 64)
