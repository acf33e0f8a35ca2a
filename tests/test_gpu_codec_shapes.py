"""GPU parity of the rsmt2d.Codec surface away from the product shape (512-byte shares):
every encode and decode kernel at shard lengths and counts that reach its tail, stride and
multi-workgroup paths, bit for bit against the oracle. "n" is the number of data shards.

encode  k_rs_encode_bs     n <= 16        32-byte granules, 64 per workgroup
        k_rs_axis_gf8      n = 32..128    256-byte slices, 4 per workgroup, xcd_block remap
        k_rs_gf16x         n = 256, 512   64-byte blocks, 4 per workgroup, xcd_block remap
        k_rs_encode_gf16p  n = 1024, 2048 LDS, chunk loop over min(len / 64, 512) workgroups
decode  k_rs_decode        n <= 8         LDS, 2 chunks per workgroup, stride loop
        k_rs_decode_axis   n = 16..128    128-byte slices, 4 per workgroup, blockIdx.y beyond
        k_rs_decode_gf16   n = 256..1024  LDS, chunk sets
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERNS = ("one", "n_random", "all_data", "all_parity")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _encode(ctx, data):
    from celestia_eds import _lib
    n, ln = data.shape
    par = np.zeros_like(data)
    st = ctx.lib.cel_codec_encode(ctx.handle, _p(np.ascontiguousarray(data)), n, ln, _p(par))
    assert st == _lib.OK, (n, ln, st)
    return par


# bit-slice: 2112 B = 66 granules, a full workgroup and a partial second one.
# axis: 64 / 320 / 704 end in partial slices of 64 / 64 / 192 bytes; 8448 = 33 slices = 9
#   workgroups; 9408 = 36.75 slices = 37 tiles = 10 workgroups with a 192-byte last slice
#   (grids above 8 that are no multiple of 8: the q > 0 && r > 0 branch of xcd_block).
# gf16x: 1 and 3 live waves of 4, and grids of 9, 10 and 14 workgroups.
# gf16p: more than one chunk; 32832 B = 513 chunks, so workgroup y = 0 of 512 runs the chunk
#   loop twice (LDS reuse behind the top-of-loop barrier). 32 MiB in, 32 MiB out.
ENCODE_SHAPES = ([(n, ln) for n in (2, 16) for ln in (64, 2112)] +
                 [(n, ln) for n in (32, 64, 128) for ln in (64, 320, 704, 8448, 9408)] +
                 [(n, 64 * b) for n in (256, 512) for b in (1, 3, 33, 37, 53)] +
                 [(n, ln) for n in (1024, 2048) for ln in (192, 512)] +
                 [(1024, 32832)])


@pytest.mark.parametrize("n,ln", ENCODE_SHAPES)
def test_encode_shapes(ctx, oracle, n, ln):
    rng = np.random.default_rng(n * 100003 + ln)
    data = rng.integers(0, 256, (n, ln), dtype=np.uint8)
    assert np.array_equal(_encode(ctx, data), oracle.rs_encode(data))


def _present(rng, n, pattern):
    """Presence of the 2n shards (data, then parity); every pattern leaves >= n present."""
    present = np.ones(2 * n, np.uint8)
    if pattern == "one":
        present[rng.integers(0, 2 * n)] = 0
    elif pattern == "n_random":
        present[rng.choice(2 * n, n, replace=False)] = 0
    elif pattern == "all_data":
        present[:n] = 0
    elif pattern == "all_parity":
        present[n:] = 0
    else:  # a random count in between
        present[rng.choice(2 * n, int(rng.integers(1, n + 1)), replace=False)] = 0
    return present


def _codeword(oracle, rng, n, ln):
    data = rng.integers(0, 256, (n, ln), dtype=np.uint8)
    return np.concatenate([data, oracle.rs_encode(data)])


def _damage(rng, cw, present):
    """The caller's buffer: erased shards hold random bytes, not zeros."""
    return np.where(present[..., None] == 1, cw, rng.integers(0, 256, cw.shape, dtype=np.uint8)).astype(np.uint8)


# LDS decoder: 192 B = 3 chunks, 2 per workgroup: gridDim.y = 2 with uneven work.
# register decoder: 576 B = 4.5 slices, a second y-block with one half-filled wave; 1088 B =
#   8.5 slices, three y-blocks.
# GF(2^16) decoder: 3 chunks, an odd count.
DECODE_SHAPES = ([(n, ln) for n in (2, 4, 8) for ln in (64, 192)] +
                 [(n, ln) for n in (16, 32, 128) for ln in (576, 1088)] +
                 [(n, 192) for n in (256, 512, 1024)])


@pytest.mark.parametrize("n,ln", DECODE_SHAPES)
def test_codec_decode_shapes(ctx, oracle, n, ln):
    """cel_codec_decode returns the whole codeword: erased shards recovered, present ones
    untouched. The oracle's own decode of the same damaged buffer gives the codeword too,
    so it is the reference of every case."""
    from celestia_eds import _lib
    rng = np.random.default_rng(n * 200003 + ln)
    cw = _codeword(oracle, rng, n, ln)
    for pattern in PATTERNS:
        present = _present(rng, n, pattern)
        buf = _damage(rng, cw, present)
        assert np.array_equal(oracle.rs_decode(buf, present), cw), (n, ln, pattern)
        st = ctx.lib.cel_codec_decode(ctx.handle, _p(buf), _p(present), n, ln)
        assert st == _lib.OK, (n, ln, pattern, st)
        assert np.array_equal(buf, cw), (n, ln, pattern)


@pytest.mark.parametrize("n,ln", [(4, 192)] + [(n, ln) for n in (16, 32, 128) for ln in (576, 1088)] + [(256, 192)])
def test_dev_decode_shapes(ctx, oracle, n, ln):
    """cel_dev_decode over 5 dense axes, one erasure pattern each (the four of PATTERNS and
    a random count), in a device buffer that ends in a 4 KiB guard of 0xA5: every axis
    comes back as its codeword, the guard and the presence bytes stay as they were."""
    from hipmem import DeviceBuffer, synchronize
    from celestia_eds import _lib
    rng = np.random.default_rng(n * 300007 + ln)
    naxes = 5
    cw = np.stack([_codeword(oracle, rng, n, ln) for _ in range(naxes)])
    pres = np.stack([_present(rng, n, (PATTERNS + ("some",))[a]) for a in range(naxes)])
    buf = _damage(rng, cw, pres)
    for a in range(naxes):
        assert np.array_equal(oracle.rs_decode(buf[a], pres[a]), cw[a]), (n, ln, a)
    guard = np.full(GUARD, 0xA5, np.uint8)
    d, dp = DeviceBuffer(buf.nbytes + GUARD), DeviceBuffer(pres.nbytes + GUARD)
    d.upload(np.concatenate([buf.reshape(-1), guard]))
    dp.upload(np.concatenate([pres.reshape(-1), guard]))
    assert ctx.lib.cel_dev_decode(ctx.handle, d.ptr, dp.ptr, naxes, n, ln, None) == _lib.OK
    synchronize()
    out = d.download(buf.nbytes + GUARD)
    pout = dp.download(pres.nbytes + GUARD)
    for a in range(naxes):
        assert np.array_equal(out[:buf.nbytes].reshape(buf.shape)[a], cw[a]), (n, ln, a)
    assert np.array_equal(out[buf.nbytes:], guard), "shard guard overwritten"
    assert np.array_equal(pout[:pres.nbytes].reshape(pres.shape), pres) and np.array_equal(pout[pres.nbytes:], guard)
