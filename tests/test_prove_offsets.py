"""CPU: cel_prove_offsets (host only, no device): the prefix sums of each proof's leaf count and
of nmt ProveRange's node count, against cel_nmt_prove_range's count-only result (the recursion
of proof.cpp) for every range of 2k = 2, 4, 8, 16, 64 leaves and 500 seeded ranges of 1024; the
range errors, which name the proof, and n = 0."""
import ctypes

import numpy as np
import pytest


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _lib():
    import celestia_eds._lib as L
    return L, L.load()


def _offsets(lib, k, starts, ends):
    n = len(starts)
    starts, ends = np.asarray(starts, np.int32), np.asarray(ends, np.int32)
    leaf_off, node_off = np.full(n + 1, 77, np.uint64), np.full(n + 1, 77, np.uint64)
    st = lib.cel_prove_offsets(k, n, _p(starts), _p(ends), _p(leaf_off), _p(node_off))
    return st, leaf_off, node_off


def _want_counts(lib, w, starts, ends):
    dummy = np.zeros(90, np.uint8)  # count only: the tree is not read
    cnt = ctypes.c_uint32()
    out = []
    for s, e in zip(starts, ends):
        assert lib.cel_nmt_prove_range(_p(dummy), w, int(s), int(e), None, ctypes.byref(cnt)) == 0
        out.append(cnt.value)
    return out


def _ranges(w):
    if w <= 64:
        return [(s, e) for s in range(w) for e in range(s + 1, w + 1)]
    rng = np.random.default_rng(w)
    out = [(0, w), (0, 1), (w - 1, w), (w // 2 - 1, w // 2 + 1)]
    while len(out) < 500:
        s = int(rng.integers(0, w))
        out.append((s, int(rng.integers(s + 1, w + 1))))
    return out


@pytest.mark.parametrize("w", [2, 4, 8, 16, 64, 1024])
def test_offsets_match_prove_range(w):
    L, lib = _lib()
    starts, ends = zip(*_ranges(w))
    st, leaf_off, node_off = _offsets(lib, w // 2, starts, ends)
    assert st == L.OK, lib.cel_prove_last_error().decode()
    assert leaf_off[0] == 0 and node_off[0] == 0
    assert np.diff(leaf_off).tolist() == [e - s for s, e in zip(starts, ends)]
    assert np.diff(node_off).tolist() == _want_counts(lib, w, starts, ends)
    # the closed form itself, restated: popcount(s) + L - popcount(e - 1)
    lg = w.bit_length() - 1
    assert np.diff(node_off).tolist() == [bin(s).count("1") + lg - bin(e - 1).count("1") for s, e in zip(starts, ends)]


def test_offsets_errors_name_the_proof():
    L, lib = _lib()
    k, w = 8, 16
    good = [(0, 1), (3, 9), (0, w)]
    for bad in [(-1, 3), (5, 5), (6, 2), (0, w + 1), (w, w + 1), (-(2 ** 31), 1), (2 ** 31 - 1, -(2 ** 31))]:
        for at in (0, 2, 3):
            ranges = good[:at] + [bad] + good[at:]
            st, _, _ = _offsets(lib, k, *zip(*ranges))
            assert st == L.EINVAL, (bad, at)
            msg = lib.cel_prove_last_error().decode()
            assert msg.startswith(f"proof {at}: range [{bad[0]}, {bad[1]})"), msg
    st, _, _ = _offsets(lib, k, *zip(*good))
    assert st == L.OK and lib.cel_prove_last_error() == b""


def test_offsets_call_errors_and_empty_batch():
    L, lib = _lib()
    off = np.full(1, 77, np.uint64)
    assert lib.cel_prove_offsets(8, 0, None, None, _p(off), _p(off)) == L.OK and off[0] == 0
    one = np.zeros(1, np.int32)
    two = np.zeros(2, np.uint64)
    assert lib.cel_prove_offsets(8, 1, None, _p(one), _p(two), _p(two)) == L.EINVAL
    assert lib.cel_prove_offsets(8, 1, _p(one), _p(one), None, _p(two)) == L.EINVAL
    assert lib.cel_prove_offsets(8, 1, _p(one), _p(one), _p(two), None) == L.EINVAL
    for k in (0, 3, 4096):
        assert lib.cel_prove_offsets(k, 0, None, None, _p(off), _p(off)) == L.EINVAL
