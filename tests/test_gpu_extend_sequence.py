"""GPU: every extension entry point in a row on one fresh ctx, twice, with nothing between the
calls. The entry points share the ctx's events, streams, scratch and page-locked staging, so what
one call leaves recorded or staged meets the next one's waits. All at k = 32, the smallest width
that takes the one-square path and has a repair:

  1. one square, page-locked ODS, full EDS into page-locked memory (direct read, early top download)
  2. the same, parity only, into pageable memory
  3. cel_extend_batch, n = 5, pageable ODSs, parity-only EDSs into pageable memory (chunks of 2, 2, 1)
  4. cel_dev_extend_batch, n = 3 (the two pipeline halves), left running
  5. cel_block_extend on the smallest block of block_inputs, with eds_out
  6. cel_repair of the round's EDS with a quarter withheld
  7. the one-square call again, header only

Every output equals the oracle's (bytes and roots), the second round equals the first, and at the
end a push-order violation across rows k/2 - 1 / k/2 still comes back as CEL_EORDER with the
reference's message."""
import ctypes

import numpy as np
import pytest

import block_inputs as B
from eds_inputs import random_ods
from hipmem import DeviceBuffer, synchronize

pytestmark = pytest.mark.gpu

K, W = 32, 64
N_HOST, N_DEV = 5, 3


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pinned(c, shape):
    nbytes = int(np.prod(shape))
    p = c.lib.cel_host_alloc(nbytes)
    assert p, "cel_host_alloc failed"
    return p, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p)).reshape(shape)


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle's EDS, roots and DAH of every square of a round, computed once."""
    one = random_ods(K, 4100)
    host = np.stack([random_ods(K, 4200 + i) for i in range(N_HOST)])
    dev = np.stack([random_ods(K, 4300 + i) for i in range(N_DEV)])
    name, txs, max_sq, kb = B.layout_blocks()[1]
    assert name == "empty" and kb == 1
    st, _, k, _, shares = B.construct(txs, max_sq, 64, 0)
    assert st == 0 and k == 1
    return {"one": (one, oracle.extend_and_commit(one)),
            "host": (host, [oracle.extend_and_commit(o) for o in host]),
            "dev": (dev, [oracle.extend_and_commit(o) for o in dev]),
            "block": (txs, max_sq, oracle.extend_and_commit(np.asarray(shares, np.uint8).reshape(1, 1, 512)))}


def _round(c, want, bufs):
    """The seven calls back to back; every output copied out after the last one."""
    from celestia_eds import _lib
    from celestia_eds.rsmt2d import ExtendedDataSquare
    l, h = c.lib, c.handle
    p_ods, p_eds, eds_pin = bufs["p_ods"], bufs["p_eds"], bufs["eds_pin"]
    out = {}

    def roots(n=1):
        return (np.zeros((n, W, 90), np.uint8), np.zeros((n, W, 90), np.uint8), np.zeros((n, 32), np.uint8),
                np.full(n, 0x7F, np.int32))

    # 1. page-locked in, full EDS into page-locked memory
    eds_pin[...] = 0
    r1 = roots()
    c.check(l.cel_extend_batch(h, ctypes.c_void_p(p_ods), 1, K, 512, ctypes.c_void_p(p_eds), _p(r1[0]), _p(r1[1]),
                               _p(r1[2]), _p(r1[3]), _lib.FLAG_ORDER_CHECK))
    # 2. parity only into pageable memory
    eds2 = np.full((W, W, 512), 0x5A, np.uint8)
    r2 = roots()
    c.check(l.cel_extend_batch(h, ctypes.c_void_p(p_ods), 1, K, 512, _p(eds2), _p(r2[0]), _p(r2[1]), _p(r2[2]),
                               _p(r2[3]), _lib.FLAG_ORDER_CHECK | _lib.FLAG_PARITY_ONLY))
    # 3. five squares, pageable, parity only
    eds3 = np.full((N_HOST, W, W, 512), 0x5A, np.uint8)
    r3 = roots(N_HOST)
    c.check(l.cel_extend_batch(h, _p(want["host"][0]), N_HOST, K, 512, _p(eds3), _p(r3[0]), _p(r3[1]), _p(r3[2]),
                               _p(r3[3]), _lib.FLAG_ORDER_CHECK | _lib.FLAG_PARITY_ONLY))
    # 4. three resident squares, asynchronous on the ctx's stream
    d = bufs["dev"]
    c.check(l.cel_dev_extend_batch(h, d["ods"].ptr, N_DEV, K, d["eds"].ptr, d["rr"].ptr, d["cr"].ptr, d["dah"].ptr,
                                   d["st"].ptr, d["work"].ptr, None, _lib.FLAG_ORDER_CHECK))
    # 5. the block path with its EDS
    txs, max_sq, _ = want["block"]
    buf, lens, ntx, _ = B.pack(txs)
    kb, nc = ctypes.c_uint32(), ctypes.c_uint32()
    inc = (ctypes.c_uint8 * max(ntx, 1))()
    rb = (np.full((2 * max_sq, 90), 0xC3, np.uint8), np.full((2 * max_sq, 90), 0xC3, np.uint8), np.zeros(32, np.uint8))
    eds5 = np.full((2, 2, 512), 0x5A, np.uint8)
    c.check(l.cel_block_extend(h, buf, lens, ntx, max_sq, 64, 0, ctypes.byref(kb), inc, _p(rb[0]), _p(rb[1]), _p(rb[2]),
                               _p(eds5), eds5.nbytes, None, None, 0, ctypes.byref(nc), _lib.FLAG_ORDER_CHECK))
    # 6. the repair of call 1's EDS with Q0 withheld
    present = np.ones((W, W), np.uint8)
    present[:K, :K] = 0
    damaged = eds_pin.copy()
    damaged[present == 0] = 0
    sq = ExtendedDataSquare(damaged, ctx=c)
    sq.Repair([x.tobytes() for x in r1[0][0]], [x.tobytes() for x in r1[1][0]], present=present)
    # 7. header only
    r7 = roots()
    c.check(l.cel_extend_batch(h, ctypes.c_void_p(p_ods), 1, K, 512, None, _p(r7[0]), _p(r7[1]), _p(r7[2]), _p(r7[3]),
                               _lib.FLAG_ORDER_CHECK))
    synchronize()
    out["one"] = (eds_pin.copy(),) + r1
    out["parity"] = (eds2,) + r2
    out["host"] = (eds3,) + r3
    out["dev"] = (d["eds"].download((N_DEV, W, W, 512)), d["rr"].download((N_DEV, W, 90)),
                  d["cr"].download((N_DEV, W, 90)), d["dah"].download((N_DEV, 32)), d["st"].download((N_DEV,), np.int32))
    out["block"] = (eds5, rb[0], rb[1], rb[2], kb.value)
    out["repair"] = np.array(sq.cells, np.uint8).reshape(W, W, 512)
    out["header"] = r7
    return out


def _check_square(got_eds, got, ref, parity_only=False, ods=None):
    """got = (row roots, col roots, dah, status) of one square against the oracle's tuple."""
    e, rr, cr, dah = ref
    assert np.array_equal(got[0], rr) and np.array_equal(got[1], cr), "roots differ"
    assert got[2].tobytes() == dah and got[3] == 0
    if got_eds is not None:
        full = got_eds.copy()
        if parity_only:
            assert (full[:K, :K] == 0x5A).all(), "Q0 written under CEL_FLAG_PARITY_ONLY"
            full[:K, :K] = ods
        assert np.array_equal(full, e), "EDS differs"


def _check_round(out, want):
    one, ref1 = want["one"]
    _check_square(out["one"][0], [x[0] for x in out["one"][1:]], ref1)
    _check_square(out["parity"][0], [x[0] for x in out["parity"][1:]], ref1, True, one)
    _check_square(None, [x[0] for x in out["header"]], ref1)
    for name, par in (("host", True), ("dev", False)):
        odss, refs = want[name]
        for i, ref in enumerate(refs):
            _check_square(out[name][0][i], [x[i] for x in out[name][1:]], ref, par, odss[i])
    e, rr, cr, dah = want["block"][2]
    eds5, brr, bcr, bdah, kb = out["block"]
    assert kb == 1 and np.array_equal(eds5, e) and bdah.tobytes() == dah
    assert np.array_equal(brr[:2], rr) and np.array_equal(bcr[:2], cr)
    assert (brr[2:] == 0xC3).all() and (bcr[2:] == 0xC3).all()
    assert np.array_equal(out["repair"], ref1[0]), "repaired square differs"


def _flat(out):
    return [np.asarray(a) for key in sorted(out) for a in (out[key] if isinstance(out[key], tuple) else (out[key],))]


def test_entry_points_in_sequence(ctx, want):
    import celestia_eds
    from celestia_eds import _lib
    c = celestia_eds.Context(ctx.device)
    p_ods, ods_pin = _pinned(c, (K, K, 512))
    p_eds, eds_pin = _pinned(c, (W, W, 512))
    try:
        ods_pin[...] = want["one"][0]
        dev = {"ods": DeviceBuffer(N_DEV * K * K * 512), "eds": DeviceBuffer(N_DEV * W * W * 512),
               "rr": DeviceBuffer(N_DEV * W * 90), "cr": DeviceBuffer(N_DEV * W * 90), "dah": DeviceBuffer(N_DEV * 32),
               "st": DeviceBuffer(N_DEV * 4, fill=0x7F), "work": DeviceBuffer(c.lib.cel_dev_workspace_size(K, N_DEV))}
        dev["ods"].upload(want["dev"][0])
        bufs = {"p_ods": p_ods, "p_eds": p_eds, "eds_pin": eds_pin, "dev": dev}
        first = _round(c, want, bufs)
        second = _round(c, want, bufs)
        _check_round(first, want)
        _check_round(second, want)
        assert all(np.array_equal(a, b) for a, b in zip(_flat(first), _flat(second))), "the rounds differ"
        # column order broken only across rows k/2 - 1 / k/2: row k/2 takes row 0's namespaces
        bad = want["one"][0].copy()
        bad[K // 2, :, :29] = bad[0, :, :29]
        assert bad[K // 2, :, :29].tobytes() < bad[K // 2 - 1, :, :29].tobytes()
        ods_pin[...] = bad
        rr, cr, dah, st = np.zeros((W, 90), np.uint8), np.zeros((W, 90), np.uint8), np.zeros(32, np.uint8), np.zeros(1, np.int32)
        status = c.lib.cel_extend_batch(c.handle, ctypes.c_void_p(p_ods), 1, K, 512, None, _p(rr), _p(cr), _p(dah), _p(st),
                                        _lib.FLAG_ORDER_CHECK)
        assert status == _lib.EORDER and st[0] == _lib.EORDER
        assert c.lib.cel_last_error(c.handle).decode() == "invalid push order: leaf namespaces must be non-decreasing"
    finally:
        c.lib.cel_host_free(p_ods)
        c.lib.cel_host_free(p_eds)
        c.close()
