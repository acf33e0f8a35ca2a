"""cel_block_extend (txs in, data root and blob share commitments out, one upload) against the
three-call sequence it replaces, on the same txs, in the same process, alternating:

  baseline   cel_blob_tx_commitments + cel_square_construct + cel_extend_shares(eds_out = NULL),
             each part timed as well (the middle one is the host square construction)
  block      cel_block_extend with the commitments requested and eds_out = NULL

for three blocks, each the txs square.Build keeps of a generous candidate list:

  pfb_mix    k = 128: blobs of 200 B .. 20 KiB (log-uniform, one per blob tx) and 300 normal txs
  big_blobs  k = 128: 500 KiB blobs (sixteen are offered; the worst-case padding go-square
             reserves per blob lets fewer in, the count is recorded)
  k512       max_square_size = 512: 1 MiB blobs until the square is full

The txs (and the baseline's share buffer) are page-locked (cel_host_alloc). Times are host wall
clock around calls that end in a device synchronise; median, min, max and the 10th / 90th
percentile of --reps calls (default 20). "clears" says whether the block call's median is below
the baseline's median by more than the baseline's own spread (max - min, and p90 - p10).
Also recorded: cel_dev_square_build alone on device-resident txs (host layout fill, plan upload
and k_square_build; the kernel's own time comes from a kernel trace, tools/ktrace.py) next to
the same-run cel_probe_hbm_copy rate for the bytes it moves (about k*k*512 read and written).
Writes profiles/block_bench.json.

  python tools/block_bench.py [--reps 20] [--out profiles/block_bench.json] [--shapes a,b]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import celestia_eds  # noqa: E402
import block_inputs as B  # noqa: E402
from square_inputs import blob_tx  # noqa: E402


def _blob_txs(rng, lens):
    out = []
    for n in lens:
        ns_id = bytes(18) + rng.integers(0, 256, 10, np.uint8).tobytes()
        out.append(blob_tx(rng.integers(0, 256, int(rng.integers(150, 400)), np.uint8).tobytes(),
                           [(ns_id, rng.integers(0, 256, int(n), np.uint8).tobytes())]))
    return out


def candidates(rng):
    normal = [rng.integers(0, 256, int(rng.integers(40, 700)), np.uint8).tobytes() for _ in range(300)]
    mix = np.exp(rng.uniform(np.log(200), np.log(20 * 1024), 3000)).astype(np.int64)
    return {
        "pfb_mix": (normal + _blob_txs(rng, mix), 128),
        "big_blobs": (_blob_txs(rng, [500 * 1024] * 16), 128),
        "k512": (_blob_txs(rng, [1 << 20] * 124), 512),
    }


def stats(ts):
    a = np.sort(np.asarray(ts))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]),
            "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_bench.json"))
    ap.add_argument("--shapes", default="pfb_mix,big_blobs,k512")
    args = ap.parse_args()

    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    lib.cel_host_alloc.restype = ctypes.c_void_p
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rng = np.random.default_rng(11)
    result = {"device": ctx.device_name(), "reps": args.reps, "threshold": 64, "shapes": {}}

    def pinned(nbytes):
        hp = lib.cel_host_alloc(max(nbytes, 1))
        assert hp, "cel_host_alloc failed"
        return hp, np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_uint8)), (max(nbytes, 1),))

    for name, (cand, max_sq) in candidates(rng).items():
        if name not in args.shapes.split(","):
            continue
        _, _, _, included, _, _ = B.layout(cand, max_sq, 64, 1)
        txs = [t for t, s in zip(cand, included) if s == 1] + [t for t, s in zip(cand, included) if s == 2]
        st, err, k, _, segs, compact = B.layout(txs, max_sq, 64, 0)
        assert st == 0, err
        raw = b"".join(txs)
        ntx = len(txs)
        lens = np.array([len(t) for t in txs], np.uint32)
        hp, htx = pinned(len(raw))
        htx[:len(raw)] = np.frombuffer(raw, np.uint8)
        hs, hshares = pinned(k * k * 512)
        n = ctypes.c_uint32()
        ctx.check(lib.cel_blob_tx_commitments(ctx.handle, hp, P(lens), ntx, 64, None, None, 0, ctypes.byref(n)))
        nb = n.value
        com_a, com_b = np.zeros((nb, 32), np.uint8), np.zeros((nb, 32), np.uint8)
        txi_a, txi_b = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32)
        rr_a, cr_a = np.zeros((2 * k, 90), np.uint8), np.zeros((2 * k, 90), np.uint8)
        rr_b, cr_b = np.zeros((2 * max_sq, 90), np.uint8), np.zeros((2 * max_sq, 90), np.uint8)
        dah_a, dah_b = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
        kk = ctypes.c_uint32()

        def baseline():
            t0 = time.perf_counter()
            ctx.check(lib.cel_blob_tx_commitments(ctx.handle, hp, P(lens), ntx, 64, P(com_a), P(txi_a), nb,
                                                  ctypes.byref(n)))
            t1 = time.perf_counter()
            assert lib.cel_square_construct(hp, P(lens), ntx, max_sq, 64, 0, hs, k * k, ctypes.byref(kk), None) == 0
            t2 = time.perf_counter()
            ctx.check(lib.cel_extend_shares(ctx.handle, hs, k * k, 512, None, P(rr_a), P(cr_a), P(dah_a), 1))
            t3 = time.perf_counter()
            return t3 - t0, t1 - t0, t2 - t1, t3 - t2

        def block():
            t0 = time.perf_counter()
            ctx.check(lib.cel_block_extend(ctx.handle, hp, P(lens), ntx, max_sq, 64, 0, ctypes.byref(kk), None,
                                           P(rr_b), P(cr_b), P(dah_b), None, 0, P(com_b), P(txi_b), nb,
                                           ctypes.byref(n), 1))
            return time.perf_counter() - t0

        def layout_only():
            t0 = time.perf_counter()
            B.lib().cel_square_layout(hp, P(lens), ntx, max_sq, 64, 0, ctypes.byref(kk), None, None, 0,
                                      ctypes.byref(n), None, 0, ctypes.byref(n))
            return time.perf_counter() - t0

        for _ in range(3):  # warm-up: scratch and staging grow on the first calls
            baseline(), block()
        assert dah_a.tobytes() == dah_b.tobytes() and np.array_equal(com_a, com_b) and np.array_equal(txi_a, txi_b)
        assert np.array_equal(rr_a, rr_b[:2 * k]) and np.array_equal(cr_a, cr_b[:2 * k]), "paths disagree"
        base, blk, lay = [], [], []
        for _ in range(args.reps):
            base.append(baseline())
            blk.append(block())
            lay.append(layout_only())
        base = np.array(base)
        b_tot, b_new = stats(base[:, 0]), stats(blk)
        gain = b_tot["median"] - b_new["median"]

        # the device-resident step alone, and the copy probe for the bytes it moves
        d_txs, d_eds = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d_txs), len(raw) + 8) == 0 and hip.hipMalloc(ctypes.byref(d_eds), 4 * k * k * 512) == 0
        assert hip.hipMemcpy(d_txs, hp, len(raw), 1) == 0
        arr = (B.Segment * len(segs))(*segs)

        def dev_build():
            t0 = time.perf_counter()
            ctx.check(lib.cel_dev_square_build(ctx.handle, d_txs, arr, len(segs), P(compact), len(compact), k, d_eds, None))
            assert hip.hipDeviceSynchronize() == 0
            return time.perf_counter() - t0

        dev_build(), dev_build()
        dev = stats([dev_build() for _ in range(args.reps)])
        gbps = ctypes.c_double()
        ctx.check(lib.cel_probe_hbm_copy(ctx.handle, 2 * k * k * 512, ctypes.byref(gbps)))
        hip.hipFree(d_txs), hip.hipFree(d_eds)

        result["shapes"][name] = {
            "k": k, "max_square_size": max_sq, "txs": ntx, "blobs": nb, "tx_bytes": len(raw),
            "offered_txs": len(cand), "segments": len(segs), "compact_shares": len(compact),
            "baseline_s": b_tot,
            "baseline_parts_s": {"blob_tx_commitments": stats(base[:, 1]), "square_construct_host": stats(base[:, 2]),
                                 "extend_shares": stats(base[:, 3])},
            "block_extend_s": b_new,
            "host_layout_s": stats(lay),
            "gain_s": gain, "speedup": b_tot["median"] / b_new["median"],
            "clears_spread_max_min": bool(gain > b_tot["max"] - b_tot["min"]),
            "clears_spread_p90_p10": bool(gain > b_tot["p90"] - b_tot["p10"]),
            "dev_square_build_call_s": dev,
            "square_bytes_moved": 2 * k * k * 512,
            "probe_hbm_copy_gbps": gbps.value,
            "probe_copy_time_for_those_bytes_s": 2 * k * k * 512 / (gbps.value * 1e9),
        }
        print(name, json.dumps(result["shapes"][name]), flush=True)
        lib.cel_host_free(ctypes.c_void_p(hp))
        lib.cel_host_free(ctypes.c_void_p(hs))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
