"""Rate of the blob share commitments (cel_dev_create_commitments on device-resident blob
bytes, cel_create_commitments from page-locked host memory) next to the same-run SHA-256
probe (cel_probe_sha256), for

  blobs64k   256 blobs of 64 KiB
  pfb_mix    2000 blobs of 200 B .. 20 KiB (a PayForBlobs-like mix)
  bulk       64 blobs of 4 MiB (enough work that launches and the plan upload do not
             dominate: the kernels' own rate)

Times are host wall clock around calls that end in a device synchronise, so the device
entry's figure includes the host planning and the plan-table upload of every call.
Compressions are counted from the shapes: 9 per leaf, 3 per NMT inner node, 2 per
RFC-6962 leaf or inner node. Writes profiles/commitments_bench.json.

  python tools/commit_bench.py [--reps 20] [--out profiles/commitments_bench.json]
                               [--leaf-ab profiles/commitments_leaf_ab.txt]

--leaf-ab also times the leaf stage's A/B partner (shares expanded into device memory, then
the EDS commit's leaf_hash; CEL_COMMIT_LEAF=expanded) against the shipped direct read.
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

import celestia_eds  # noqa: E402
from celestia_eds import inclusion  # noqa: E402

H2D = 1


def batches(rng):
    return {
        "blobs64k": [65536] * 256,
        "pfb_mix": [int(x) for x in rng.integers(200, 20 * 1024 + 1, 2000)],
        "bulk": [4 << 20] * 64,
    }


def compressions(lens, threshold):
    leaf = node = rfc = shares = 0
    for n in lens:
        s, _, sizes = inclusion.blob_subtree_sizes(n, threshold)
        shares += s
        leaf += 9 * s
        node += 3 * (s - len(sizes))
        rfc += 2 * (2 * len(sizes) - 1)
    return shares, {"leaf": leaf, "nmt_node": node, "rfc": rfc, "total": leaf + node + rfc}


def median_time(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threshold", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commitments_bench.json"))
    ap.add_argument("--leaf-ab", default=None, help="also run the leaf stage A/B and write it to this text file")
    args = ap.parse_args()
    ab_lines = []

    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.cel_host_alloc.restype = ctypes.c_void_p

    def dmalloc(n):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(n, 1)) == 0, "hipMalloc"
        return p

    def probe():
        g, mhz = ctypes.c_double(), ctypes.c_double()
        ctx.check(lib.cel_probe_sha256(ctx.handle, ctypes.byref(g), ctypes.byref(mhz)))
        return g.value, mhz.value

    rng = np.random.default_rng(7)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    result = {"device": ctx.device_name(), "threshold": args.threshold, "reps": args.reps, "batches": {}}
    peak0, mhz0 = probe()
    for name, lens in batches(rng).items():
        nb, total = len(lens), sum(lens)
        shares, comp = compressions(lens, args.threshold)
        offsets = np.zeros(nb + 1, np.uint64)
        np.cumsum(lens, out=offsets[1:])
        ns = np.zeros((nb, 29), np.uint8)
        ns[:, 19:] = rng.integers(0, 256, (nb, 10), np.uint8)
        hp = lib.cel_host_alloc(total)
        assert hp, "cel_host_alloc failed"
        data = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_uint8)), (total,))
        data[:] = rng.integers(0, 256, total, np.uint8)
        d_data, d_out = dmalloc(total), dmalloc(32 * nb)
        d_work = dmalloc(lib.cel_dev_commitments_workspace_size(shares, nb))
        assert hip.hipMemcpy(d_data, hp, total, H2D) == 0
        out_dev = np.zeros((nb, 32), np.uint8)
        out_host = np.zeros((nb, 32), np.uint8)

        def dev_call():
            ctx.check(lib.cel_dev_create_commitments(ctx.handle, d_data, P(offsets), nb, P(ns), None, args.threshold,
                                                     d_out, d_work, None))
            assert hip.hipDeviceSynchronize() == 0

        def host_call():
            ctx.check(lib.cel_create_commitments(ctx.handle, hp, P(offsets), nb, P(ns), None, args.threshold,
                                                 P(out_host)))

        if args.leaf_ab:
            # leaf stage A/B: the direct read of blob bytes against shares expanded into device
            # memory and hashed by the EDS commit's leaf_hash (CEL_COMMIT_LEAF=expanded, read
            # by the library on every call), alternating in one process, same inputs
            outs = {}
            for rnd in range(3):
                for mode in ("direct", "expanded"):
                    os.environ["CEL_COMMIT_LEAF"] = mode
                    t = median_time(dev_call, args.reps)
                    o = np.zeros((nb, 32), np.uint8)
                    assert hip.hipMemcpy(P(o), d_out, 32 * nb, 2) == 0
                    outs[mode] = o
                    ab_lines.append(f"{name:9s} round {rnd} {mode:8s} median {t[0] * 1e6:9.1f} us  min {t[1] * 1e6:9.1f} us"
                                    f"  ({shares / t[0] / 1e6:7.1f} M shares/s)")
            os.environ["CEL_COMMIT_LEAF"] = "direct"
            assert np.array_equal(outs["direct"], outs["expanded"]), "leaf variants disagree"
        peak, mhz = probe()
        dev = median_time(dev_call, args.reps)
        host = median_time(host_call, max(args.reps // 4, 3))
        assert hip.hipMemcpy(P(out_dev), d_out, 32 * nb, 2) == 0
        assert np.array_equal(out_dev, out_host), "device-resident and host entry disagree"
        gcomp = comp["total"] / dev[0] / 1e9
        result["batches"][name] = {
            "blobs": nb, "bytes": total, "shares": shares, "compressions": comp,
            "dev_entry_s": {"median": dev[0], "min": dev[1], "max": dev[2]},
            "dev_blobs_per_s": nb / dev[0], "dev_shares_per_s": shares / dev[0],
            "dev_gcompressions_per_s": gcomp,
            "probe_gcompressions_per_s": peak, "probe_shader_mhz": mhz,
            "fraction_of_probe_peak": gcomp / peak,
            "host_entry_pinned_s": {"median": host[0], "min": host[1], "max": host[2]},
            "host_blobs_per_s": nb / host[0], "host_gbytes_per_s": total / host[0] / 1e9,
        }
        print(name, json.dumps(result["batches"][name]), flush=True)
        for p in (d_data, d_out, d_work):
            hip.hipFree(p)
        lib.cel_host_free(ctypes.c_void_p(hp))
    if args.leaf_ab:
        with open(args.leaf_ab, "w") as f:
            f.write("Leaf stage A/B of the blob commitments (tools/commit_bench.py --leaf-ab), " + result["device"] + "\n"
                    "cel_dev_create_commitments on device-resident blobs, host wall clock per call ending in a\n"
                    "device synchronise (host planning and the plan upload included in both), median of "
                    f"{args.reps} calls.\n"
                    "direct   = k_blob_tile<false>: leaf message formed from the blob bytes\n"
                    "expanded = k_blob_expand writes every share to device memory, k_blob_tile<true> hashes\n"
                    "           them with leaf_hash; commitments compared equal\n\n")
            f.write("\n".join(ab_lines) + "\n")
    result["probe_first_gcompressions_per_s"] = peak0
    result["probe_first_shader_mhz"] = mhz0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
