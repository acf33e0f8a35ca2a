"""Times of the batched fraud-proof verifier at k = 128: 1, 16 and 256 proofs of k entries each
(an honest square's rows, data half, every entry proved in its column tree), medians of --reps.

  batch    cel_befp_verify_batch: one upload, verify -> place -> decode -> encode -> roots ->
           verdict on one stream, one download
  chained  what a caller had before it, in the same loop: cel_nmt_verify_batch over every
           entry, then per proof cel_codec_decode, cel_codec_encode and cel_axis_root (three
           synchronous calls, each with its own upload and download), the root compared on the
           host; its verdicts must equal the batch's
  probe    cel_probe_hbm_copy over the bytes the place kernel moves for 256 proofs (each share
           read once and written once), the same run's ceiling for that kernel

Times are host wall clock around synchronous calls, profiler off. Kernel times come from a run
of its own under rocprofv3 --kernel-trace --stats (--profile keeps that run to the batch route),
folded into a text table by --trace-csv. Writes profiles/befp_bench.json.

  python tools/befp_bench.py [--reps 20] [--out profiles/befp_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/befp_bench.py --profile
  python tools/befp_bench.py --trace-csv DIR/.../*_kernel_trace.csv --json profiles/befp_bench.json \
      --out profiles/befp_kernel_times.txt
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

COUNTS = (1, 16, 256)


def fold_trace(path, bench_json, out):
    """The kernel trace of a --profile run as a table: per kernel, dispatches, average and
    minimum microseconds; the place kernel beside the HBM copy probe of the JSON."""
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            by.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    with open(bench_json) as f:
        bench = json.load(f)
    lines = [f"rocprofv3 --kernel-trace --stats of tools/befp_bench.py --profile on {bench['device']}:",
             f"cel_befp_verify_batch, k = {bench['k']}, {COUNTS[-1]} proofs of k entries, all dispatches of the run",
             "", f"{'kernel':<64} {'dispatches':>10} {'avg us':>10} {'min us':>10}"]
    for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{name[:64]:<64} {len(v):>10} {sum(v) / len(v):>10.2f} {min(v):>10.2f}")
    place = [v for n, v in by.items() if "k_befp_place" in n]
    if place:
        moved, gbps = bench["probe"]["place_bytes_moved"], bench["probe"]["hbm_copy_gbps"]
        us = min(place[0])
        lines += ["", f"k_befp_place moves {moved} bytes (each share read and written once): {moved / us / 1e3:.0f} GB/s "
                      f"at its best dispatch, {moved / us / 1e3 / gbps:.2f} of the same-size cel_probe_hbm_copy "
                      f"({gbps:.0f} GB/s, from the timing run)"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--profile", action="store_true", help="the batch route alone, 256 proofs, a few calls")
    ap.add_argument("--trace-csv", help="fold this kernel trace into --out (a text table) and stop")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "befp_bench.json"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_csv:
        return fold_trace(args.trace_csv, args.json, args.out or os.path.join(ROOT, "profiles", "befp_kernel_times.txt"))
    out_path = args.out or args.json
    k, w = args.k, 2 * args.k

    import celestia_eds
    from celestia_eds import _lib, da
    from celestia_eds.testfactory import random_ods

    ctx = celestia_eds.default_context(0)
    lib, h = ctx.lib, ctx.handle
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    eds = da._extend(random_ods(k, 7).reshape(-1, 512), ctx=ctx)
    rr = np.frombuffer(b"".join(eds.RowRoots()), np.uint8).copy()
    cr = np.frombuffer(b"".join(eds.ColRoots()), np.uint8).copy()
    per = w.bit_length() - 1
    result = {"device": ctx.device_name(), "k": k, "reps": args.reps, "entries_per_proof": k, "proofs": {}}

    def inputs(n):
        """n proofs: row i of the square, its k data cells, each proved in its column's tree."""
        rows = np.arange(n, dtype=np.uint32) % w
        coords = [(int(r), c, 1) for r in rows for c in range(k)]
        got = eds.SampleProofs(coords)
        return dict(
            n=n, axes=np.zeros(n, np.uint8), index=rows, ent_off=(np.arange(n + 1, dtype=np.uint64) * k),
            pos=np.tile(np.arange(k, dtype=np.uint32), n), ea=np.ones(n * k, np.uint8),
            shares=np.frombuffer(b"".join(g[3] for g in got), np.uint8).copy(),
            nodes=np.frombuffer(b"".join(x for g in got for x in g[4]), np.uint8).copy(),
            node_off=(np.arange(n * k + 1, dtype=np.uint64) * per), rr=np.tile(rr, n), cr=np.tile(cr, n))

    def batch(q):
        out = np.full(q["n"], 0xEE, np.uint8)
        ctx.check(lib.cel_befp_verify_batch(h, q["n"], k, P(q["axes"]), P(q["index"]), P(q["ent_off"]), P(q["pos"]),
                                            P(q["ea"]), P(q["shares"]), P(q["nodes"]), P(q["node_off"]), P(q["rr"]),
                                            P(q["cr"]), P(out), None))
        return out

    def chained(q):
        n, ne = q["n"], q["n"] * k
        starts = np.repeat(q["index"], k).astype(np.int32)  # leaf = the row, in column pos's tree
        ns = q["shares"].reshape(ne, 512)[:, :29].copy()
        ns[np.repeat(q["index"], k) >= k] = 0xFF
        root_idx = q["pos"].astype(np.uint32)
        leaf_off = np.arange(ne + 1, dtype=np.uint64)
        ok = np.zeros(ne, np.uint8)
        ctx.check(lib.cel_nmt_verify_batch(h, ne, P(starts), P(starts + 1), P(ns), P(q["shares"]), P(leaf_off),
                                           P(q["nodes"]), P(q["node_off"]), P(cr), w, P(root_idx), P(ok)))
        out = np.zeros(n, np.uint8)
        present = np.zeros(w, np.uint8)
        present[:k] = 1
        for i in range(n):
            if not ok[i * k:(i + 1) * k].all():
                out[i] = _lib.BEFP_BAD_SHARE
                continue
            shards = np.zeros((w, 512), np.uint8)
            shards[:k] = q["shares"].reshape(ne, 512)[i * k:(i + 1) * k]
            ctx.check(lib.cel_codec_decode(h, P(shards), P(present), k, 512))
            ctx.check(lib.cel_codec_encode(h, P(shards), k, 512, P(shards[k:])))
            root = np.zeros(90, np.uint8)
            ctx.check(lib.cel_axis_root(h, P(shards), k, int(q["index"][i]), 512, P(root), 0))
            r0 = int(q["index"][i]) * 90
            out[i] = _lib.BEFP_NOT_FRAUD if np.array_equal(root, rr[r0:r0 + 90]) else _lib.BEFP_FRAUD
        return out

    if args.profile:
        q = inputs(COUNTS[-1])
        for _ in range(5):
            assert not batch(q).any()
        return
    place_bytes = COUNTS[-1] * k * 512 * 2
    hc = ctypes.c_double()
    ctx.check(lib.cel_probe_hbm_copy(h, place_bytes, ctypes.byref(hc)))
    result["probe"] = {"place_bytes_moved": place_bytes, "hbm_copy_gbps": hc.value}
    for n in COUNTS:
        q = inputs(n)
        a, b = batch(q), chained(q)
        assert not a.any() and np.array_equal(a, b), "the two routes disagree"
        ta, tb = [], []
        for _ in range(args.reps):  # the same loop: one call of each per turn
            t0 = time.perf_counter()
            batch(q)
            t1 = time.perf_counter()
            chained(q)
            t2 = time.perf_counter()
            ta.append(t1 - t0)
            tb.append(t2 - t1)
        ta.sort()
        tb.sort()
        result["proofs"][str(n)] = {
            "entries": n * k, "batch_us": ta[len(ta) // 2] * 1e6, "batch_min_us": ta[0] * 1e6,
            "chained_us": tb[len(tb) // 2] * 1e6, "chained_min_us": tb[0] * 1e6,
            "chained_over_batch": tb[len(tb) // 2] / ta[len(ta) // 2]}
        print(n, json.dumps(result["proofs"][str(n)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
