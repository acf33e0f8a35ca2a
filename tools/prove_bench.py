"""Times of the batched NMT prover on the sampling shape of tools/verify_bench.py: a k = 128
square and the samples of the p = 0.55, seed-7 mask with alternating axes (35,942 single-leaf
proofs of 8 nodes), and every cell on both axes (131,072 proofs).

  index_build   cel_dev_tree_index_build beside cel_dev_commit_only (n = 1) on the same square;
                the bytes the index keeps beyond the commit's workspace, priced at the same
                run's cel_probe_hbm_stream write rate
  prove         cel_dev_prove_batch on both sample sets; bytes moved (96 read + 90 written per
                node, 512 + 512 per share) over the call time, beside cel_probe_hbm_copy
  parent        the route to the same 35,942 proofs before the index: proof.axis_trees for both
                axes, then proof.nmt_prove_range per sample; its proofs must equal the batch's
  condition     index_build + prove (samples) < parent

Times are host wall clock around calls that end in a device synchronise, medians of --reps,
profiler off. Kernel times come from a run of its own under rocprofv3 --kernel-trace
(--no-parent keeps that run short); --trace-csv folds that run's kernel trace into the JSON.
Writes profiles/prove_bench.json.

  python tools/prove_bench.py [--reps 20] [--out profiles/prove_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/prove_bench.py --no-parent --out other.json
  python tools/prove_bench.py --trace-csv DIR/.../*_kernel_trace.csv --out profiles/prove_bench.json
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

NODE_BYTES = 96 + 90      # a record read, a packed node written
SHARE_BYTES = 512 + 512


def median_time(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def fold_trace(path, out):
    """Kernel times of a rocprofv3 --kernel-trace run of this tool into the JSON at `out`:
    per kernel, and for k_prove per grid size (the two sample sets), count and average."""
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            if "k_prove" in name:
                name = f"k_prove[grid {row.get('Grid_Size_X') or row.get('Grid_Size')}]"
            elif not any(x in name for x in ("k_leaf", "k_level", "k_merkle", "k_fill_i32")):
                continue
            by.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    with open(out) as f:
        result = json.load(f)
    result["kernel_trace"] = {n: {"dispatches": len(v), "average_us": sum(v) / len(v), "min_us": min(v)}
                              for n, v in sorted(by.items())}
    for key in ("samples", "all_cells"):
        p = result["prove"][key]
        ks = [v for n, v in result["kernel_trace"].items() if n == f"k_prove[grid {p['lanes']}]"]
        if ks:
            p["kernel_us"] = ks[0]["average_us"]
            p["kernel_gbps"] = p["bytes_moved"] / ks[0]["average_us"] / 1e3
            p["kernel_fraction_of_hbm_copy"] = p["kernel_gbps"] / result["probe"]["hbm_copy_gbps"]
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["kernel_trace"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--no-parent", action="store_true", help="skip the parent route (the profiled run)")
    ap.add_argument("--trace-csv", help="fold this kernel trace into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_bench.json"))
    args = ap.parse_args()
    if args.trace_csv:
        return fold_trace(args.trace_csv, args.out)
    k, w = args.k, 2 * args.k

    import celestia_eds
    from celestia_eds import da, proof
    from celestia_eds.testfactory import random_ods

    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def dmalloc(n):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), max(n, 1)) == 0, "hipMalloc"
        return p

    def download(d, shape):
        a = np.empty(shape, np.uint8)
        assert hip.hipMemcpy(P(a), d, a.nbytes, 2) == 0
        return a

    eds = da._extend(random_ods(k, 7).reshape(-1, 512), ctx=ctx)
    cells = np.ascontiguousarray(eds.cells)
    d_eds = dmalloc(cells.nbytes)
    assert hip.hipMemcpy(d_eds, P(cells), cells.nbytes, 1) == 0
    result = {"device": ctx.device_name(), "k": k, "reps": args.reps}

    copy, rd, wr = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    ctx.check(lib.cel_probe_hbm_stream(ctx.handle, 4 << 30, ctypes.byref(copy), ctypes.byref(rd), ctypes.byref(wr)))
    hc = ctypes.c_double()
    ctx.check(lib.cel_probe_hbm_copy(ctx.handle, 4 << 30, ctypes.byref(hc)))
    result["probe"] = {"hbm_copy_gbps": hc.value, "hbm_stream_copy_gbps": copy.value, "hbm_stream_read_gbps": rd.value,
                       "hbm_stream_write_gbps": wr.value}

    # ---- the index beside the commit
    index_bytes = lib.cel_dev_tree_index_size(k)
    d_index = dmalloc(index_bytes)
    d_rr, d_cr, d_dah, d_st = dmalloc(w * 90), dmalloc(w * 90), dmalloc(32), dmalloc(4)
    work_bytes = lib.cel_dev_workspace_size(k, 1)
    d_cwork = dmalloc(work_bytes)

    def index_build():
        ctx.check(lib.cel_dev_tree_index_build(ctx.handle, d_eds, k, d_index, d_rr, d_cr, d_dah, None, 0, None))
        assert hip.hipDeviceSynchronize() == 0

    def commit_only():
        ctx.check(lib.cel_dev_commit_only(ctx.handle, d_eds, 1, k, d_rr, d_cr, d_dah, d_st, d_cwork, None, 0))
        assert hip.hipDeviceSynchronize() == 0

    tc = median_time(commit_only, args.reps)
    roots_commit = (download(d_rr, (w, 90)), download(d_cr, (w, 90)), download(d_dah, (32,)))
    ti = median_time(index_build, args.reps)
    roots_index = (download(d_rr, (w, 90)), download(d_cr, (w, 90)), download(d_dah, (32,)))
    assert all(np.array_equal(a, b) for a, b in zip(roots_commit, roots_index)), "index roots differ from the commit's"
    # what the commit writes lands in its workspace (the leaves, then levels in two areas used in
    # turn); the index writes the same records, each level to memory of its own
    extra = max(index_bytes - work_bytes, 0)
    gap = ti["median"] - tc["median"]
    result["index_build"] = {
        "index_build_s": ti, "commit_only_s": tc, "ratio": ti["median"] / tc["median"], "gap_us": gap * 1e6,
        "index_bytes": index_bytes, "commit_workspace_bytes": work_bytes, "extra_bytes": extra,
        "extra_bytes_at_write_rate_us": extra / (wr.value * 1e9) * 1e6,
        "within_bound": gap <= extra / (wr.value * 1e9)}
    print("index_build", json.dumps(result["index_build"]), flush=True)

    # ---- the prove call
    present = (np.random.default_rng(7).random((w, w)) < 0.55).astype(np.uint8)
    coords = [(int(r), int(c)) for r, c in zip(*np.nonzero(present))]

    def request_set(rows, cols, axes):
        index = np.where(axes == 1, cols, rows).astype(np.uint32)
        starts = np.where(axes == 1, rows, cols).astype(np.int32)
        return dict(n=len(axes), axes=axes.astype(np.uint8), index=index, starts=starts, ends=starts + 1)

    n = len(coords)
    rows = np.array([r for r, _ in coords], np.uint32)
    cols = np.array([c for _, c in coords], np.uint32)
    sets = {"samples": request_set(rows, cols, (np.arange(n) % 2).astype(np.uint8))}
    rr_, cc_ = np.divmod(np.arange(w * w, dtype=np.uint32), w)
    sets["all_cells"] = request_set(np.concatenate([rr_, rr_]), np.concatenate([cc_, cc_]),
                                    np.repeat(np.array([0, 1], np.uint8), w * w))
    result["prove"] = {}
    flat = {}
    for key, q in sets.items():
        leaf_off, node_off = proof.prove_offsets(k, q["starts"], q["ends"])
        tl, tn = int(leaf_off[-1]), int(node_off[-1])
        d_leaves, d_nodes = dmalloc(tl * 512), dmalloc(tn * 90)
        d_work = dmalloc(lib.cel_dev_prove_workspace_size(q["n"]))

        def prove():
            ctx.check(lib.cel_dev_prove_batch(ctx.handle, d_eds, d_index, k, q["n"], P(q["axes"]), P(q["index"]),
                                              P(q["starts"]), P(q["ends"]), d_leaves, d_nodes, d_work, None))
            assert hip.hipDeviceSynchronize() == 0

        t = median_time(prove, args.reps)
        moved = tn * NODE_BYTES + tl * SHARE_BYTES
        result["prove"][key] = {"proofs": q["n"], "nodes": tn, "shares": tl, "lanes": ((q["n"] + 3) // 4) * 256, "s": t,
                                "us": t["median"] * 1e6, "table_bytes": 32 * q["n"], "bytes_moved": moved,
                                "call_gbps": moved / t["median"] / 1e9,
                                "call_fraction_of_hbm_copy": moved / t["median"] / 1e9 / hc.value}
        flat[key] = (download(d_leaves, (tl, 512)), download(d_nodes, (tn, 90)), node_off)
        print("prove", key, json.dumps(result["prove"][key]), flush=True)
    q = sets["samples"]
    assert np.array_equal(flat["samples"][0], cells[rows, cols]), "sample shares differ from the square's cells"

    # ---- the route before the index
    if not args.no_parent:
        def parent():
            trees = [proof.axis_trees(eds, axis, 0, w) for axis in (0, 1)]
            return [proof.nmt_prove_range(trees[a][t], s, s + 1) for a, t, s in zip(q["axes"], q["index"], q["starts"])]

        tp = median_time(parent, args.reps)
        want = np.frombuffer(b"".join(x for nl in parent() for x in nl), np.uint8).reshape(-1, 90)
        assert np.array_equal(flat["samples"][1], want), "batch proofs differ from the parent route's"
        ours = result["index_build"]["index_build_s"]["median"] + result["prove"]["samples"]["s"]["median"]
        result["parent"] = {"s": tp, "route": "proof.axis_trees for both axes + proof.nmt_prove_range per sample",
                            "index_build_plus_prove_s": ours, "speedup": tp["median"] / ours,
                            "condition_met": ours < tp["median"]}
        print("parent", json.dumps(result["parent"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not args.no_parent and not result["parent"]["condition_met"]:
        sys.exit("index build + prove call is not faster than the parent route")


if __name__ == "__main__":
    main()
