"""Times of the namespace queries on a k = 128 square whose ODS carries namespaces in runs of
1 .. 3k shares, for n = 1, 64 and 1024 queried namespaces, half of them absent (the present
half drawn from the square's namespaces, with repetition where there are fewer of them; the
absent half drawn from the values between two runs).

  plan / prove   cel_dev_namespace_plan (synchronous) and cel_dev_namespace_prove + a device
                 synchronise, on the resident index
  verify         cel_dev_nmt_verify_namespace_batch on the producer's own device output, whole and
                 with CEL_VERIFY_STAGES = 2 (leaves) and 4 (fold) over the records the whole run left
  parent         the route to the same answers before this: proof.axis_trees for the k upper rows,
                 then proof.nmt_prove_namespace per (namespace, row); its bytes must equal the device's
  emit_vs_prove  the present namespaces alone (every entry an inclusion entry) through
                 cel_dev_namespace_prove, and the same ranges through cel_dev_prove_batch: the same
                 bytes moved (96 read + 90 written per node, 512 + 512 per share), beside
                 cel_probe_hbm_copy of the same run

Times are host wall clock around calls that end in a device synchronise, medians of --reps
(the parent route: of at most 5), profiler off. Kernel times come from a run of its own under
rocprofv3 --kernel-trace (--no-parent keeps that run short); --trace-csv folds that run's kernel
trace into the JSON, with the kernels' shares of the copy probe of that same traced run
(--trace-json). Writes profiles/namespace_bench.json.

  python tools/namespace_bench.py [--reps 20] [--out profiles/namespace_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- \
      python tools/namespace_bench.py --no-parent --out DIR/other.json
  python tools/namespace_bench.py --trace-csv DIR/.../t_kernel_trace.csv --trace-json DIR/other.json \
      --out profiles/namespace_bench.json
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
KERNELS = ("k_ns_find", "k_ns_sums", "k_ns_scan", "k_ns_compact", "k_ns_emit", "k_prove", "k_verify_ns_leaves",
           "k_verify_ns_fold", "k_verify_repack")


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


def ns_value(v):
    return bytes(19) + int(v).to_bytes(10, "big")


def run_square(k, seed):
    """ODS of runs of 1 .. 3k shares, run i under namespace 1000 * (i + 1)."""
    rng = np.random.default_rng(seed)
    ods = rng.integers(0, 256, (k * k, 512), dtype=np.uint8)
    at, i = 0, 0
    while at < k * k:
        r = min(int(rng.integers(1, 3 * k + 1)), k * k - at)
        ods[at:at + r, :29] = np.frombuffer(ns_value(1000 * (i + 1)), np.uint8)
        at += r
        i += 1
    return ods, i


def query_set(n, runs, seed):
    rng = np.random.default_rng(seed)
    half = n // 2
    present = [ns_value(1000 * (int(i) + 1)) for i in rng.integers(0, runs, n - half)]
    absent = [ns_value(1000 * (int(i) + 1) + int(d)) for i, d in zip(rng.integers(0, runs, half), rng.integers(1, 1000, half))]
    qs = present + absent
    return [qs[i] for i in rng.permutation(n)]


def fold_trace(path, out, trace_json=None):
    """Kernel times of a rocprofv3 --kernel-trace run of this tool into the JSON at `out`: per
    kernel and grid size, count and average; the emit and prove kernels beside the copy probe."""
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            hit = [x for x in KERNELS if x in row["Kernel_Name"]]  # the names carry "(anonymous namespace)"
            if not hit:
                continue
            key = f"{hit[0]}[grid {row.get('Grid_Size_X') or row.get('Grid_Size')}]"
            by.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    with open(out) as f:
        result = json.load(f)
    trace = {n: {"dispatches": len(v), "average_us": sum(v) / len(v), "min_us": min(v)} for n, v in sorted(by.items())}
    result["kernel_trace"] = trace
    ev = result["emit_vs_prove"]
    probe = result["probe"]["hbm_copy_gbps"]
    if trace_json:  # the probe of the run the kernel times come from
        with open(trace_json) as f:
            probe = json.load(f)["probe"]["hbm_copy_gbps"]
        ev["traced_run_hbm_copy_gbps"] = probe
    for kernel, key in (("k_ns_emit", "emit"), ("k_prove", "prove")):
        ks = trace.get(f"{kernel}[grid {ev['lanes']}]")
        if ks:
            ev[key + "_kernel_us"] = ks["average_us"]
            ev[key + "_kernel_gbps"] = ev["bytes_moved"] / ks["average_us"] / 1e3
            ev[key + "_kernel_fraction_of_hbm_copy"] = ev[key + "_kernel_gbps"] / probe
    for n, q in result["queries"].items():
        for kernel in ("k_ns_find", "k_ns_sums", "k_ns_scan", "k_ns_compact", "k_ns_emit", "k_verify_ns_leaves",
                       "k_verify_ns_fold"):
            ks = trace.get(f"{kernel}[grid {q['grids'][kernel]}]")
            if ks:
                q.setdefault("kernel_us", {})[kernel] = ks["average_us"]
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(trace, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--no-parent", action="store_true", help="skip the parent route (the profiled run)")
    ap.add_argument("--trace-csv", help="fold this kernel trace into --out and stop")
    ap.add_argument("--trace-json", help="the JSON the traced run wrote: its copy probe prices the kernel times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "namespace_bench.json"))
    args = ap.parse_args()
    if args.trace_csv:
        return fold_trace(args.trace_csv, args.out, args.trace_json)
    k, w = args.k, 2 * args.k

    import celestia_eds
    from celestia_eds import da, proof

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

    ods, runs = run_square(k, 7)
    eds = da._extend(ods, ctx=ctx)
    cells = np.ascontiguousarray(eds.cells)
    d_eds = dmalloc(cells.nbytes)
    assert hip.hipMemcpy(d_eds, P(cells), cells.nbytes, 1) == 0
    result = {"device": ctx.device_name(), "k": k, "reps": args.reps, "runs": runs, "run_lengths": f"1 .. {3 * k}"}

    hc = ctypes.c_double()
    ctx.check(lib.cel_probe_hbm_copy(ctx.handle, 4 << 30, ctypes.byref(hc)))
    result["probe"] = {"hbm_copy_gbps": hc.value}

    d_index = dmalloc(lib.cel_dev_tree_index_size(k))
    d_roots = dmalloc(2 * w * 90)
    d_cr = ctypes.c_void_p(d_roots.value + w * 90)
    ctx.check(lib.cel_dev_tree_index_build(ctx.handle, d_eds, k, d_index, d_roots, d_cr, None, None, 0, None))
    assert hip.hipDeviceSynchronize() == 0

    def plan_and_prove(queries, reps):
        """The plan, the proofs and the verifier over `queries`; times and the outputs."""
        n = len(queries)
        ns = np.frombuffer(b"".join(queries), np.uint8).copy()
        cap = n * w
        arr = dict(ns_idx=np.zeros(cap, np.uint32), rows=np.zeros(cap, np.uint32), starts=np.zeros(cap, np.int32),
                   ends=np.zeros(cap, np.int32), kinds=np.zeros(cap, np.uint8), leaf_off=np.zeros(cap + 1, np.uint64),
                   node_off=np.zeros(cap + 1, np.uint64))
        cnt = ctypes.c_uint64()
        d_work = dmalloc(lib.cel_dev_namespace_workspace_size(k, n))

        def plan():
            ctx.check(lib.cel_dev_namespace_plan(ctx.handle, d_index, k, n, P(ns), cap, P(arr["ns_idx"]), P(arr["rows"]),
                                                 P(arr["starts"]), P(arr["ends"]), P(arr["kinds"]), P(arr["leaf_off"]),
                                                 P(arr["node_off"]), ctypes.byref(cnt), d_work, None))

        t_plan = median_time(plan, reps)
        m = cnt.value
        e = {key: v[:m + 1] if key.endswith("_off") else v[:m] for key, v in arr.items()}
        tl, tn = int(e["leaf_off"][-1]), int(e["node_off"][-1])
        d_leaves, d_nodes = dmalloc(tl * 512), dmalloc(tn * 90)

        def prove():
            ctx.check(lib.cel_dev_namespace_prove(ctx.handle, d_eds, d_index, k, m, d_leaves, d_nodes, d_work, None))
            assert hip.hipDeviceSynchronize() == 0

        t_prove = median_time(prove, reps)
        qns = np.stack([np.frombuffer(queries[i], np.uint8) for i in e["ns_idx"]]) if m else np.zeros((1, 29), np.uint8)
        d_ok = dmalloc(m)
        d_vwork = dmalloc(lib.cel_dev_nmt_verify_namespace_workspace_size(tl, tn, m))

        def verify():
            ctx.check(lib.cel_dev_nmt_verify_namespace_batch(ctx.handle, m, P(e["starts"]), P(e["ends"]), P(e["kinds"]), P(qns),
                                                             d_leaves, P(e["leaf_off"]), d_nodes, P(e["node_off"]), d_roots,
                                                             2 * w, P(e["rows"]), d_ok, d_vwork, None))
            assert hip.hipDeviceSynchronize() == 0

        t_verify = median_time(verify, reps)
        assert (download(d_ok, (m,)) == 1).all(), "a produced proof does not verify"
        stages = {}
        for name, mask in (("leaves", "2"), ("fold", "4")):
            os.environ["CEL_VERIFY_STAGES"] = mask
            stages[name] = median_time(verify, reps)
        os.environ.pop("CEL_VERIFY_STAGES")
        verify()
        stats = {"namespaces": n, "entries": m, "absence_entries": int((e["kinds"] == 1).sum()), "nodes": tn, "shares": tl,
                 "plan_s": t_plan, "prove_s": t_prove, "plan_us": t_plan["median"] * 1e6, "prove_us": t_prove["median"] * 1e6,
                 "verify_s": t_verify, "verify_us": t_verify["median"] * 1e6,
                 "verify_leaves_stage_us": stages["leaves"]["median"] * 1e6,
                 "verify_fold_stage_us": stages["fold"]["median"] * 1e6,
                 "bytes_moved": tn * NODE_BYTES + tl * SHARE_BYTES,
                 "grids": {"k_ns_find": ((n * ((w + 63) // 64) + 3) // 4) * 256, "k_ns_sums": ((n * w + 255) // 256) * 256, "k_ns_scan": 256,
                           "k_ns_compact": ((n * w + 255) // 256) * 256, "k_ns_emit": ((m + 3) // 4) * 256,
                           "k_verify_ns_leaves": ((tl + 255) // 256) * 256, "k_verify_ns_fold": ((m + 255) // 256) * 256}}
        return stats, e, download(d_leaves, (tl, 512)), download(d_nodes, (tn, 90)), (d_leaves, d_nodes)

    result["queries"] = {}
    for n in (1, 64, 1024):
        queries = query_set(n, runs, 100 + n)
        stats, e, leaves, nodes, _ = plan_and_prove(queries, args.reps)
        if not args.no_parent:
            def parent():
                trees = proof.axis_trees(eds, 0, 0, k)
                return [(i, r, proof.nmt_prove_namespace(trees[r], w, q)) for i, q in enumerate(queries) for r in range(k)]

            preps = min(args.reps, 5)
            tp = median_time(parent, preps)
            got = [(i, r, p) for i, r, p in parent() if p is not None]
            assert [(i, r, p.Start, p.End) for i, r, p in got] == list(zip(e["ns_idx"], e["rows"], e["starts"], e["ends"]))
            want = b"".join(x for _, _, p in got for x in list(p.Nodes) + ([p.LeafHash] if p.LeafHash else []))
            assert nodes.tobytes() == want, "device nodes differ from the parent route's"
            ours = stats["plan_s"]["median"] + stats["prove_s"]["median"]
            stats["parent"] = {"s": tp, "reps": preps, "route": "proof.axis_trees for the k upper rows + "
                               "proof.nmt_prove_namespace per (namespace, row)", "plan_plus_prove_s": ours,
                               "speedup": tp["median"] / ours}
        result["queries"][str(n)] = stats
        print("queries", n, json.dumps(stats), flush=True)

    # ---- the emit kernel beside k_prove on the same bytes: every present namespace, inclusion alone
    queries = [ns_value(1000 * (i + 1)) for i in range(runs)]
    stats, e, leaves, nodes, (d_leaves, d_nodes) = plan_and_prove(queries, args.reps)
    assert (e["kinds"] == 0).all()
    m = len(e["rows"])
    axes = np.zeros(m, np.uint8)
    d_pwork = dmalloc(lib.cel_dev_prove_workspace_size(m))

    def prove_batch():
        ctx.check(lib.cel_dev_prove_batch(ctx.handle, d_eds, d_index, k, m, P(axes), P(e["rows"]), P(e["starts"]), P(e["ends"]),
                                          d_leaves, d_nodes, d_pwork, None))
        assert hip.hipDeviceSynchronize() == 0

    tb = median_time(prove_batch, args.reps)
    assert np.array_equal(download(d_nodes, nodes.shape), nodes) and np.array_equal(download(d_leaves, leaves.shape), leaves)
    result["emit_vs_prove"] = {"entries": m, "nodes": stats["nodes"], "shares": stats["shares"],
                               "bytes_moved": stats["bytes_moved"], "lanes": ((m + 3) // 4) * 256,
                               "emit_call_us": stats["prove_us"], "prove_batch_call_us": tb["median"] * 1e6,
                               "emit_call_s": stats["prove_s"], "prove_batch_call_s": tb}
    print("emit_vs_prove", json.dumps(result["emit_vs_prove"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
