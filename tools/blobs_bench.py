"""Times of blobs by namespace on a k = 128 square (the shape of profiles/namespace_bench.json):
the ODS carries namespaces in runs of 1 .. 3k shares, each run one to four blobs, and n = 1, 64
and 1024 namespaces are queried, half of them absent (the present half drawn from the square's
namespaces, with repetition where there are fewer of them).

  device   the square and its tree index resident: cel_dev_namespace_plan, cel_namespace_ods_ranges,
           cel_dev_blobs_plan, cel_dev_blobs_emit with commitments, a stream synchronise. Only the
           records (64 bytes a blob) and the plan's arrays cross PCIe. blobs_plan_us and
           blobs_emit_us are the two new calls alone.
  before   the route to the same answers before this: cel_namespace_rows (upload, index, plan,
           proofs, download of the shares), blob.parse_sparse_shares over each namespace's shares on
           the host, cel_create_commitments from host memory. before_resident is the same with the
           square and index resident (TreeIndex.namespace_flat in place of cel_namespace_rows).
  gather   k_bp_gather alone over the whole ODS as one range (every blob of the square): ten
           cel_dev_blobs_emit calls without commitments between two events, a tenth of the
           elapsed time; its bytes (each blob's padded length read and written) per second beside
           cel_probe_hbm_copy of the same run.

Both routes run in this process on the same square, and their blobs and commitments must be equal.
Times are host wall clock around calls that end in a synchronise (the gather: events), medians of
--reps, profiler off. Kernel times come from a run of its own under rocprofv3 --kernel-trace
(--no-before keeps that run short); --trace-csv folds that run's kernel trace into the JSON, the
gather kernel priced by the copy probe of that same traced run (--trace-json). Writes
profiles/blobs_bench.json.

  python tools/blobs_bench.py [--reps 20] [--out profiles/blobs_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- \
      python tools/blobs_bench.py --no-before --reps 5 --out DIR/other.json
  python tools/blobs_bench.py --trace-csv DIR/.../t_kernel_trace.csv --trace-json DIR/other.json \
      --out profiles/blobs_bench.json
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

FIRST, CONT, SHARE, NS = 478, 482, 512, 29
KERNELS = ("k_bp_classify", "k_bp_sums", "k_bp_scan", "k_bp_compact", "k_bp_cand", "k_bp_status", "k_bp_bsums",
           "k_bp_bscan", "k_bp_bcompact", "k_bp_gather", "k_ns_find", "k_blob_")


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


def blob_square(k, seed):
    """ODS of runs of 1 .. 3k shares, run i under namespace 1000 * (i + 1) and cut into one to four
    blobs whose last share is filled to a random length. -> (ods [k*k][512], runs, blobs)"""
    rng = np.random.default_rng(seed)
    ods = np.zeros((k * k, SHARE), np.uint8)
    at, i, blobs = 0, 0, 0
    while at < k * k:
        r = min(int(rng.integers(1, 3 * k + 1)), k * k - at)
        ns = np.frombuffer(ns_value(1000 * (i + 1)), np.uint8)
        parts = min(int(rng.integers(1, 5)), r)
        cuts = sorted(rng.choice(np.arange(1, r), parts - 1, replace=False).tolist()) if parts > 1 else []
        for a, b in zip([0] + cuts, cuts + [r]):
            n = b - a
            length = FIRST + CONT * (n - 1) - int(rng.integers(0, FIRST if n == 1 else CONT))
            sh = ods[at + a:at + b]
            sh[:, :NS] = ns
            sh[0, NS] = 1
            sh[0, NS + 1:NS + 5] = np.frombuffer(length.to_bytes(4, "big"), np.uint8)
            payload = np.zeros(FIRST + CONT * (n - 1), np.uint8)
            payload[:length] = rng.integers(0, 256, length, dtype=np.uint8)
            sh[0, NS + 5:] = payload[:FIRST]
            if n > 1:
                sh[1:, NS + 1:] = payload[FIRST:].reshape(-1, CONT)
            blobs += 1
        at += r
        i += 1
    return ods, i, blobs


def query_set(n, runs, seed):
    rng = np.random.default_rng(seed)
    half = n // 2
    present = [ns_value(1000 * (int(i) + 1)) for i in rng.integers(0, runs, n - half)]
    absent = [ns_value(1000 * (int(i) + 1) + int(d)) for i, d in zip(rng.integers(0, runs, half), rng.integers(1, 1000, half))]
    qs = present + absent
    return [qs[i] for i in rng.permutation(n)]


def fold_trace(path, out, trace_json):
    """Kernel times of a rocprofv3 --kernel-trace run of this tool into the JSON at `out`: per
    kernel and grid size, count and average; the whole-ODS gather beside the traced run's probe."""
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
    with open(trace_json) as f:
        traced = json.load(f)
    trace = {n: {"dispatches": len(v), "average_us": sum(v) / len(v), "min_us": min(v)} for n, v in sorted(by.items())}
    result["kernel_trace"] = trace
    g = result["gather"]
    ks = trace.get(f"k_bp_gather[grid {g['lanes']}]")
    if ks:
        probe = traced["probe"]["hbm_copy_gbps"]
        g.update(kernel_us=ks["average_us"], kernel_gbps=g["bytes_moved"] / ks["average_us"] / 1e3,
                 traced_run_hbm_copy_gbps=probe, kernel_fraction_of_hbm_copy=g["bytes_moved"] / ks["average_us"] / 1e3 / probe)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(trace, indent=1))
    print("gather", json.dumps(g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--no-before", action="store_true", help="skip the route before (the profiled run)")
    ap.add_argument("--trace-csv", help="fold this kernel trace into --out and stop")
    ap.add_argument("--trace-json", help="the JSON the traced run wrote: its copy probe prices the gather kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blobs_bench.json"))
    args = ap.parse_args()
    if args.trace_csv:
        return fold_trace(args.trace_csv, args.out, args.trace_json)
    k, w = args.k, 2 * args.k

    import torch

    import celestia_eds
    from celestia_eds import blob, da, inclusion, proof

    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ods, runs, nblobs = blob_square(k, 7)
    eds = da._extend(ods, ctx=ctx)
    cells = np.ascontiguousarray(eds.cells)
    index = proof.TreeIndex(eds, ctx=ctx, order_check=True)
    T = index._ptr
    stream = index._stream_ptr()
    dev = index._dev
    result = {"device": ctx.device_name(), "k": k, "reps": args.reps, "runs": runs, "blobs_in_square": nblobs,
              "run_lengths": f"1 .. {3 * k}", "blobs_per_run": "1 .. 4"}
    hc = ctypes.c_double()
    ctx.check(lib.cel_probe_hbm_copy(ctx.handle, 4 << 30, ctypes.byref(hc)))
    result["probe"] = {"hbm_copy_gbps": hc.value}

    def device_route(queries):
        """-> (times, blobs per query as (ns, data, commitment, index))"""
        n = len(queries)
        ns = np.frombuffer(b"".join(queries), np.uint8).copy()
        cap = n * w
        arr = dict(ns_idx=np.zeros(cap, np.uint32), rows=np.zeros(cap, np.uint32), starts=np.zeros(cap, np.int32),
                   ends=np.zeros(cap, np.int32), kinds=np.zeros(cap, np.uint8), leaf_off=np.zeros(cap + 1, np.uint64),
                   node_off=np.zeros(cap + 1, np.uint64))
        cnt, nb, tb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        a, b = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint32)
        st = {}
        with torch.cuda.stream(index._stream):
            d_nswork = torch.empty((lib.cel_dev_namespace_workspace_size(k, n),), dtype=torch.uint8, device=dev)

            def ns_plan():
                ctx.check(lib.cel_dev_namespace_plan(ctx.handle, T(index.d_index), k, n, P(ns), cap, P(arr["ns_idx"]),
                                                     P(arr["rows"]), P(arr["starts"]), P(arr["ends"]), P(arr["kinds"]),
                                                     P(arr["leaf_off"]), P(arr["node_off"]), ctypes.byref(cnt), T(d_nswork),
                                                     stream))
                assert lib.cel_namespace_ods_ranges(k, n, cnt.value, P(arr["ns_idx"]), P(arr["rows"]), P(arr["starts"]),
                                                    P(arr["ends"]), P(arr["kinds"]), P(a), P(b)) == 0

            ns_plan()
            total = int((b.astype(np.int64) - a).sum())
            d_work = torch.empty((lib.cel_dev_blobs_workspace_size(total, n),), dtype=torch.uint8, device=dev)
            recs = (blob.BlobRec * max(total, 1))()

            def blobs_plan():
                ctx.check(lib.cel_dev_blobs_plan(ctx.handle, T(index.d_eds), k, n, P(a), P(b), max(total, 1), recs, P(status),
                                                 ctypes.byref(nb), ctypes.byref(tb), T(d_work), stream))

            blobs_plan()
            m, nbytes = nb.value, tb.value
            shares = sum(recs[i].shares for i in range(m))
            d_data = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            d_com = torch.empty((max(m, 1), 32), dtype=torch.uint8, device=dev)
            d_cwork = torch.empty((lib.cel_dev_commitments_workspace_size(shares, max(m, 1)),), dtype=torch.uint8, device=dev)

            def blobs_emit():
                ctx.check(lib.cel_dev_blobs_emit(ctx.handle, T(index.d_eds), k, m, T(d_data), T(d_com), 64, T(d_work),
                                                 T(d_cwork), stream))
                index._stream.synchronize()

            def route():
                ns_plan()
                blobs_plan()
                blobs_emit()

            st["route_s"] = median_time(route, args.reps)
            st["namespace_plan_s"] = median_time(ns_plan, args.reps)
            st["blobs_plan_s"] = median_time(blobs_plan, args.reps)
            st["blobs_emit_s"] = median_time(blobs_emit, args.reps)
            route()
            data, com = d_data[:nbytes].cpu().numpy(), d_com[:m].cpu().numpy()
        assert not status.any()
        out = [[] for _ in range(n)]
        for i in range(m):
            r = recs[i]
            out[r.range].append((bytes(r.ns)[:NS], data[r.data_off:r.data_off + r.len].tobytes(), com[i].tobytes(), r.start))
        st.update(namespaces=n, blobs=m, blob_bytes=int(sum(recs[i].len for i in range(m))), padded_bytes=nbytes,
                  shares=int(total), device_us=st["route_s"]["median"] * 1e6,
                  namespace_plan_us=st["namespace_plan_s"]["median"] * 1e6,
                  blobs_plan_us=st["blobs_plan_s"]["median"] * 1e6, blobs_emit_us=st["blobs_emit_s"]["median"] * 1e6)
        return st, out

    def host_tail(queries, per_ns_shares):
        """parse_sparse_shares per namespace, then one cel_create_commitments from host memory."""
        parsed = [blob.parse_sparse_shares(sh) if len(sh) else [] for sh in per_ns_shares]
        flat = [(g.namespace, g.data) for p in parsed for g in p]
        com = inclusion.CreateCommitments(flat, ctx=ctx) if flat else []
        it = iter(com)
        return [[(g.namespace, g.data, next(it)) for g in p] for p in parsed]

    def before_host(queries):
        n = len(queries)
        ns = np.frombuffer(b"".join(queries), np.uint8).copy()
        cnt, tl, tn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        ctx.check(lib.cel_namespace_rows(ctx.handle, P(cells), k, n, P(ns), 0, 0, 0, *([None] * 9), ctypes.byref(cnt),
                                         ctypes.byref(tl), ctypes.byref(tn)))
        m = cnt.value
        ns_idx, rows = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
        starts, ends, kinds = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.uint8)
        leaf_off, node_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
        leaves, nodes = np.zeros((max(tl.value, 1), SHARE), np.uint8), np.zeros((max(tn.value, 1), 90), np.uint8)
        ctx.check(lib.cel_namespace_rows(ctx.handle, P(cells), k, n, P(ns), m, tl.value, tn.value, P(ns_idx), P(rows),
                                         P(starts), P(ends), P(kinds), P(leaf_off), P(node_off), P(leaves), P(nodes),
                                         ctypes.byref(cnt), ctypes.byref(tl), ctypes.byref(tn)))
        per = [[] for _ in range(n)]
        for e in range(m):
            per[ns_idx[e]].append(leaves[int(leaf_off[e]):int(leaf_off[e + 1])])
        return host_tail(queries, [np.concatenate(p) if p else np.zeros((0, SHARE), np.uint8) for p in per])

    def before_resident(queries):
        f = index.namespace_flat(queries)
        per = [[] for _ in queries]
        for e in range(len(f["rows"])):
            per[int(f["ns_idx"][e])].append(f["leaves"][int(f["leaf_off"][e]):int(f["leaf_off"][e + 1])])
        return host_tail(queries, [np.concatenate(p) if p else np.zeros((0, SHARE), np.uint8) for p in per])

    result["queries"] = {}
    for n in (1, 64, 1024):
        queries = query_set(n, runs, 100 + n)
        st, ours = device_route(queries)
        if args.no_before:
            result["queries"][str(n)] = st
            continue
        want = before_host(queries)
        assert [[x[:3] for x in o] for o in ours] == want, "the two routes differ"
        assert before_resident(queries) == want
        preps = args.reps
        tb = median_time(lambda: before_host(queries), preps)
        tr = median_time(lambda: before_resident(queries), preps)
        st["before"] = {"s": tb, "reps": preps, "us": tb["median"] * 1e6,
                        "route": "cel_namespace_rows + blob.parse_sparse_shares + cel_create_commitments",
                        "speedup": tb["median"] / st["route_s"]["median"]}
        st["before_resident"] = {"s": tr, "reps": preps, "us": tr["median"] * 1e6,
                                 "route": "TreeIndex.namespace_flat + blob.parse_sparse_shares + cel_create_commitments",
                                 "speedup": tr["median"] / st["route_s"]["median"]}
        result["queries"][str(n)] = st
        print("queries", n, json.dumps(st), flush=True)

    # ---- the gather kernel alone: the whole ODS as one range
    a, b = np.zeros(1, np.uint32), np.full(1, k * k, np.uint32)
    nb, tb = ctypes.c_uint64(), ctypes.c_uint64()
    with torch.cuda.stream(index._stream):
        d_work = torch.empty((lib.cel_dev_blobs_workspace_size(k * k, 1),), dtype=torch.uint8, device=dev)
        ctx.check(lib.cel_dev_blobs_plan(ctx.handle, T(index.d_eds), k, 1, P(a), P(b), 0, None, None, ctypes.byref(nb),
                                         ctypes.byref(tb), T(d_work), stream))
        assert nb.value == nblobs
        d_data = torch.empty((tb.value,), dtype=torch.uint8, device=dev)
        inner, ts = 10, []
        for rep in range(args.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(index._stream)
            for _ in range(inner):
                ctx.check(lib.cel_dev_blobs_emit(ctx.handle, T(index.d_eds), k, nb.value, T(d_data), None, 64, T(d_work), None,
                                                 stream))
            e1.record(index._stream)
            index._stream.synchronize()
            if rep >= 2:
                ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    ts.sort()
    us = ts[len(ts) // 2]
    moved = 2 * tb.value
    result["gather"] = {"blobs": nb.value, "padded_bytes": tb.value, "bytes_moved": moved,
                        "lanes": (tb.value // 16 + 255) // 256 * 256, "us": us, "min_us": ts[0],
                        "max_us": ts[-1], "gbps": moved / us / 1e3, "fraction_of_hbm_copy": moved / us / 1e3 / hc.value,
                        "method": f"{inner} emit calls without commitments between two events, elapsed / {inner}; "
                                  "bytes: each blob's padded length once read, once written"}
    print("gather", json.dumps(result["gather"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
