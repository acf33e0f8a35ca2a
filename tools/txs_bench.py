"""Times of txs out of a resident square, on two squares: a k = 128 square whose ODS is one tx
stream (16384 compact shares, units of 1 .. 2000 bytes) and mainnet block 408 (k = 32, its tx
and PayForBlob runs as two ranges).

  device   the square resident: cel_dev_txs_plan, cel_dev_txs_emit with hashes, a stream
           synchronise. Nothing but the counts, statuses and flags crosses PCIe; txs_plan_us and
           txs_emit_us are the two calls alone.
  before   the route to the same answers before this: a download of the ranges' shares,
           square.parse_compact_shares over each range on the host, hashlib.sha256 of every unit.
  gather   k_tx_gather beside k_bp_gather on equal bytes: the k = 128 tx square and a k = 128
           square of blobs (blobs_bench.blob_square), each gathered as one range, priced from a
           kernel trace run of its own by the bytes they write and read (twice the padded bytes).

Both routes run in this process on the same square, and their units and hashes must be equal.
Times are host wall clock around calls that end in a synchronise, medians of --reps, profiler off.
Kernel times come from a run of its own under rocprofv3 --kernel-trace (--no-before keeps that
run short); --trace-csv folds that run's kernel trace into the JSON. Writes
profiles/txs_bench.json.

  python tools/txs_bench.py [--reps 20] [--out profiles/txs_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- \
      python tools/txs_bench.py --no-before --reps 5 --out DIR/other.json
  python tools/txs_bench.py --trace-csv DIR/.../t_kernel_trace.csv --trace-json DIR/other.json \
      --out profiles/txs_bench.json
"""
import argparse
import csv
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blobs_bench import blob_square, median_time  # noqa: E402

SHARE, NS = 512, 29
KERNELS = ("k_tx_classify", "k_tx_sums", "k_tx_scan", "k_tx_bases", "k_tx_status", "k_tx_walk", "k_tx_link",
           "k_tx_resolve", "k_tx_usums", "k_tx_uscan", "k_tx_ubases", "k_tx_records", "k_tx_gather", "k_tx_hash",
           "k_bp_gather")


def uvarint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def tx_square(k, seed):
    """A k*k ODS that is one sequence of the tx namespace, as square.cpp's write_compact lays it
    out, filled to its last share. -> (ods [k*k][512], units)"""
    rng = np.random.default_rng(seed)
    room = 474 + 478 * (k * k - 1)
    units, starts, used = [], [], 0
    while True:
        n = int(rng.integers(1, 2001))
        if used + len(uvarint(n)) + n > room:
            break
        starts.append(used)
        units.append(rng.integers(0, 256, n, np.uint8).tobytes())
        used += len(uvarint(n)) + n
    stream = np.zeros(room, np.uint8)
    stream[:used] = np.frombuffer(b"".join(uvarint(len(u)) + u for u in units), np.uint8)
    ods = np.zeros((k * k, SHARE), np.uint8)
    ods[:, NS - 1] = 1
    ods[0, NS] = 1
    ods[0, NS + 1:NS + 5] = np.frombuffer(used.to_bytes(4, "big"), np.uint8)
    ods[0, 38:] = stream[:474]
    ods[1:, 34:] = stream[474:].reshape(-1, 478)
    base = np.concatenate(([0], 474 + 478 * np.arange(k * k - 1)))  # each share's first stream byte
    first = np.searchsorted(np.array(starts), base)  # the first unit at or behind it
    for j in range(k * k):
        h = 38 if j == 0 else 34
        end = base[j] + 512 - h
        r = h + starts[first[j]] - base[j] if first[j] < len(starts) and starts[first[j]] < end else 0
        ods[j, h - 4:h] = np.frombuffer(int(r).to_bytes(4, "big"), np.uint8)
    return ods, units


def fold_trace(path, out, trace_json):
    """Kernel times of a rocprofv3 --kernel-trace run of this tool into the JSON at `out`: per
    kernel and grid size, count and average; the two gather kernels by their bytes."""
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
    g = result["gather"] = traced["gather"]
    for name, kernel in (("txs", "k_tx_gather"), ("blobs", "k_bp_gather")):
        ks = trace.get(f"{kernel}[grid {g[name]['lanes']}]")
        if ks:
            g[name].update(kernel=kernel, kernel_us=ks["average_us"], kernel_gbps=g[name]["bytes_moved"] / ks["average_us"] / 1e3)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(trace, indent=1))
    print("gather", json.dumps(g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-before", action="store_true", help="skip the route before (the profiled run)")
    ap.add_argument("--trace-csv", help="fold this kernel trace into --out and stop")
    ap.add_argument("--trace-json", help="the JSON the traced run wrote: it holds the gathers' bytes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txs_bench.json"))
    args = ap.parse_args()
    if args.trace_csv:
        return fold_trace(args.trace_csv, args.out, args.trace_json)

    import torch

    import celestia_eds
    import square_inputs as SI
    from celestia_eds import blob, block, da, proof, square

    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    result = {"device": ctx.device_name(), "reps": args.reps, "cases": {}}

    def measure(index, ranges):
        """-> (times, units per range, hashes per range) of the device route."""
        k, T, stream, dev = index.k, index._ptr, index._stream_ptr(), index._dev
        n = len(ranges)
        a, b = np.array([r[0] for r in ranges], np.uint32), np.array([r[1] for r in ranges], np.uint32)
        total = int(sum(y - x for x, y in ranges))
        status, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        nu, tb = ctypes.c_uint64(), ctypes.c_uint64()
        st = {}
        with torch.cuda.stream(index._stream):
            d_work = torch.empty((lib.cel_dev_txs_workspace_size(total, n),), dtype=torch.uint8, device=dev)

            def plan():
                ctx.check(lib.cel_dev_txs_plan(ctx.handle, T(index.d_eds), k, n, P(a), P(b), P(status), P(flags),
                                               ctypes.byref(nu), ctypes.byref(tb), T(d_work), stream))

            plan()
            m, nbytes = nu.value, tb.value
            d_recs = torch.empty((max(m, 1) * 32,), dtype=torch.uint8, device=dev)
            d_data = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            d_hash = torch.empty((max(m, 1), 32), dtype=torch.uint8, device=dev)

            def emit(hashes=True):
                ctx.check(lib.cel_dev_txs_emit(ctx.handle, T(index.d_eds), k, m, T(d_recs), T(d_data),
                                               T(d_hash) if hashes else None, T(d_work), stream))
                index._stream.synchronize()

            def route():
                plan()
                emit()

            st["route_s"] = median_time(route, args.reps)
            st["txs_plan_s"] = median_time(plan, args.reps)
            st["txs_emit_s"] = median_time(emit, args.reps)
            st["txs_emit_no_hashes_s"] = median_time(lambda: emit(False), args.reps)
            route()
            recs = (square.TxRec * m).from_buffer_copy(d_recs.cpu().numpy().tobytes()[:32 * m])
            data, hs = d_data[:nbytes].cpu().numpy(), d_hash[:m].cpu().numpy()
        assert not status.any() and not flags.any()
        units, hashes = [[] for _ in ranges], [[] for _ in ranges]
        for i, r in enumerate(recs):
            units[r.range].append(data[r.data_off:r.data_off + r.len].tobytes())
            hashes[r.range].append(hs[i].tobytes())
        st.update(ranges=n, shares=total, units=m, unit_bytes=int(sum(r.len for r in recs)), padded_bytes=nbytes,
                  device_us=st["route_s"]["median"] * 1e6, txs_plan_us=st["txs_plan_s"]["median"] * 1e6,
                  txs_emit_us=st["txs_emit_s"]["median"] * 1e6,
                  txs_emit_no_hashes_us=st["txs_emit_no_hashes_s"]["median"] * 1e6,
                  lanes=(nbytes // 16 + 255) // 256 * 256)
        return st, units, hashes

    def before(index, ranges):
        k = index.k
        with torch.cuda.stream(index._stream):
            q0 = index.d_eds[:k, :k].reshape(k * k, SHARE)
            shares = [q0[a:b].cpu().numpy() for a, b in ranges]
        units = [square.parse_compact_shares(sh) for sh in shares]
        return units, [[hashlib.sha256(u).digest() for u in us] for us in units]

    def case(name, index, ranges):
        st, units, hashes = measure(index, ranges)
        if not args.no_before:
            assert before(index, ranges) == (units, hashes), "the two routes differ"
            t = median_time(lambda: before(index, ranges), args.reps)
            st["before"] = {"s": t, "us": t["median"] * 1e6, "speedup": t["median"] / st["route_s"]["median"],
                            "route": "download of the shares + square.parse_compact_shares + hashlib.sha256"}
        result["cases"][name] = st
        print(name, json.dumps(st), flush=True)
        return st

    k = 128
    ods, units = tx_square(k, 11)
    index = proof.TreeIndex(da._extend(ods, ctx=ctx), ctx=ctx)
    full = case("k128_full_of_compact_shares", index, [(0, k * k)])
    assert full["units"] == len(units)

    txs = SI.block408_txs()
    b = block.block_extend(ctx, txs, want_eds=True)
    index408 = proof.TreeIndex(b.eds, ctx=ctx)
    runs = blob.ods_ranges(index408.k, 2, index408.namespace_flat([square.TX_NAMESPACE, square.PFB_NAMESPACE]))
    case("block408", index408, runs)

    # ---- the two gather kernels on equal bytes, for the kernel trace: each square as one range
    bods, _, nblobs = blob_square(k, 7)
    bindex = proof.TreeIndex(da._extend(bods, ctx=ctx), ctx=ctx, order_check=True)
    a, e = np.zeros(1, np.uint32), np.full(1, k * k, np.uint32)
    nb, tb = ctypes.c_uint64(), ctypes.c_uint64()
    with torch.cuda.stream(bindex._stream):
        d_work = torch.empty((lib.cel_dev_blobs_workspace_size(k * k, 1),), dtype=torch.uint8, device=bindex._dev)
        ctx.check(lib.cel_dev_blobs_plan(ctx.handle, bindex._ptr(bindex.d_eds), k, 1, P(a), P(e), 0, None, None,
                                         ctypes.byref(nb), ctypes.byref(tb), bindex._ptr(d_work), bindex._stream_ptr()))
        d_data = torch.empty((tb.value,), dtype=torch.uint8, device=bindex._dev)
        for _ in range(args.reps):
            ctx.check(lib.cel_dev_blobs_emit(ctx.handle, bindex._ptr(bindex.d_eds), k, nb.value, bindex._ptr(d_data), None,
                                             64, bindex._ptr(d_work), None, bindex._stream_ptr()))
        bindex._stream.synchronize()
    result["gather"] = {
        "txs": {"units": full["units"], "padded_bytes": full["padded_bytes"], "bytes_moved": 2 * full["padded_bytes"],
                "lanes": full["lanes"]},
        "blobs": {"blobs": nb.value, "padded_bytes": tb.value, "bytes_moved": 2 * tb.value,
                  "lanes": (tb.value // 16 + 255) // 256 * 256},
        "method": "kernel times from the kernel trace; bytes: each unit's or blob's padded length once read, once written"}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
