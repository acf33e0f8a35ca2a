"""Rate of the batched NMT proof verifier on the sampling shape: a k = 128 square, one cell
sample with a single-leaf proof (8 nodes) per cell of the p = 0.55, seed-7 mask (about 36K
samples, alternating between row-root and column-root proofs), 33 SHA-256 compressions per
sample (9 for the 542-byte leaf, 8 x 3 for the path).

  verify_dev      cel_dev_nmt_verify_batch on device-resident leaves, nodes and roots
  stages          the same call with CEL_VERIFY_STAGES = 0 (table fill and upload only), 1
                  (repack), 2 (leaves), 4 (fold); a stage's device time is its call minus the
                  call without kernels
  repair_samples  cel_repair_samples (verify, place, repair) beside cel_repair on the same
                  mask in the same process
  host_mirror     NMTProof.VerifyInclusion of celestia_eds/proof.py for the same samples on
                  one core: Python + hashlib, not a tuned host verifier

Times are host wall clock around calls that end in a device synchronise, medians of --reps;
the compression rate is set beside the same run's cel_probe_sha256. Writes
profiles/verify_bench.json.

  python tools/verify_bench.py [--reps 20] [--out profiles/verify_bench.json]
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
from celestia_eds import da, proof  # noqa: E402
from celestia_eds.testfactory import random_ods  # noqa: E402

COMPRESSIONS = 9 + 8 * 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    args = ap.parse_args()
    k, w = args.k, 2 * args.k

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

    def upload(a):
        d = dmalloc(a.nbytes)
        assert hip.hipMemcpy(d, P(a), a.nbytes, 1) == 0
        return d

    def probe():
        g, mhz = ctypes.c_double(), ctypes.c_double()
        ctx.check(lib.cel_probe_sha256(ctx.handle, ctypes.byref(g), ctypes.byref(mhz)))
        return g.value, mhz.value

    # the square, its trees, the samples
    eds = da._extend(random_ods(k, 7).reshape(-1, 512), ctx=ctx)
    cells = np.ascontiguousarray(eds.cells)
    trees = [proof.axis_trees(eds, axis, 0, w) for axis in (0, 1)]
    rr, cr = np.ascontiguousarray(trees[0][:, -1]), np.ascontiguousarray(trees[1][:, -1])
    present = (np.random.default_rng(7).random((w, w)) < 0.55).astype(np.uint8)
    coords = [(int(r), int(c)) for r, c in zip(*np.nonzero(present))]
    n = len(coords)
    rows = np.array([r for r, _ in coords], np.uint32)
    cols = np.array([c for _, c in coords], np.uint32)
    axes = (np.arange(n) % 2).astype(np.uint8)
    shares = np.ascontiguousarray(cells[rows, cols])
    node_lists = [proof.nmt_prove_range(trees[a][c if a else r], r if a else c, (r if a else c) + 1)
                  for (r, c), a in zip(coords, axes)]
    nodes = np.frombuffer(b"".join(x for nl in node_lists for x in nl), np.uint8).copy()
    node_off = np.cumsum([0] + [len(nl) for nl in node_lists]).astype(np.uint64)
    assert int(node_off[-1]) == 8 * n or k != 128
    starts = np.where(axes == 1, rows, cols).astype(np.int32)
    ends = starts + 1
    ns = np.full((n, 29), 0xFF, np.uint8)
    q0 = (rows < k) & (cols < k)
    ns[q0] = shares[q0, :29]
    leaf_off = np.arange(n + 1, dtype=np.uint64)
    roots = np.concatenate([rr, cr])
    root_idx = np.where(axes == 1, w + cols, rows).astype(np.uint32)

    d_leaves, d_nodes, d_roots, d_ok = upload(shares), upload(nodes), upload(roots), dmalloc(n)
    d_work = dmalloc(lib.cel_dev_nmt_verify_workspace_size(n, int(node_off[-1]), n))

    def verify_dev():
        ctx.check(lib.cel_dev_nmt_verify_batch(ctx.handle, n, P(starts), P(ends), P(ns), d_leaves, P(leaf_off), d_nodes,
                                               P(node_off), d_roots, 2 * w, P(root_idx), d_ok, d_work, None))
        assert hip.hipDeviceSynchronize() == 0

    comp = COMPRESSIONS * n if k == 128 else None
    result = {"device": ctx.device_name(), "k": k, "samples": n, "reps": args.reps,
              "compressions_per_sample": COMPRESSIONS if k == 128 else None}
    peak, mhz = probe()
    t = median_time(verify_dev, args.reps)
    ok = np.zeros(n, np.uint8)
    assert hip.hipMemcpy(P(ok), d_ok, n, 2) == 0 and ok.all(), "a genuine sample was rejected"
    result["verify_dev"] = {"s": t, "us": t["median"] * 1e6, "samples_per_s": n / t["median"],
                            "probe_gcompressions_per_s": peak, "probe_shader_mhz": mhz}
    if comp:
        g = comp / t["median"] / 1e9
        result["verify_dev"].update({"gcompressions_per_s": g, "fraction_of_probe": g / peak})
    print("verify_dev", json.dumps(result["verify_dev"]), flush=True)

    # the stages apart: the workspace keeps the records the full runs above left in it
    stage_t = {}
    for name, mask in (("none", 0), ("repack", 1), ("leaves", 2), ("fold", 4)):
        os.environ["CEL_VERIFY_STAGES"] = str(mask)
        stage_t[name] = median_time(verify_dev, args.reps)
    del os.environ["CEL_VERIFY_STAGES"]
    base = stage_t["none"]["median"]
    result["stages"] = {"call_without_kernels_us": base * 1e6}
    for name, c in (("repack", 0), ("leaves", 9), ("fold", 24)):
        dt = max(stage_t[name]["median"] - base, 1e-9)
        result["stages"][name] = {"call_us": stage_t[name]["median"] * 1e6, "device_us": dt * 1e6}
        if c and k == 128:
            g = c * n / dt / 1e9
            result["stages"][name].update({"gcompressions_per_s": g, "fraction_of_probe": g / peak})
    print("stages", json.dumps(result["stages"]), flush=True)

    # samples -> repaired square, beside the repair alone
    damaged = cells.copy()
    damaged[present == 0] = 0
    rrb, crb = rr.copy(), cr.copy()
    out, mask_out, okh = np.zeros_like(cells), np.zeros((w, w), np.uint8), np.zeros(n, np.uint8)
    ba, bi = ctypes.c_int32(), ctypes.c_int32()

    def repair_samples():
        ctx.check(lib.cel_repair_samples(ctx.handle, k, P(rrb), P(crb), n, P(rows), P(cols), P(axes), P(shares), P(nodes),
                                         P(node_off), P(okh), P(out), P(mask_out), ctypes.byref(ba), ctypes.byref(bi),
                                         None, None))

    work, mask_in = damaged.copy(), present.copy()

    def repair_only():
        work[:] = damaged
        mask_in[:] = present
        ctx.check(lib.cel_repair(ctx.handle, P(work), P(mask_in), k, 512, P(rrb), P(crb), ctypes.byref(ba),
                                 ctypes.byref(bi), None, None))

    def reset_only():
        work[:] = damaged
        mask_in[:] = present

    t0 = median_time(reset_only, args.reps)
    ts, tr = median_time(repair_samples, args.reps), median_time(repair_only, args.reps)
    assert np.array_equal(out, cells) and np.array_equal(work, cells) and okh.all()
    result["repair_samples"] = {"cel_repair_samples_s": ts, "cel_repair_s": tr,
                                "cel_repair_input_reset_s": t0,
                                "note": "cel_repair's figure includes restoring its 32 MiB input in place "
                                        "(cel_repair_input_reset_s); both entries take pageable host memory"}
    print("repair_samples", json.dumps(result["repair_samples"]), flush=True)

    # the host mirror on one core
    plist = [proof.NMTProof(Start=int(s), End=int(s) + 1, Nodes=nl) for s, nl in zip(starts, node_lists)]
    nsb = [r.tobytes() for r in ns]
    shb = [[r.tobytes()] for r in shares]
    rtb = [roots[i].tobytes() for i in root_idx]

    def mirror():
        assert all(p.VerifyInclusion(a, b, c) for p, a, b, c in zip(plist, nsb, shb, rtb))

    tm = median_time(mirror, args.reps)
    result["host_mirror"] = {"s": tm, "samples_per_s": n / tm["median"],
                             "what": "celestia_eds.proof.NMTProof.VerifyInclusion, Python + hashlib, one core"}
    if comp:
        result["host_mirror"]["gcompressions_per_s"] = comp / tm["median"] / 1e9
    print("host_mirror", json.dumps(result["host_mirror"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
