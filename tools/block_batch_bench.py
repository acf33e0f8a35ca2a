"""cel_block_extend_batch (a range of blocks' txs in, every data root and commitment out, one
call) against the same blocks through cel_block_extend one after another, in the same process,
on the same page-locked txs, alternating:

  loop    cel_block_extend per block, commitments requested, eds_out = NULL; timed as two
          interleaved series (A before the batch call, B after it): the difference of their
          medians is the margin below which a difference to the batch means nothing
  batch   cel_block_extend_batch, commitments requested, host_threads = 16 (and 1); its phase
          times (host layout wall time, device time between events) at host_threads 1 and 16
          come from the same calls, which create and record two timing events each

Workloads:

  b408x256      256 copies of block 408 (k = 32)
  mixed256      256 blocks of mixed widths k = 1 .. 64 from tests/square_inputs.random_block,
                parameters drawn with a fixed seed (the width histogram is recorded)
  full128xN     N = 1, 2, 4, 16, 64 copies of block_bench.py's full k = 128 block (pfb_mix)

Every shape is warmed (three rounds of both variants) and both variants' outputs are compared
before timing. Times are host wall clock around calls that end in a device synchronise; medians
of --reps rounds (default 20). Each workload runs in a child process of its own under a time
limit; the parent never opens the device and stops at the first child that fails. Writes
profiles/block_batch_bench.json.

  python tools/block_batch_bench.py [--reps 20] [--out profiles/block_batch_bench.json] [--workloads a,b]
  python tools/block_batch_bench.py --trace NAME    # a few batch calls and the copy probe, for
                                                    # rocprofv3 --kernel-trace (tools/ktrace.py)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = ["b408x256", "mixed256", "full128x1", "full128x2", "full128x4", "full128x16", "full128x64"]
CHILD_LIMIT_S = 420
THREADS = 16  # never from the machine's CPU count: a GPU machine grants 16 and reports many more


def blocks_of(name):
    """-> (blocks: a list of tx lists, max_square_size)"""
    import block_inputs as B
    from square_inputs import block408_txs, random_block
    if name == "b408x256":
        return [block408_txs()] * 256, 128
    if name == "mixed256":
        rng = np.random.default_rng(408)
        out = []
        for i in range(256):
            n_blob = int(rng.choice([0, 0, 1, 2, 4, 8, 20, 60]))
            out.append(random_block(1000 + i, int(rng.integers(0, 7)), n_blob, max_blob=int(rng.choice([800, 6000, 12000]))))
        return out, 128
    assert name.startswith("full128x")
    from block_bench import candidates
    cand, max_sq = candidates(np.random.default_rng(11))["pfb_mix"]
    included = B.layout(cand, max_sq, 64, 1)[3]
    txs = [t for t, s in zip(cand, included) if s == 1] + [t for t, s in zip(cand, included) if s == 2]
    return [txs] * int(name[len("full128x"):]), max_sq


def med(ts):
    a = np.sort(np.asarray(ts, np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1])}


def run_workload(name, reps, trace=False):
    import celestia_eds
    ctx = celestia_eds.default_context(0)
    lib = ctx.lib
    lib.cel_host_alloc.restype = ctypes.c_void_p
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    blocks, max_sq = blocks_of(name)
    n = len(blocks)
    flat = [t for b in blocks for t in b]
    raw = b"".join(flat)
    lens = np.array([len(t) for t in flat] + [0], np.uint32)
    nt = np.array([len(b) for b in blocks], np.uint32)
    tx0 = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))])[tx0]
    hp = lib.cel_host_alloc(max(len(raw), 1))
    assert hp, "cel_host_alloc failed"
    np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_uint8)), (max(len(raw), 1),))[:len(raw)] = \
        np.frombuffer(raw, np.uint8)
    c = ctypes.c_uint32()
    ctx.check(lib.cel_blob_tx_commitments(ctx.handle, hp, P(lens), len(flat), 64, None, None, 0, ctypes.byref(c)))
    nb = max(c.value, 1)
    cap = n * 2 * max_sq
    k_b, st_b, off_b = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n + 1, np.uint32)
    rr_b, cr_b, dah_b = np.zeros((cap, 90), np.uint8), np.zeros((cap, 90), np.uint8), np.zeros((n, 32), np.uint8)
    com_b, cb_b, ct_b = np.zeros((nb, 32), np.uint8), np.zeros(nb, np.uint32), np.zeros(nb, np.uint32)
    k_a = np.zeros(n, np.uint32)
    rr_a, cr_a, dah_a = np.zeros((n, 2 * max_sq, 90), np.uint8), np.zeros((n, 2 * max_sq, 90), np.uint8), np.zeros((n, 32), np.uint8)
    com_a, ct_a, nc_a = np.zeros((nb, 32), np.uint8), np.zeros(nb, np.uint32), np.zeros(n, np.uint32)
    ncom, kk = ctypes.c_uint32(), ctypes.c_uint32()
    phase = np.zeros(2, np.float32)

    def loop():
        t0 = time.perf_counter()
        at = 0
        for i in range(n):
            ctx.check(lib.cel_block_extend(ctx.handle, ctypes.c_void_p(hp + int(boff[i])), P(lens[tx0[i]:]), int(nt[i]),
                                           max_sq, 64, 0, ctypes.byref(kk), None, P(rr_a[i]), P(cr_a[i]), P(dah_a[i]),
                                           None, 0, P(com_a[at:]), P(ct_a[at:]), nb - at, ctypes.byref(ncom), 1))
            k_a[i], nc_a[i] = kk.value, ncom.value
            at += ncom.value
        return time.perf_counter() - t0

    def batch(threads=THREADS):
        t0 = time.perf_counter()
        ctx.check(lib.cel_block_extend_batch(ctx.handle, hp, P(lens), P(nt), n, max_sq, 64, 0, threads, 0, P(k_b), P(st_b),
                                             None, P(rr_b), P(cr_b), P(off_b), cap, P(dah_b), P(com_b), P(cb_b), P(ct_b),
                                             nb, ctypes.byref(ncom), P(phase), 1))
        return time.perf_counter() - t0, float(phase[0]) * 1e-3, float(phase[1]) * 1e-3

    if trace:
        for _ in range(6):
            batch()
        gbps = ctypes.c_double()
        eds_q0 = int(sum(int(k) ** 2 for k in k_b)) * 512
        ctx.check(lib.cel_probe_hbm_copy(ctx.handle, 2 * eds_q0, ctypes.byref(gbps)))
        print(json.dumps({"workload": name, "blocks": n, "q0_bytes_written": eds_q0, "probe_bytes_moved": 2 * eds_q0,
                          "probe_hbm_copy_gbps": gbps.value}), flush=True)
        return None

    for _ in range(3):  # warm-up: scratch and staging grow on the first calls
        loop(), batch(), batch(1)
    assert np.array_equal(k_a, k_b) and np.array_equal(dah_a, dah_b), "paths disagree"
    assert np.array_equal(com_a[:ncom.value], com_b[:ncom.value]) and np.array_equal(ct_a[:ncom.value], ct_b[:ncom.value])
    for i in range(n):
        k2 = 2 * int(k_a[i])
        assert np.array_equal(rr_a[i, :k2], rr_b[off_b[i]:off_b[i] + k2]) and np.array_equal(cr_a[i, :k2], cr_b[off_b[i]:off_b[i] + k2])
    la, lb, bt, b1 = [], [], [], []
    for _ in range(reps):
        la.append(loop())
        bt.append(batch())
        lb.append(loop())
        b1.append(batch(1))
    bt, b1 = np.array(bt), np.array(b1)
    A, Bs, T = med(la), med(lb), med(bt[:, 0])
    loop_med = 0.5 * (A["median"] + Bs["median"])
    margin = abs(A["median"] - Bs["median"])
    ks, counts = np.unique(k_a, return_counts=True)
    out = {
        "blocks": n, "max_square_size": max_sq, "txs": len(flat), "tx_bytes": len(raw), "blobs": int(ncom.value),
        "widths": {str(int(k)): int(c) for k, c in zip(ks, counts)},
        "loop_a_s": A, "loop_b_s": Bs, "loop_margin_s": margin,
        "batch_s": T, "batch_host_threads_1_s": med(b1[:, 0]),
        "loop_blocks_per_s": n / loop_med, "batch_blocks_per_s": n / T["median"],
        "batch_over_loop": loop_med / T["median"],
        "batch_beats_loop_by_more_than_margin": bool(loop_med - T["median"] > margin),
        "batch_within_margin_of_loop": bool(abs(loop_med - T["median"]) <= margin),
        "host_layout_s": {"threads_16": med(bt[:, 1])["median"], "threads_1": med(b1[:, 1])["median"]},
        "device_s": {"threads_16": med(bt[:, 2])["median"], "threads_1": med(b1[:, 2])["median"]},
    }
    lib.cel_host_free(ctypes.c_void_p(hp))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_batch_bench.json"))
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--child", help="run one workload in this process and print its JSON line")
    ap.add_argument("--trace", help="a few batch calls of one workload and the copy probe, nothing timed")
    args = ap.parse_args()
    if args.trace:
        run_workload(args.trace, 0, trace=True)
        return 0
    if args.child:
        print("RESULT " + json.dumps(run_workload(args.child, args.reps)), flush=True)
        return 0
    result = {"reps": args.reps, "threshold": 64, "host_threads": THREADS, "workloads": {}}
    for name in args.workloads.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CHILD_LIMIT_S} s; stopping", flush=True)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"{name}: exit {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        result["workloads"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, lines[-1][len("RESULT "):], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
