"""Batch repair against one repair per square, same process, same squares.

  python tools/repair_batch_bench.py [--out profiles/repair_batch_bench.json]
  python tools/repair_batch_bench.py --trace N            # one shape, for a kernel trace
  python tools/repair_batch_bench.py --kernel-times STATS.csv --trace-json T.json --out-txt FILE

Default run. k = 128 squares, each a distinct random ODS extended on the device; two masks:
p = 0.55 with seed 7 (bench.py --mode repair's) and Q0 only; n = 1, 2, 4, 16, 64; and k = 32 at
n = 256 (p = 0.55). For each shape, alternating in one loop: a fresh damaged copy (device to
device, outside the clock), cel_dev_repair_batch under a host clock; a fresh copy, n sequential
cel_dev_repair calls under a host clock (the path a caller had before the batch call), twice,
so the two sequential series give the same-run spread. Every shape is warmed up; medians of
--reps (20). The host planner alone (cel_debug_repair_batch_plan over the n masks, host clock)
and the HBM copy probe of the same run are recorded beside them. The repaired bytes of every
p = 0.55 batch are compared with the original squares on the device.

--trace N runs the k = 128, p = 0.55 batch of N squares a few times and nothing else, for
`rocprofv3 --kernel-trace --stats`; it writes the decode launches' algorithmic bytes (every
shard of every decoded axis read once, every missing shard written once, as bench.py counts
them) and the copy probe's GB/s as JSON. --kernel-times turns that trace's kernel stats and
those JSON files into the text table of time per decode, check and commit launch, with the
decode kernel's bytes over its time as a fraction of the probe."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

P = lambda x: x.ctypes.data_as(ctypes.c_void_p)


def _squares(ctx, k, n):
    """n distinct squares extended on the device: (torch uint8 [n, W, W, 512] on the GPU, row
    roots [n, W, 90], column roots)."""
    import numpy as np
    import torch
    from celestia_eds import da
    from celestia_eds.testfactory import random_ods
    w = 2 * k
    d = torch.empty((n, w, w, 512), dtype=torch.uint8, device="cuda")
    rr, cr = np.zeros((n, w, 90), np.uint8), np.zeros((n, w, 90), np.uint8)
    for i in range(n):
        eds = da._extend(random_ods(k, 1000 + i).reshape(-1, 512), ctx=ctx)
        d[i].copy_(torch.from_numpy(np.ascontiguousarray(eds.cells)))
        rr[i], cr[i] = eds._row_roots, eds._col_roots
    return d, rr, cr


def _mask(kind, k):
    import numpy as np
    w = 2 * k
    if kind == "p055":
        return (np.random.default_rng(7).random((w, w)) < 0.55).astype(np.uint8)
    m = np.zeros((w, w), np.uint8)
    m[:k, :k] = 1
    return m


class Shape:
    """n squares of one k under one mask: the damaged originals and a working copy."""

    def __init__(self, ctx, pristine, rr, cr, kind, k, n):
        import numpy as np
        import torch
        self.ctx, self.k, self.n, self.kind = ctx, k, n, kind
        self.mask = _mask(kind, k)
        self.pristine = pristine[:n]
        keep = torch.from_numpy(self.mask).cuda()[None, :, :, None]
        self.damaged = self.pristine * keep
        self.work = torch.empty_like(self.damaged)
        self.rr, self.cr = np.ascontiguousarray(rr[:n]), np.ascontiguousarray(cr[:n])
        self.status = np.zeros(n, np.int32)
        self.sq_bytes = self.work[0].numel()

    def fresh(self):
        import numpy as np
        import torch
        self.work.copy_(self.damaged)
        torch.cuda.synchronize()
        return np.ascontiguousarray(np.broadcast_to(self.mask, (self.n,) + self.mask.shape)).copy()

    def batch(self, pres):
        lib, ctx = self.ctx.lib, self.ctx
        ctx.check(lib.cel_dev_repair_batch(ctx.handle, ctypes.c_void_p(self.work.data_ptr()), P(pres), self.n, self.k,
                                           P(self.rr), P(self.cr), P(self.status), None, None, None, None))
        assert (self.status == 0).all(), self.status

    def sequential(self, pres):
        lib, ctx = self.ctx.lib, self.ctx
        base = self.work.data_ptr()
        for i in range(self.n):
            ctx.check(lib.cel_dev_repair(ctx.handle, ctypes.c_void_p(base + i * self.sq_bytes), P(pres[i]), self.k,
                                         P(self.rr[i]), P(self.cr[i]), None, None, None, None))

    def timed(self, f):
        pres = self.fresh()
        t0 = time.perf_counter()
        f(pres)
        return time.perf_counter() - t0

    def plan_seconds(self, reps):
        """The host planner alone over the n masks (merged passes, checks, solve logs)."""
        import numpy as np
        lib, k, n = self.ctx.lib, self.k, self.n
        m = np.ascontiguousarray(np.broadcast_to(self.mask, (n,) + self.mask.shape)).copy()
        dirs, off = np.zeros(8 * k, np.int32), np.zeros(8 * k + 1, np.uint32)
        sq, ax = np.zeros(n * 4 * k, np.uint32), np.zeros(n * 4 * k, np.int32)
        npass = ctypes.c_uint32(0)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            assert lib.cel_debug_repair_batch_plan(P(m), n, k, P(dirs), P(off), ctypes.byref(npass), P(sq), P(ax)) == 0
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), int(npass.value), int(off[npass.value])

    def decode_bytes(self):
        """Algorithmic bytes of the batch's decode launches: per pass, every shard of every
        decoded axis read once and every missing shard written once."""
        m = self.mask.astype(bool).copy()
        w, k, total = 2 * self.k, self.k, 0
        while True:
            progress = False
            for d in (0, 1):
                cnt = m.sum(axis=1 - d)
                sel = (cnt >= k) & (cnt < w)
                if sel.any():
                    total += int(sel.sum()) * w * 512 + int((w - cnt[sel]).sum()) * 512
                    if d == 0:
                        m[sel, :] = True
                    else:
                        m[:, sel] = True
                    progress = True
            if not progress:
                return total * self.n


def measure(shape, reps, warmup):
    import torch
    for _ in range(warmup):
        shape.timed(shape.batch)
        shape.timed(shape.sequential)
    tb, ts1, ts2 = [], [], []
    for _ in range(reps):
        tb.append(shape.timed(shape.batch))
        ts1.append(shape.timed(shape.sequential))
        ts2.append(shape.timed(shape.sequential))
    if shape.kind == "p055":  # the batch's bytes, not the sequential calls'
        shape.timed(shape.batch)
        assert torch.equal(shape.work, shape.pristine), "repaired squares differ from the originals"
    n = shape.n
    b, s1, s2 = (statistics.median(t) for t in (tb, ts1, ts2))
    s = statistics.median(ts1 + ts2)
    plan_s, npass, nent = shape.plan_seconds(max(3, reps // 4))
    return {"k": shape.k, "n": n, "mask": shape.kind, "reps": reps,
            "batch_ms": b * 1e3, "sequential_ms": s * 1e3,
            "batch_repairs_per_s": n / b, "sequential_repairs_per_s": n / s,
            "batch_over_sequential": s / b,
            "batch_ms_per_square": b * 1e3 / n, "sequential_ms_per_square": s * 1e3 / n,
            "sequential_spread": abs(s1 - s2) / s,
            "host_plan_ms": plan_s * 1e3, "host_plan_frac_of_batch": plan_s / b,
            "merged_passes": npass, "entries": nent}


def run(a):
    import torch
    torch.cuda.set_device(0)  # before the library opens the device, as bench.py does
    from celestia_eds import default_context
    from celestia_eds.multi import probe
    ctx = default_context(0)
    hbm = probe(ctx, 4 << 30, rs_k=())
    out = {"reps": a.reps, "warmup": a.warmup, "hbm_copy_gbps": hbm["hbm_copy_gbps"], "shapes": []}
    d, rr, cr = _squares(ctx, 128, 64)
    for kind in ("p055", "q0"):
        for n in (1, 2, 4, 16, 64):
            r = measure(Shape(ctx, d, rr, cr, kind, 128, n), a.reps, a.warmup)
            out["shapes"].append(r)
            print(json.dumps(r), flush=True)
    del d
    d, rr, cr = _squares(ctx, 32, 256)
    r = measure(Shape(ctx, d, rr, cr, "p055", 32, 256), a.reps, a.warmup)
    out["shapes"].append(r)
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def trace(a):
    import torch
    torch.cuda.set_device(0)
    from celestia_eds import default_context
    from celestia_eds.multi import probe
    ctx = default_context(0)
    n = a.trace
    d, rr, cr = _squares(ctx, 128, n)
    shape = Shape(ctx, d, rr, cr, "p055", 128, n)
    calls = 5
    for _ in range(calls):
        shape.timed(shape.batch)
    _, npass, nent = shape.plan_seconds(1)
    hbm = probe(ctx, 4 << 30, rs_k=())
    with open(a.out, "w") as f:
        json.dump({"k": 128, "n": n, "mask": "p055", "batch_calls": calls, "merged_passes": npass, "entries": nent,
                   "decode_bytes_per_batch": shape.decode_bytes(), "hbm_copy_gbps": hbm["hbm_copy_gbps"]}, f, indent=1)


def kernel_times(a):
    """Per batch call: launches and microseconds of the batch decode, the batch check and the
    commit's kernels, from rocprofv3's kernel stats of --trace runs."""
    lines = ["Batch repair, k = 128, p = 0.55 (seed 7): kernel time per cel_dev_repair_batch call.",
             "From rocprofv3 --kernel-trace --stats over tools/repair_batch_bench.py --trace N (a run of its own;",
             "5 batch calls each). decode = k_rs_decode_axis<8, true>, check = k_rs_check_axes_batch<7>, commit = the",
             "n-square commit's leaf and level kernels (k_leaf_quad_*, k_level_split). decode bytes = algorithmic bytes",
             "(every shard of every decoded axis read once, every missing shard written once) over their kernel time,",
             "as a fraction of the same run's streaming-copy probe.", ""]
    for stats, tj in zip(a.kernel_times, a.trace_json):
        t = json.load(open(tj))
        groups = {"decode": [0, 0], "check": [0, 0], "commit": [0, 0]}
        with open(stats) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                g = ("decode" if "k_rs_decode_axis" in name else "check" if "k_rs_check_axes_batch" in name else
                     # the n-square commit's own kernels (the squares' extension commits one at a time)
                     "commit" if "k_leaf_quad" in name or "k_level_split" in name else None)
                if g:
                    groups[g][0] += int(row["Calls"])
                    groups[g][1] += int(row["TotalDurationNs"])
        calls = t["batch_calls"]
        lines.append(f"n = {t['n']}: {t['merged_passes']} merged passes, {t['entries']} axes per call, "
                     f"copy probe {t['hbm_copy_gbps']:.0f} GB/s")
        for g, (c, ns) in groups.items():
            per = ns / calls / 1e3
            lines.append(f"  {g:<7}{c / calls:7.1f} launches/call {per:10.1f} us/call {per / max(c / calls, 1e-9):9.1f} us/launch"
                         f" {per / t['n']:8.2f} us/square")
        dec_s = groups["decode"][1] / calls / 1e9
        if dec_s > 0:
            gbs = t["decode_bytes_per_batch"] / dec_s / 1e9
            lines.append(f"  decode bytes {t['decode_bytes_per_batch'] / 1e6:.1f} MB/call -> {gbs:.0f} GB/s = "
                         f"{gbs / t['hbm_copy_gbps']:.3f} of the copy probe")
        lines.append("")
    with open(a.out_txt, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_batch_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--kernel-times", nargs="+")
    ap.add_argument("--trace-json", nargs="+")
    ap.add_argument("--out-txt", default=os.path.join(ROOT, "profiles", "repair_batch_kernel_times.txt"))
    a = ap.parse_args()
    if a.kernel_times:
        kernel_times(a)
    elif a.trace:
        trace(a)
    else:
        run(a)
