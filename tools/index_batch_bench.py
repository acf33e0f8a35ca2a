"""Serving many resident squares: the batch calls (cel_dev_tree_index_build_batch,
cel_dev_prove_squares, cel_dev_namespace_plan_squares, cel_dev_namespace_prove_squares) against the
same work through the single-square calls one square after another, in the same process, on the
same resident squares, alternating.

Workload per square, a light client's shape: the tree index, 16 sample proofs with their shares,
one namespace query with its proofs and shares.

  loop    per square cel_dev_tree_index_build, cel_dev_prove_batch (16 samples),
          cel_dev_namespace_plan (1 namespace), cel_dev_namespace_prove; timed as two interleaved
          series (A before the batch, B after it): the difference of their medians is the margin
          below which a difference to the batch means nothing
  batch   one call each over all squares: 16 n samples in one request table, n queries in one plan

Shapes: k = 32 with n = 256 and n = 1; k = 128 with n = 16, n = 64 and n = 1. Every shape is warmed
(three rounds of both variants) and the two variants' outputs are compared before timing. Times
are host wall clock around calls that end in a device synchronise; medians of --reps rounds
(default 20). Kernel times come from a rocprofv3 --kernel-trace run of its own per variant
(--ktrace; nothing else is traced in it): the sum of all kernel durations of a round. Each shape
runs in a child process under a time limit; the parent never opens the device and stops at the
first child that fails. Writes profiles/index_batch_bench.json.

  python tools/index_batch_bench.py [--reps 20] [--ktrace] [--shapes k32n256,k128n16] [--out FILE]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ["k32n256", "k32n1", "k128n16", "k128n64", "k128n1"]
SAMPLES = 16
CHILD_LIMIT_S = 300
TRACE_ROUNDS = 4


def med(ts):
    a = np.sort(np.asarray(ts, np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1])}


class Shape:
    """n copies of one square of width k on the device, and both variants' buffers."""

    def __init__(self, name):
        import torch
        import celestia_eds
        from celestia_eds.testfactory import random_ods
        self.k, self.n = (int(x) for x in name[1:].split("n"))
        k, n, w = self.k, self.n, 2 * self.k
        self.ctx = celestia_eds.default_context(0)
        lib = self.lib = self.ctx.lib
        dev = torch.device("cuda", self.ctx.device)
        rng = np.random.default_rng(k)
        ods = random_ods(k, 5)
        cells = rng.integers(0, 256, (w, w, 512), dtype=np.uint8)  # any cells: the index hashes what is there
        cells[:k, :k] = ods
        new = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
        self.d_eds = torch.as_tensor(cells).to(dev).unsqueeze(0).repeat(n, 1, 1, 1).contiguous()
        self.size = lib.cel_dev_tree_index_size(k)
        self.d_index = new(n * self.size)
        self.d_roots, self.d_dah = new(2, n, w, 90), new(n, 32)
        self.sq = np.repeat(np.arange(n, dtype=np.uint32), SAMPLES)
        self.axes = rng.integers(0, 2, n * SAMPLES).astype(np.uint8)
        self.index = rng.integers(0, w, n * SAMPLES).astype(np.uint32)
        self.starts = rng.integers(0, w, n * SAMPLES).astype(np.int32)
        self.ends = self.starts + 1
        lg = w.bit_length() - 1
        self.tn = n * SAMPLES * lg
        self.d_leaves, self.d_nodes = new(n * SAMPLES, 512), new(self.tn, 90)
        self.d_pwork = new(max(lib.cel_dev_prove_squares_workspace_size(n * SAMPLES), lib.cel_dev_prove_workspace_size(SAMPLES)))
        self.qsq = np.arange(n, dtype=np.uint32)
        self.ns = np.ascontiguousarray(np.stack([ods[int(r), int(c), :29] for r, c in rng.integers(0, k, (n, 2))]))
        self.d_nwork = new(lib.cel_dev_namespace_squares_workspace_size(k, n))
        cap = n * w
        self.cap = cap
        self.ent = [np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.int32), np.zeros(cap, np.int32),
                    np.zeros(cap, np.uint8), np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint64)]
        # room for the namespaces' shares and nodes: each variant checks the plan's totals against
        # it before it lets the prove call write
        self.leaf_cap, self.node_cap = 64 * n, 64 * n * (lg + 1)
        self.d_nleaves, self.d_nnodes = new(self.leaf_cap, 512), new(self.node_cap, 90)
        self.cnt = ctypes.c_uint64()
        self.status = np.zeros(n, np.int32)
        self.torch = torch
        self.entries = 0
        torch.cuda.synchronize()  # the library's stream does not wait for torch's

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def batch(self):
        P, p, lib, h, k, n = (lambda a: a.ctypes.data_as(ctypes.c_void_p)), self.p, self.lib, self.ctx.handle, self.k, self.n
        t0 = time.perf_counter()
        c = self.ctx.check
        c(lib.cel_dev_tree_index_build_batch(h, p(self.d_eds), n, k, p(self.d_index), p(self.d_roots[0]), p(self.d_roots[1]),
                                             p(self.d_dah), P(self.status), 0, None))
        c(lib.cel_dev_prove_squares(h, p(self.d_eds), p(self.d_index), k, n, n * SAMPLES, P(self.sq), P(self.axes),
                                    P(self.index), P(self.starts), P(self.ends), p(self.d_leaves), p(self.d_nodes),
                                    p(self.d_pwork), None))
        c(lib.cel_dev_namespace_plan_squares(h, p(self.d_index), k, n, n, P(self.qsq), P(self.ns), self.cap,
                                             *[P(a) for a in self.ent], ctypes.byref(self.cnt), p(self.d_nwork), None))
        m = self.cnt.value
        assert int(self.ent[5][m]) <= self.leaf_cap and int(self.ent[6][m]) <= self.node_cap, "the plan outgrows the buffers"
        c(lib.cel_dev_namespace_prove_squares(h, p(self.d_eds), p(self.d_index), k, n, self.cnt.value, p(self.d_nleaves),
                                              p(self.d_nnodes), p(self.d_nwork), None))
        self.torch.cuda.synchronize()
        self.entries = self.cnt.value
        return time.perf_counter() - t0

    def loop(self):
        P, lib, h, k, n, w = (lambda a: a.ctypes.data_as(ctypes.c_void_p)), self.lib, self.ctx.handle, self.k, self.n, 2 * self.k
        at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off)
        lg = w.bit_length() - 1
        c = self.ctx.check
        st = ctypes.c_int32()
        t0 = time.perf_counter()
        e0 = l0 = n0 = 0
        for i in range(n):
            eds, idx = at(self.d_eds, i * w * w * 512), at(self.d_index, i * self.size)
            s = slice(i * SAMPLES, (i + 1) * SAMPLES)
            c(lib.cel_dev_tree_index_build(h, eds, k, idx, at(self.d_roots, i * w * 90), at(self.d_roots, (n + i) * w * 90),
                                           at(self.d_dah, i * 32), ctypes.byref(st), 0, None))
            c(lib.cel_dev_prove_batch(h, eds, idx, k, SAMPLES, P(self.axes[s]), P(self.index[s]), P(self.starts[s]),
                                      P(self.ends[s]), at(self.d_leaves, i * SAMPLES * 512), at(self.d_nodes, i * SAMPLES * lg * 90),
                                      self.p(self.d_pwork), None))
            ent = [a[e0:] for a in self.ent]
            c(lib.cel_dev_namespace_plan(h, idx, k, 1, P(self.ns[i]), self.cap - e0, *[P(a) for a in ent],
                                         ctypes.byref(self.cnt), self.p(self.d_nwork), None))
            m = self.cnt.value
            assert l0 + int(ent[5][m]) <= self.leaf_cap and n0 + int(ent[6][m]) <= self.node_cap, "the plan outgrows the buffers"
            c(lib.cel_dev_namespace_prove(h, eds, idx, k, m, at(self.d_nleaves, l0 * 512), at(self.d_nnodes, n0 * 90),
                                          self.p(self.d_nwork), None))
            l0, n0, e0 = l0 + int(ent[5][m]), n0 + int(ent[6][m]), e0 + m
        self.torch.cuda.synchronize()
        self.entries = e0
        return time.perf_counter() - t0

    def outputs(self):
        """What a variant left on the device, for the comparison."""
        t = self.torch
        idx = self.d_index.view(self.n, self.size)[:, :self.size - 48]  # but the DAH, flag and status of the tail
        return [x.clone() for x in (idx, self.d_roots, self.d_dah, self.d_leaves, self.d_nodes, self.d_nleaves, self.d_nnodes)] + \
               [t.as_tensor(np.stack([a[:self.entries] for a in self.ent[1:5]]).astype(np.int64))]


def run_shape(name, reps, trace=None):
    s = Shape(name)
    if trace:
        for _ in range(TRACE_ROUNDS):
            getattr(s, trace)()
        return None
    for _ in range(3):
        s.loop()
        want = s.outputs()
        s.batch()
        got = s.outputs()
    for a, b in zip(want, got):
        assert a.shape == b.shape and bool((a == b).all()), "the batch calls and the single-square calls disagree"
    la, lb, bt = [], [], []
    for _ in range(reps):
        la.append(s.loop())
        bt.append(s.batch())
        lb.append(s.loop())
    A, B, T = med(la), med(lb), med(bt)
    loop_med, margin = 0.5 * (A["median"] + B["median"]), abs(A["median"] - B["median"])
    return {"k": s.k, "squares": s.n, "samples_per_square": SAMPLES, "namespace_entries": int(s.entries),
            "loop_a_s": A, "loop_b_s": B, "loop_margin_s": margin, "batch_s": T,
            "loop_us_per_square": 1e6 * loop_med / s.n, "batch_us_per_square": 1e6 * T["median"] / s.n,
            "batch_over_loop": loop_med / T["median"],
            "batch_beats_loop_by_more_than_margin": bool(loop_med - T["median"] > margin),
            "batch_within_margin_of_loop": bool(abs(loop_med - T["median"]) <= margin)}


def kernel_time(name, variant):
    """Sum of the kernel durations of one round of `variant`, from a rocprofv3 --kernel-trace run
    of a child that runs TRACE_ROUNDS rounds of it and nothing else: {kernel: us per round}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--trace", name, "--variant", variant]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 exit {r.returncode}: {r.stderr[-2000:]}")
        per = {}
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                kname = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0][:60]
                per[kname] = per.get(kname, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
    per = {kn: us / TRACE_ROUNDS for kn, us in per.items() if "cel" in kn or "k_" in kn}
    return {"total_us": sum(per.values()), "kernels_us": dict(sorted(per.items(), key=lambda kv: -kv[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_batch_bench.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ktrace", action="store_true", help="also one rocprofv3 --kernel-trace run per shape and variant")
    ap.add_argument("--child", help="run one shape in this process and print its JSON line")
    ap.add_argument("--trace", help="a few rounds of one variant of one shape, nothing timed")
    ap.add_argument("--variant", default="batch", choices=["batch", "loop"])
    args = ap.parse_args()
    if args.trace:
        run_shape(args.trace, 0, trace=args.variant)
        return 0
    if args.child:
        print("RESULT " + json.dumps(run_shape(args.child, args.reps)), flush=True)
        return 0
    result = {"reps": args.reps, "samples_per_square": SAMPLES, "queries_per_square": 1, "shapes": {}}
    for name in args.shapes.split(","):
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
        result["shapes"][name] = json.loads(lines[-1][len("RESULT "):])
        if args.ktrace:
            try:
                result["shapes"][name]["kernel_trace"] = {v: kernel_time(name, v) for v in ("batch", "loop")}
            except (RuntimeError, subprocess.TimeoutExpired, OSError) as e:
                print(f"{name}: kernel trace failed: {e}; stopping", flush=True)
                return 1
        print(name, json.dumps(result["shapes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
