"""A/B of the host extension paths between this tree and another build of the project (the parent
commit in a second tree), by the protocol of profiles/repair_refactor_ab.txt.

  python tools/extend_ab.py run --parent DIR --out DIR ab1 aa1 ab2 ...
  python tools/extend_ab.py table --out DIR ab1 ab2 ...

A set is parent, new, parent; a run is five processes, each under its own time limit:
tools/header_lat.py page-locked and pageable (k = 128, 256, 512), bench.py's measure_host_io at
k = 128 (three batch figures, three single-square figures), bench.py's rowshard512_lib rider on one
device, and tools/block_bench.py's block medians. A set named aa* is the null experiment: all three
runs are the parent's. The run stops at the first process that fails. Milliseconds throughout.
spread = |parent1 - parent2|, over = new - the slower parent, a figure is flagged when over > spread."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_IO = ("import json, bench, celestia_eds; r = bench.measure_host_io(celestia_eds.default_context(0), 128); "
           "print('RESULT ' + json.dumps(r))")
ROWSHARD = "import json, bench; print('RESULT ' + json.dumps(bench.measure_rowshard_lib(512, 1, 5, 2, 4)))"


def proc(tree, limit, cmd):
    env = dict(os.environ, PYTHONPATH=os.path.join(tree, "celestia-app_amd"))
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=tree, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print(f"STOP: {tree} {cmd[:3]} exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", flush=True)
        sys.exit(3)
    return r.stdout


def result(out):
    return json.loads(next(l for l in reversed(out.split("\n")) if l.startswith("RESULT "))[7:])


def measure(tree):
    f = {}
    for mode in ("pinned", "pageable"):
        out = proc(tree, 120, [sys.executable, "tools/header_lat.py", "10"] + (["pageable"] if mode == "pageable" else []))
        for k, ms in re.findall(r"k=\s*(\d+):\s*([\d.]+) ms", out):
            f[f"header {mode} k={k}"] = float(ms)
    io = result(proc(tree, 180, [sys.executable, "-c", HOST_IO]))
    for name in ("with_eds", "parity_only", "roots_only"):
        f[f"host_io batch {name}"] = io[name]["ms_per_call"]
    for name in ("single_square_parity_only_ms", "single_square_dah_only_ms", "single_square_k512_dah_only_ms"):
        f[f"host_io {name[:-3]}"] = io[name]
    f["rowshard512_lib latency"] = result(proc(tree, 180, [sys.executable, "-c", ROWSHARD]))["latency_ms"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "block.json")
        proc(tree, 240, [sys.executable, "tools/block_bench.py", "--reps", "20", "--out", path])
        for shape, d in json.load(open(path))["shapes"].items():
            f[f"block {shape}"] = d["block_extend_s"]["median"] * 1e3
    return f


def run(a):
    os.makedirs(a.out, exist_ok=True)
    for s in a.sets:
        new = a.parent if s.startswith("aa") else ROOT
        res = {}
        for name, tree in (("parent1", a.parent), ("new", new), ("parent2", a.parent)):
            res[name] = measure(tree)
            print(s, name, res[name], flush=True)
            with open(os.path.join(a.out, f"set_{s}.json"), "w") as f:
                json.dump(res, f, indent=1)


def table(a):
    data = {s: json.load(open(os.path.join(a.out, f"set_{s}.json"))) for s in a.sets}
    figs = list(data[a.sets[0]]["new"])
    flags = {f: 0 for f in figs}
    for s in a.sets:
        print(f"set {s}\n  {'figure':<40}{'parent1':>10}{'parent2':>10}{'new':>10}{'spread':>9}{'over':>9}")
        for f in figs:
            p1, p2, n = (data[s][r][f] for r in ("parent1", "parent2", "new"))
            spread, over = abs(p1 - p2), n - max(p1, p2)
            flags[f] += over > spread
            print(f"  {f:<40}{p1:10.4f}{p2:10.4f}{n:10.4f}{spread:9.4f}{over:+9.4f}{' flag' if over > spread else ''}")
        print()
    print(f"Across sets {', '.join(a.sets)}: median of the parent runs, of the new runs, sets flagged.")
    print(f"  {'figure':<40}{'parent':>10}{'new':>10}{'new/parent':>11}{'flags':>7}")
    for f in figs:
        mp = statistics.median(data[s][r][f] for s in a.sets for r in ("parent1", "parent2"))
        mn = statistics.median(data[s]["new"][f] for s in a.sets)
        print(f"  {f:<40}{mp:10.4f}{mn:10.4f}{mn / mp:11.4f}{flags[f]:7d}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "table"])
    ap.add_argument("--parent")
    ap.add_argument("--out", required=True)
    ap.add_argument("sets", nargs="+")
    a = ap.parse_args()
    run(a) if a.cmd == "run" else table(a)
