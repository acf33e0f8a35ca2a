"""A/B of `bench.py --mode repair` between this tree and another build of the project (the parent
commit in a second tree), by the protocol of profiles/repair_refactor_ab.txt.

  python tools/repair_ab.py run --parent DIR --out DIR ab1 aa1 ab2 ...
  python tools/repair_ab.py table --out DIR ab1 ab2 ...

A set is, per k = 32, 128, 256, 512: parent, new, parent, every bench run its own process under
its own time limit (--steps 20 --warmup 3 --cpu-seconds 0.5, device input). A set named aa* is the
null experiment: all three runs are the parent's. The run stops at the first bench run that does
not end with a result line. spread = |parent1 - parent2|, over = new - the slower parent, a figure
is flagged when over > spread.

k = 32: bench.py's byzantine measurement indexes row 200 and column 77 of the mask and raises at
2k = 64, so that width runs bench.py's run_repair with that one function replaced by a stub
(ms_per_step only)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [32, 128, 256, 512]
LIMIT = {32: 120, 128: 120, 256: 150, 512: 240}
NO_BYZ = ("import sys, bench; bench.measure_byzantine_repair = lambda *a, **k: None; "
          "sys.argv = ['bench.py'] + sys.argv[1:]; bench.main()")
FIGS = [(f"k={k} ms_per_step", str(k), "ms_per_step") for k in KS] + \
       [(f"k={k} byzantine ms_per_repair", str(k), "byz_ms_per_repair") for k in KS if k != 32]


def bench(tree, k):
    args = ["--gpus", "1", "--mode", "repair", "--k", str(k), "--steps", "20", "--warmup", "3", "--cpu-seconds", "0.5"]
    cmd = [sys.executable, "-c", NO_BYZ] + args if k == 32 else [sys.executable, "bench.py"] + args
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT[k])] + cmd, cwd=tree, capture_output=True, text=True)
    line = next((l for l in reversed(r.stdout.strip().split("\n")) if l.startswith("{")), None)
    if r.returncode != 0 or line is None:
        print(f"STOP: {tree} k={k} exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", flush=True)
        sys.exit(3)
    d = json.loads(line)
    return {"ms_per_step": d["ms_per_step"],
            "byz_ms_per_repair": d["byzantine"]["ms_per_repair"] if d.get("byzantine") else None}


def run(a):
    os.makedirs(a.out, exist_ok=True)
    for s in a.sets:
        new = a.parent if s.startswith("aa") else ROOT
        res = {}
        for k in KS:
            res[str(k)] = {"parent1": bench(a.parent, k), "new": bench(new, k), "parent2": bench(a.parent, k)}
            print(s, k, res[str(k)], flush=True)
            with open(os.path.join(a.out, f"set_{s}.json"), "w") as f:
                json.dump(res, f, indent=1)


def table(a):
    data = {s: json.load(open(os.path.join(a.out, f"set_{s}.json"))) for s in a.sets}
    flags = {f[0]: 0 for f in FIGS}
    for s in a.sets:
        print(f"set {s}\n  {'figure':<34}{'parent1':>10}{'parent2':>10}{'new':>10}{'spread':>9}{'over':>9}")
        for label, k, field in FIGS:
            p1, p2, n = (data[s][k][r][field] for r in ("parent1", "parent2", "new"))
            spread, over = abs(p1 - p2), n - max(p1, p2)
            flags[label] += over > spread
            print(f"  {label:<34}{p1:10.4f}{p2:10.4f}{n:10.4f}{spread:9.4f}{over:+9.4f}{' flag' if over > spread else ''}")
        print()
    print(f"Across sets {', '.join(a.sets)}: median of the parent runs, of the new runs, sets flagged.")
    print(f"  {'figure':<34}{'parent':>10}{'new':>10}{'new/parent':>11}{'flags':>7}")
    for label, k, field in FIGS:
        mp = statistics.median(data[s][k][r][field] for s in a.sets for r in ("parent1", "parent2"))
        mn = statistics.median(data[s][k]["new"][field] for s in a.sets)
        print(f"  {label:<34}{mp:10.4f}{mn:10.4f}{mn / mp:11.4f}{flags[label]:7d}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "table"])
    ap.add_argument("--parent")
    ap.add_argument("--out", required=True)
    ap.add_argument("sets", nargs="+")
    a = ap.parse_args()
    run(a) if a.cmd == "run" else table(a)
