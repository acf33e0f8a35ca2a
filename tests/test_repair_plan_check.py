"""CPU: tools/repair_plan_check.cpp, a stand-alone host program (its own main,
csrc/repair_plan.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For every
width 2 .. 256 it runs the repair's pass schedule over random and structured presence masks
beside a byte mask filled cell by cell: the first-row scan, every pass's list, the counts and
bitsets after every fill_pass, the orthogonal axes each solve completes, the closure against
rsmt2d's sweep order, rollback, and the replay of the check order over synthetic results. Both
builds must run clean and report ok, with the number of masks, passes and solves per width
worked out here independently (the same masks, whole directions filled with numpy)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "repair_plan_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
WIDTHS = [2, 4, 8, 16, 32, 64, 128, 256]
SURVIVAL = [0.3, 0.5, 0.55, 0.7, 0.9]
REPS = 4


def _random_mask(w, seed, p):
    """Cell c survives when splitmix64(seed, c) < p, as the program draws it."""
    x = np.uint64(seed) + (np.arange(w * w, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return ((x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) < p).reshape(w, w)


def _masks(w):
    k = w // 2
    out = [_random_mask(w, 0xC0FFEE + w * 1000 + pi * 10 + rep, p)
           for pi, p in enumerate(SURVIVAL) for rep in range(REPS)]
    quad = np.zeros((w, w), bool)
    quad[:k, :k] = True
    left = np.zeros((w, w), bool)
    left[:, :k] = True
    but_one = np.ones((w, w), bool)
    but_one[w - 1, k] = False
    return out + [quad, left, but_one, np.ones((w, w), bool)]


def _schedule(m):
    """Passes (every solvable row, then every solvable column, until none) and solves of a mask."""
    w = m.shape[0]
    m = m.copy()
    passes = solves = 0
    while True:
        progress = False
        for axis in (1, 0):  # rows: counts along axis 1
            cnt = m.sum(axis=axis)
            sel = (cnt >= w // 2) & (cnt < w)
            if not sel.any():
                continue
            if axis == 1:
                m[sel, :] = True
            else:
                m[:, sel] = True
            passes += 1
            solves += int(sel.sum())
            progress = True
        if m.all() or not progress:
            return passes, solves


def _counts(w):
    masks = _masks(w)
    sched = [_schedule(m) for m in masks]
    return len(masks), sum(p for p, _ in sched), sum(s for _, s in sched)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_repair_plan_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    want = [_counts(w) for w in WIDTHS]
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert "FAIL" not in r.stdout and lines[-1] == "repair plan check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + 1
        for w, (masks, passes, solves), line in zip(WIDTHS, want, lines):
            assert line.split() == ["W", "=", f"{w}:", str(masks), "masks,", str(passes), "passes,", str(solves),
                                    "solves"], line
