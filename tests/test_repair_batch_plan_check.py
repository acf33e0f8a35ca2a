"""CPU: tools/repair_batch_plan_check.cpp, a stand-alone host program (its own main,
csrc/repair_plan.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For every
width 2 .. 256 it merges the pass schedules of five batches of five masks (the masks of
tools/repair_plan_check.cpp) as cel_dev_repair_batch does and checks the early pass, the entry
bounds, each square's projection against a byte mask filled cell by cell, each square's check
order, solve log and rollback against the single-square loop, and the per-square verdicts over
synthetic batch results in which one square fails and the others pass. Both builds must run
clean and report ok, with the number of merged passes and entries per width worked out here
independently (the same masks, whole directions filled with numpy)."""
import os
import shutil
import subprocess

import pytest

from test_repair_plan_check import INC, ROOT, SAN, WIDTHS, _masks

SRC = os.path.join(ROOT, "tools", "repair_batch_plan_check.cpp")
BATCHES, BATCH = 5, 5


def _merged(masks):
    """(non-empty global passes, entries) of the merged schedule: every square's solvable rows,
    then every square's solvable columns, until no square has any."""
    ms = [m.copy() for m in masks]
    passes = entries = 0
    while True:
        progress = False
        for axis in (1, 0):  # rows: counts along axis 1
            here = 0
            for m in ms:
                w = m.shape[0]
                cnt = m.sum(axis=axis)
                sel = (cnt >= w // 2) & (cnt < w)
                if axis == 1:
                    m[sel, :] = True
                else:
                    m[:, sel] = True
                here += int(sel.sum())
            if here:
                passes += 1
                entries += here
                progress = True
        if not progress:
            return passes, entries


def _counts(w):
    masks = _masks(w)
    got = [_merged([masks[(b + 5 * j) % len(masks)] for j in range(BATCH)]) for b in range(BATCHES)]
    return BATCHES, sum(p for p, _ in got), sum(e for _, e in got)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_repair_batch_plan_check_sanitizer_clean(tmp_path):
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
        assert "FAIL" not in r.stdout and lines[-1] == "repair batch plan check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + 1
        for w, (batches, passes, entries), line in zip(WIDTHS, want, lines):
            assert line.split() == ["W", "=", f"{w}:", str(batches), "batches,", str(passes), "passes,", str(entries),
                                    "entries"], line
