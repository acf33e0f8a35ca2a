"""CPU: tools/befp_plan_check.cpp, a stand-alone host program (its own main,
csrc/befp_plan.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For every
width 2 .. 64 it walks the fraud proofs' host planner: every MALFORMED cause, TOO_FEW at k - 1
entries and not at k, each entry's place in the square, the packed offsets of a batch that mixes
every outcome with empty proofs, the producer's selection over the masks of
tools/repair_plan_check.cpp, and the node records of a single-leaf proof against a recursive
ProveRange. Both builds must run clean and report ok, with the number of positions taken and
skipped per width worked out here independently (the same masks, numpy)."""
import os
import shutil
import subprocess

import pytest

from test_repair_plan_check import INC, ROOT, SAN, _masks

SRC = os.path.join(ROOT, "tools", "befp_plan_check.cpp")
WIDTHS = [2, 4, 8, 16, 32, 64]


def _counts(w):
    """Over the masks and the six accused axes the program takes: known cells whose orthogonal
    axis is complete (taken), and known cells whose orthogonal axis is not (skipped)."""
    k = w // 2
    taken = skipped = 0
    masks = _masks(w)
    for m in masks:
        full_cols, full_rows = m.all(axis=0), m.all(axis=1)
        for index in (0, k, w - 1):
            row, col = m[index, :], m[:, index]
            taken += int((row & full_cols).sum()) + int((col & full_rows).sum())
            skipped += int((row & ~full_cols).sum()) + int((col & ~full_rows).sum())
    return len(masks), taken, skipped


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_befp_plan_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    want = [_counts(w) for w in WIDTHS]
    assert any(t for _, t, _ in want) and any(s for _, _, s in want)
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert "FAIL" not in r.stdout and lines[-1] == "befp plan check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + 1
        for w, (masks, taken, skipped), line in zip(WIDTHS, want, lines):
            assert line.split() == ["W", "=", f"{w}:", str(masks), "masks,", str(taken), "taken,", str(skipped),
                                    "skipped"], line
