"""CPU: tools/extend_plan_check.cpp, a stand-alone host program (its own main,
csrc/extend_plan.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For every
k = 1 .. 512 and n = 1 .. 40 it checks that the chunks of the device batch, of the host pipeline
and of the k = 512 upload partition their range in order with the counts, slots and workspace
offsets of the formulas, and the result block's offsets and unpack; for k = 2 .. 64 it paints a
host map from a device map through the copy-back rectangles (full and parity only; the whole
square, the row ranges of the early download, every rank's slab at N = 1, 2, 4, 8) against a map
filled cell by cell. Both builds must run clean and report ok, with the counts per k worked out
here independently, so a check that skips cases fails."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "extend_plan_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
WIDTHS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
NS = range(1, 41)


def _host_chunks(n):
    """nc = min(n, 4), chunk = ceil(n / nc), nchunks = ceil(n / chunk)."""
    chunk = -(-n // min(n, 4))
    return -(-n // chunk)


def _painted(k):
    """(rectangles, cells) over the painting cases of width k: a case's wanted cells as a boolean
    map, one rectangle for the rows above k if any cell is wanted there, one for the rows below."""
    w = 2 * k
    cases = [(0, w, 0, w), (0, k, 0, w), (k, w, 0, w)]
    if k >= 4:
        cases += [(c * k // 4, (c + 1) * k // 4, 0, w) for c in range(4)]
    cases += [(0, w, r * (w // n), w // n) for n in (1, 2, 4, 8) if n <= w for r in range(n)]
    rects = cells = 0
    for parity in (False, True):
        for r0, r1, c0, cw in cases:
            want = np.zeros((w, w), bool)
            want[r0:r1, c0:c0 + cw] = True
            if parity:
                want[:k, :k] = False
            rects += int(want[:k].any()) + int(want[k:].any())
            cells += int(want.sum())
    return rects, cells


def _counts(k):
    rects, cells = _painted(k) if 2 <= k <= 64 else (0, 0)
    return (sum(1 if n < 2 else 2 for n in NS),          # device batch: two halves from n = 2 on
            sum((n + 1) // 2 for n in NS),               # ... the first one ceil(n / 2) squares
            sum(_host_chunks(n) for n in NS),
            sum(c % 4 for n in NS for c in range(_host_chunks(n))),  # chunk c on stream and workspace slot c % kPipe
            sum(min(_host_chunks(n), 4) for n in NS),    # workspace slots in use
            4 if k >= 4 else 0, rects, cells)


def test_formulas_of_the_issue():
    """The figures the plans must reproduce, at the shapes the GPU tests lean on."""
    assert [_host_chunks(n) for n in (1, 2, 4, 5, 16, 17)] == [1, 2, 4, 3, 4, 4]
    assert _painted(2)[1] > 0 and _counts(1)[-2:] == (0, 0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_extend_plan_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    want = [_counts(k) for k in WIDTHS]
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert "FAIL" not in r.stdout and lines[-1] == "extend plan check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + 1
        for k, (pipe, first, host, slot_sum, nslots, up, rects, cells), line in zip(WIDTHS, want, lines):
            assert line == (f"k = {k:3d}: {pipe} pipe chunks, {first} in first halves, {host} host chunks, "
                            f"{slot_sum} slot sum, {nslots} slots in use, {up} upload chunks, {rects} rectangles, "
                            f"{cells} cells"), line
