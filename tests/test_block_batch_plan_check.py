"""CPU: tools/block_batch_plan_check.cpp, a stand-alone host program (its own main,
csrc/block_batch_plan.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime
linked statically: nothing is preloaded and nothing is loaded into python) and once plain. For
every multiset of 1 .. 6 widths from {1, 2, 4, ..., 512}, shuffled and with failed blocks
interleaved, it plans the batch under four budgets (one byte, the widest block, the whole batch,
0 = the default) and checks the map back, the width classes, the chunks, the class runs and the
per-block records. Both builds must run clean and report ok, with the number of multisets and of
chunks per batch size worked out here independently with numpy: the chunks of a budget are a
greedy cut of the ascending EDS sizes, whatever the caller's order and the failed blocks."""
import itertools
import shutil
import subprocess

import numpy as np
import pytest

from test_repair_plan_check import INC, ROOT, SAN
import os

SRC = os.path.join(ROOT, "tools", "block_batch_plan_check.cpp")
WIDTHS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
MAX_BLOCKS = 6
DEFAULT_BUDGET = 2 << 30


def _chunks(sizes, budget):
    """Chunks of the ascending sizes: a chunk ends where the next size would pass the budget."""
    ends = np.cumsum(sizes)
    n = start = 0
    while start < len(sizes):
        base = ends[start - 1] if start else 0
        fit = int(np.searchsorted(ends, base + budget, side="right"))  # sizes[start:fit] fit
        start = max(fit, start + 1)
        n += 1
    return n


def _counts(m):
    sets = chunks = 0
    for ws in itertools.combinations_with_replacement(WIDTHS, m):
        sizes = np.sort(np.array([4 * k * k * 512 for k in ws], np.int64))
        for budget in (1, int(sizes.max()), int(sizes.sum()), DEFAULT_BUDGET):
            chunks += _chunks(sizes, budget)
        sets += 1
    return sets, chunks


def test_chunk_count_by_hand():
    mib = 1 << 20
    assert _chunks(np.array([32 * mib] * 3), 64 * mib) == 2
    assert _chunks(np.array([2048, 8192, 512 * mib]), 1) == 3
    assert _chunks(np.array([512 * mib] * 6), DEFAULT_BUDGET) == 2


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_batch_plan_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    want = [_counts(m) for m in range(1, MAX_BLOCKS + 1)]
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert "FAIL" not in r.stdout and lines[-1] == "block batch plan check: ok", r.stdout[-2000:]
        assert len(lines) == MAX_BLOCKS + 1
        for m, (sets, chunks), line in zip(range(1, MAX_BLOCKS + 1), want, lines):
            assert line.split() == ["n", "=", f"{m}:", str(sets), "multisets,", str(chunks), "chunks"], line
