"""CPU: tools/prove_select_check.cpp, a stand-alone host program (its own main, csrc/nmt_prove.hpp
alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked statically: nothing is
preloaded and nothing is loaded into python) and once plain. For every range of every width
2k = 2 .. 256 it compares the closed form of nmt ProveRange's node selection, which the prove
kernel and cel_prove_offsets share, with the recursion of proof.cpp: count, order, levels and
positions. For k = 1 .. 512 it checks that the tree index's levels and tail tile its size
without gap or overlap, and for k <= 32 that index_record names every record of a table of
exactly that size (leaves twice, by row and by column; the rest once). Both builds must run
clean and report ok."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "prove_select_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
WIDTHS = [2, 4, 8, 16, 32, 64, 128, 256]
KS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


def _ranges_nodes(w):
    """Ranges of w leaves and the nodes of all their proofs: popcount(s) + L - popcount(e - 1)."""
    L = w.bit_length() - 1
    return w * (w + 1) // 2, sum(bin(s).count("1") + L - bin(e - 1).count("1")
                                 for s in range(w) for e in range(s + 1, w + 1))


def _index_bytes(k):
    w = 2 * k
    records = w * w + 2 * w * (w - 1)  # the leaves once, then 2w trees of w - 1 inner nodes
    return records, records * 96 + 2 * w * 32 + 48


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_prove_select_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        assert "FAIL" not in r.stdout and lines[-1] == "prove select check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + len(KS) + 1
        for w, line in zip(WIDTHS, lines):
            ranges, nodes = _ranges_nodes(w)
            assert line.split() == ["W", "=", f"{w}:", str(ranges), "ranges,", str(nodes), "proof", "nodes"], line
        for k, line in zip(KS, lines[len(WIDTHS):]):
            records, nbytes = _index_bytes(k)
            assert line.split() == ["k", "=", f"{k}:", str(records), "records", "in", str((2 * k).bit_length()),
                                    "levels,", str(nbytes), "bytes"], line


def test_index_size_matches_layout():
    """cel_dev_tree_index_size is the layout's size; 0 for a width the index does not take."""
    import celestia_eds._lib as L
    lib = L.load()
    for k in KS:
        assert lib.cel_dev_tree_index_size(k) == _index_bytes(k)[1]
    for k in (0, 3, 6, 4096):
        assert lib.cel_dev_tree_index_size(k) == 0
    assert lib.cel_dev_prove_workspace_size(0) > 0
    assert lib.cel_dev_prove_workspace_size(1000) >= 32 * 1000
