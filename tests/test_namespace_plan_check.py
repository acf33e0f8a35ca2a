"""CPU: tools/namespace_plan_check.cpp, a stand-alone host program (its own main,
csrc/nmt_namespace.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For every row
width 2 .. 256 and every class of a (namespace, row) pair it checks the entry classification and
the node counts against a walk of the tree, that every range and every absence leaf lies inside
the row, and that the offsets of the prefix sum tile the outputs without gap or overlap. Both
builds must run clean and report ok, with the counts worked out here independently."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "namespace_plan_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
WIDTHS = [2, 4, 8, 16, 32, 64, 128, 256]


def _nodes(w, s, e):
    L = w.bit_length() - 1
    return bin(s).count("1") + L - bin(e - 1).count("1")


def _counts(w):
    """Pairs: inside or not, 0 <= lt <= le <= w. Entries: inside and lt < w."""
    pairs = 2 * (w + 1) * (w + 2) // 2
    entries = nodes = leaves = 0
    for lt in range(w):
        for le in range(lt, w + 1):
            entries += 1
            if le > lt:
                nodes += _nodes(w, lt, le)
                leaves += le - lt
            else:
                nodes += _nodes(w, lt, lt + 1) + 1
    return pairs, entries, nodes, leaves


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_namespace_plan_check_sanitizer_clean(tmp_path):
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
        assert "FAIL" not in r.stdout and lines[-1] == "namespace plan check: ok", r.stdout[-2000:]
        assert len(lines) == len(WIDTHS) + 1
        for w, line in zip(WIDTHS, lines):
            pairs, entries, nodes, leaves = _counts(w)
            assert line.split() == ["W", "=", f"{w}:", str(pairs), "pairs,", str(entries), "entries,", str(nodes),
                                    "nodes,", str(leaves), "shares"], line
