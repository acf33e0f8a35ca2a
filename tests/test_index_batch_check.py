"""CPU: tools/index_batch_check.cpp, a stand-alone host program (its own main, csrc/nmt_prove.hpp
and csrc/nmt_namespace.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime
linked statically: nothing is preloaded and nothing is loaded into python) and once plain. It
walks the slice, level, record and cell arithmetic of the batch tree index, which the batch
build, k_prove_squares and the k_ns_*_squares kernels share, for k = 1 .. 64 and n = 1 .. 5
squares against index_record per square, one shape past 2^32 (k = 128, n = 300) in 64-bit, and
the (square, namespace) query row. Both builds must run clean and report ok. The size entry
point is checked against the same closed form."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "index_batch_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
KS = [1, 2, 4, 8, 16, 32, 64]
NS = [1, 2, 3, 4, 5]


def _index_bytes(k):
    w = 2 * k
    return (w * w + 2 * w * (w - 1)) * 96 + 2 * w * 32 + 48


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_index_batch_check_sanitizer_clean(tmp_path):
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
        assert "FAIL" not in r.stdout and lines[-1] == "index batch check: ok", r.stdout[-2000:]
        assert len(lines) == len(KS) * len(NS) + 3
        shapes = [(k, n) for k in KS for n in NS]
        for (k, n), line in zip(shapes, lines):
            assert line.split() == ["k", "=", f"{k},", "n", "=", f"{n}:", str(n * _index_bytes(k)), "bytes"], line
        big = 299 * _index_bytes(128)
        assert big > 1 << 32
        assert lines[-3] == f"k = 128, n = 300: square 299 at index byte {big}, cell byte {299 * 256 * 256 * 512}"
        assert lines[-2] == "queries: squares 0 .. 65535 round-trip"


def test_batch_size_matches_single():
    """cel_dev_tree_index_batch_size is n times the single size; 0 for a width or a count the
    batch calls do not take."""
    import celestia_eds._lib as L
    lib = L.load()
    for k in (1, 2, 8, 32, 128, 512, 1024, 2048):  # every width the single size is given for
        single = lib.cel_dev_tree_index_size(k)
        assert single == _index_bytes(k) and single % 16 == 0
        for n in (1, 3, 67, 256, 65535):
            assert lib.cel_dev_tree_index_batch_size(k, n) == n * single
    for k in (0, 3, 4096):
        assert lib.cel_dev_tree_index_batch_size(k, 1) == 0
    assert lib.cel_dev_tree_index_batch_size(8, 0) == 0
    assert lib.cel_dev_tree_index_batch_size(8, 65536) == 0  # more squares than one call takes
    assert lib.cel_dev_prove_squares_workspace_size(0) > 0
    assert lib.cel_dev_prove_squares_workspace_size(1000) >= 40 * 1000
    assert lib.cel_dev_namespace_squares_workspace_size(8, 5) == lib.cel_dev_namespace_workspace_size(8, 5)
    assert lib.cel_dev_namespace_squares_workspace_size(3, 5) == 0
