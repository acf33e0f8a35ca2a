"""CPU: tools/blob_parse_check.cpp, a stand-alone host program (its own main,
csrc/blob_parse.hpp alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. It checks the
blob parser's host-side arithmetic: the status of a range against a share-by-share walk for every
sequence of up to 8 share classes, the shortness test up to a declared length of 0xFFFFFFFF, the
cut of every 16-byte output chunk into its one or two source shares (every byte taken once, every
dword read inside its cell), the range checks and offsets, and the workspace carve. Both builds
must run clean and report ok, with the counts worked out here independently."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "blob_parse_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
CHUNK_LENGTHS = [1, 15, 16, 17, 477, 478, 479, 480, 481, 959, 960, 961, 1442, 1443, 6000, 70000]
OFFSET_LENGTHS = [1, 16, 17, 478, 70000, 2]


def _want():
    pad16 = lambda n: (n + 15) // 16 * 16
    return ["walk: %d sequences" % sum(4 ** n for n in range(9)),
            "short: %d lengths" % (40 * 5),
            "chunks: %d" % sum((n + 15) // 16 for n in CHUNK_LENGTHS),
            "ranges: %d positions" % (21 + sum(pad16(n) for n in OFFSET_LENGTHS) // 16),
            "carve: %d workspaces" % (7 * 3),
            "blob parse check: ok"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_blob_parse_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, "-o", exe, SRC],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert "FAIL" not in r.stdout, r.stdout[-2000:]
        assert r.stdout.strip().split("\n") == _want(), r.stdout[-2000:]
