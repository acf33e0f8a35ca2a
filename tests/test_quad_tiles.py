"""CPU: tools/quad_tiles_check.cpp, a stand-alone host program (its own main, header-only
csrc/quad_tiles.hpp, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. For
k = 16, 32, 64, 128, 256 and 512 it walks both leaf launches of a batch lane by lane, as
k_leaf_quad_q0 and k_leaf_quad_par index them, into a table of exactly the (k/8) x (k/8) tile
grid and checks that every tile is produced exactly once over the two classes, that a Q0
tile has both block coordinates below k/2 and no parity tile has, that every block coordinate
is below k, and that each launch grid covers its class with fewer than 256 surplus lanes.
Both builds must run clean and report ok."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "quad_tiles_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
WIDTHS = [16, 32, 64, 128, 256, 512]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_quad_tiles_check_sanitizer_clean(tmp_path):
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
        assert "FAIL" not in r.stdout and lines[-1] == "quad tiles check: ok", r.stdout[-2000:]
        # one line per width, with the class sizes: h^2 and 3 h^2 tiles for h = k / 16
        assert len(lines) == len(WIDTHS) + 1
        for k, line in zip(WIDTHS, lines):
            h = k // 16
            assert line.split()[:7] == ["k", "=", f"{k}:", str(h * h), "Q0", "tiles", "in"], line
            assert f" {3 * h * h} parity tiles " in line, line
