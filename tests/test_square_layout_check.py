"""CPU: tools/square_layout_check.cpp, a stand-alone host program (its own main, linked
with csrc/square.cpp, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. It
builds random and edge blocks, expands each cel_square_layout on the CPU in exactly sized
buffers and compares with cel_square_construct. Both builds must run clean and print the
same digest."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tools", "square_layout_check.cpp"),
       os.path.join(ROOT, "celestia-app_amd", "csrc", "square.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_square_layout_check_sanitizer_clean(tmp_path):
    out = {}
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-o", exe] + SRC, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.split("\n")
        assert lines[0] == "square layout check: ok", r.stdout[-2000:]
        out[name] = lines[1]
    assert len(out["san"]) == 16 and out["san"] == out["plain"]
