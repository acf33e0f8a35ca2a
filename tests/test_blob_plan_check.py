"""CPU: tools/blob_plan_check.cpp, a stand-alone host program (its own main, header-only
csrc/blob_plan.hpp, no HIP), built once with ASan + UBSan (no recovery, runtime linked
statically: nothing is preloaded and nothing is loaded into python) and once plain. It plans
the batches the GPU commitment tests run (widths 256 and 1024, width-1 root counts round the
commit kernel's switches, mixed random batches at thresholds 1, 5, 64 and 1000) in exactly
sized tables and checks the slot layout and root_at against MerkleMountainRangeSizes. Both
builds must run clean and report ok."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "blob_plan_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_blob_plan_check_sanitizer_clean(tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name, flags in (("san", ["-g", "-O1"] + SAN), ("plain", ["-O2"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17"] + flags + ["-I", INC, "-o", exe, SRC], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, f"{name} exit {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout.split("\n")[0] == "blob plan check: ok", r.stdout[-2000:]
