"""CPU: tools/tx_parse_check.cpp, a stand-alone host program (its own main, csrc/tx_parse.hpp
alone, no HIP), built once with ASan + UBSan (no recovery, runtime linked statically: nothing is
preloaded and nothing is loaded into python) and once plain. It checks the tx parser's host-side
arithmetic: the uvarint reader and the parse step against a bytewise model for every 1-byte and
2-byte stream and the overflow edges, the cut of every 16-byte output chunk into its one or two
source shares for every first-share reserved value and both header sizes (every byte taken once,
every dword read inside its cell), the rule that accepts the shares' reserved bytes against the
sequential parse over every pattern of ten values per later share of short streams, and the
workspace carve. Both builds must run clean and report ok, with the counts worked out here
independently."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "tx_parse_check.cpp")
INC = os.path.join(ROOT, "celestia-app_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]
# the checker's streams: (first share's reserved value, share 1 a start share, unit lengths, bytes behind them)
STREAMS = [(38, False, [498, 998, 40], 0), (38, False, [100, 100, 100, 100, 300, 20, 600], 0), (38, False, [472], 0),
           (38, False, [472, 476], 0), (38, True, [472, 472, 30], 0), (38, False, [1500], 2),
           (38, False, [470, 1, 1, 1, 1, 700], 11), (38, False, [], 0), (0, False, [300, 400], 0),
           (100, False, [600, 5], 0), (511, False, [700, 9], 0)]


def _shares(r0, start1, lens, extra):
    """The shares a stream of that many bytes takes."""
    need = sum((1 if n < 128 else 2) + n for n in lens) + extra
    have, shares = (512 - r0 if r0 else 0), 1
    while have < need:
        have += 474 if (shares == 1 and start1) else 478
        shares += 1
    return shares


def _want():
    return ["uvarint: %d streams" % (256 + 65536 + 4 * 6 * 2 * 3),
            "chunks: %d" % (2 * 16 * (sum(512 - r for r in range(1, 512)) + 478 + 474)),
            "hints: %d patterns" % sum(10 ** (_shares(*s) - 1) for s in STREAMS),
            "carve: %d workspaces" % (7 * 3),
            "tx parse check: ok"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tx_parse_check_sanitizer_clean(tmp_path):
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
