"""CPU: the fraud-proof entry points are exported, declared in the header and bound, the verdict
codes agree between header and binding, and the calls reject what they can without a device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "celestia_eds.h")
LIB = os.path.join(ROOT, "celestia-app_amd", "libcelestia_eds.so")
SYMBOLS = ["cel_befp_verify_batch", "cel_dev_befp_build", "cel_befp_build"]


def test_befp_symbols_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    text = open(HEADER).read()
    import celestia_eds._lib as L
    lib = L.load()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"^cel_status " + name + r"\(", text, re.M), name
        assert name in L.EXPORTS and hasattr(lib, name)


def test_befp_verdict_codes_match_header():
    import celestia_eds._lib as L
    from celestia_eds import fraud
    codes = dict(re.findall(r"^#define CEL_BEFP_([A-Z_]+) (\d+)", open(HEADER).read(), re.M))
    assert set(codes) == {"NOT_FRAUD", "FRAUD", "BAD_SHARE", "TOO_FEW", "MALFORMED"}
    assert {k: int(v) for k, v in codes.items()} == {k: getattr(L, "BEFP_" + k) for k in codes}
    assert L.BEFP_NOT_FRAUD == 0 and len(set(codes.values())) == 5
    assert fraud.BEFP_FRAUD == L.BEFP_FRAUD


def test_befp_calls_validate_without_a_device():
    import celestia_eds._lib as L
    lib = L.load()
    z = ctypes.c_uint32()
    assert lib.cel_befp_verify_batch(None, 0, 2, *([None] * 12)) == L.EINVAL
    assert lib.cel_dev_befp_build(None, None, None, 2, None, None, 0, 0, None, None, None, None, ctypes.byref(z)) == L.EINVAL
    assert lib.cel_befp_build(None, None, None, 2, None, None, 0, 0, None, None, None, None, ctypes.byref(z)) == L.EINVAL
