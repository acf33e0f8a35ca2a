"""Compact shares for the tx parser tests (test_tx_parse.py on the host, test_gpu_txs.py on the
device): hand-made shares, one per rule of the definition in include/celestia_eds.h ("txs by
range"), each with its expected result written out, and unit lists chosen by byte for the honest
builder (oracle/square_layout.compact_shares)."""
import numpy as np

import square_layout as SL

SHARE = 512
TX_NS = bytes(28) + b"\x01"
PFB_NS = bytes(28) + b"\x04"
BLOB_NS = bytes(19) + b"\x07" * 10
EVERSION, ENAMESPACE, ERESERVED, EVARINT = 1, 2, 3, 4


def uvarint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n >> 7 else 0))
        n >>= 7
        if not n:
            return bytes(out)


def share(ns, start, reserved, payload=b"", version=0, seq_len=0, tail=b""):
    """A compact share: namespace, info byte, the sequence length of a start share, the reserved
    bytes, then the payload; zeros up to 512 bytes, or up to `tail`, which ends the share."""
    sh = ns + bytes([version << 1 | start]) + (seq_len.to_bytes(4, "big") if start else b"")
    sh += reserved.to_bytes(4, "big") + payload
    assert len(sh) + len(tail) <= SHARE
    return sh + bytes(SHARE - len(sh) - len(tail)) + tail


def unit(data):
    return uvarint(len(data)) + data


FULL = bytes(range(256)) + bytes(range(216))  # 472 bytes: with its 2-byte prefix a start share's 474

# (name, shares, status, units): what the definition gives, worked out by hand.
HAND = [
    # the first share's reserved value
    ("first share R = 0 gives no bytes", [share(TX_NS, 1, 0, unit(b"abc"))], 0, []),
    ("first share R = 0, the stream begins in the second",
     [share(TX_NS, 1, 0, unit(b"abc")), share(TX_NS, 0, 34, unit(b"de"))], 0, [b"de"]),
    # bytes 5 .. 27 of a compact namespace are zero: the stream begins with a length of 0
    ("first share R = 5 reads the namespace's zeros", [share(TX_NS, 1, 5, unit(b"abc"))], 0, []),
    # R = 34 < h = 38 on a start share: the stream begins with the reserved bytes 00 00 00 22
    ("first share R = 34 below h = 38 reads the reserved bytes", [share(TX_NS, 1, 34, unit(b"abc"))], 0, []),
    ("first share a continuation with R = 34", [share(TX_NS, 0, 34, unit(b"abc"))], 0, [b"abc"]),
    ("first share R = 511 gives one byte",
     [share(TX_NS, 1, 511, tail=b"\x02"), share(TX_NS, 0, 0, b"hi")], 0, [b"hi"]),
    ("first share R = 512", [share(TX_NS, 1, 512, unit(b"abc"))], ERESERVED, []),
    # the units
    ("padded varint 81 00 is skipped by its canonical length",
     [share(TX_NS, 1, 38, b"\x81\x00" + unit(b"xy"))], 0, [b"\x00", b"xy"]),
    ("11-byte varint", [share(TX_NS, 1, 38, unit(b"a") + b"\x80" * 10 + b"\x01")], EVARINT, []),
    ("10th varint byte above 1", [share(TX_NS, 1, 38, unit(b"a") + b"\xff" * 9 + b"\x02")], EVARINT, []),
    ("L = 2^64 - 1 is a cut unit", [share(TX_NS, 1, 38, unit(b"a") + b"\xff" * 9 + b"\x01" + b"z" * 40)], 0, [b"a"]),
    ("cut last unit", [share(TX_NS, 1, 38, unit(b"a") + uvarint(600) + b"q" * 400)], 0, [b"a"]),
    ("unit that ends with the stream", [share(TX_NS, 1, 38, unit(b"a") + uvarint(470) + b"q" * 470)], 0,
     [b"a", b"q" * 470]),
    ("zero padding stops before a PFB start share",
     [share(TX_NS, 1, 38, unit(b"abc")), share(PFB_NS, 1, 38, unit(b"wxyz"))], 0, [b"abc"]),
    ("full tx share continues into a start share",
     [share(TX_NS, 1, 38, unit(FULL)), share(PFB_NS, 1, 38, unit(b"wxyz"))], 0, [FULL, b"wxyz"]),
    # the status order
    ("version 1 behind a blob namespace", [share(BLOB_NS, 1, 38, unit(b"abc")), share(TX_NS, 0, 0, version=1)],
     EVERSION, []),
    ("version 1 behind R = 512", [share(TX_NS, 1, 512), share(TX_NS, 0, 0, version=1)], EVERSION, []),
    ("blob namespace behind R = 512", [share(TX_NS, 1, 512), share(BLOB_NS, 0, 0)], ENAMESPACE, []),
    ("blob namespace", [share(TX_NS, 1, 38, unit(b"abc")), share(BLOB_NS, 0, 0)], ENAMESPACE, []),
    ("a varint error does not outrank the namespace",
     [share(TX_NS, 1, 38, b"\x80" * 11), share(BLOB_NS, 0, 0)], ENAMESPACE, []),
]


def pattern(n, salt):
    return bytes((i * 7 + salt) & 0xFF for i in range(n))


EDGE_LENGTHS = [1, 127, 128, 473, 474, 475, 951, 952, 16383, 16384]
# name -> units for the honest builder
HONEST = {
    "edge lengths": [pattern(n, n) for n in EDGE_LENGTHS],
    "ends on a share's last byte": [FULL, pattern(5, 1)],
    # 2 + 471 bytes leave the first share one byte: the first of a 2-byte prefix
    "2-byte varint split across two shares": [pattern(471, 2), pattern(300, 3)],
    "239 one-byte units in one share": [FULL] + [bytes([i]) for i in range(239)],
    "a unit over more than 3 shares": [pattern(1500, 4), pattern(9, 5)],
}
for _n in EDGE_LENGTHS:
    HONEST[f"length {_n}"] = [pattern(_n, _n + 1)]


# The stream of the hint tests: four shares, units beginning at stream bytes 0, 500 (share 1,
# byte 60) and 1500 (share 3, byte 104); no unit begins in share 2.
HINT_UNITS = [pattern(498, 1), pattern(998, 2), pattern(40, 3)]
# A stream that still parses into units when its first share gives nothing: the first share is
# filled by a unit and the prefix of a second one whose 600 bytes are 200 units of their own;
# they begin in share 1, which names none (R = 0), and end in share 2 (R = 156).
NESTED_UNITS = [pattern(470, 6), b"\x02zz" * 200, pattern(50, 7)]


def with_reserved(shares, j, r):
    """`shares` with the reserved value of share j replaced."""
    at = 34 if shares[j][29] & 1 else 30
    out = list(shares)
    out[j] = out[j][:at] + r.to_bytes(4, "big") + out[j][at + 4:]
    return out


# (name, stream, share, reserved value): honest streams with one hint damaged; each must parse as
# before, but for the last, whose stream begins elsewhere, and be flagged.
DAMAGED_HINTS = [
    ("R one too high", HINT_UNITS, 1, 61),
    ("R one too low", HINT_UNITS, 3, 103),
    ("R = 0 where a unit begins", HINT_UNITS, 1, 0),
    ("R != 0 where none begins", HINT_UNITS, 2, 40),
    ("R < h", HINT_UNITS, 1, 33),
    ("R >= 512 on a later share", HINT_UNITS, 3, 512),
    ("the first share has R = 0", NESTED_UNITS, 0, 0),
]


def corpus(seed, n=300):
    """n damaged compact runs: honest runs of 1 .. 6 shares of the tx namespace, a PFB start share
    behind some, with 1 .. 3 bits flipped (a third of them in bytes 26 .. 41 of a share: the
    namespace's end, the info byte, the reserved bytes) or with shares cut off at either end. The
    units' bytes are 0x80 and above, so that a parse that has lost its place soon meets a varint
    that overflows. Seed 1 gives 1000 shares: one 32 x 32 square. -> [list of 512-byte shares]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        want = int(rng.integers(1, 7))
        units = []
        while len(SL.compact_shares(TX_NS, units)) < want or not units:
            size = int(rng.choice([1, 3, 40, 130, 300, 700]))
            units.append((rng.integers(0x80, 0x100, size, np.uint8)).tobytes())
        shares = SL.compact_shares(TX_NS, units)[:want]
        if want < 6 and rng.integers(0, 4) == 0:
            shares.append(share(PFB_NS, 1, 38, unit(b"\x90" * 20)))
        a = np.frombuffer(b"".join(shares), np.uint8).reshape(-1, SHARE).copy()
        if rng.integers(0, 5) == 0 and len(a) > 1:  # a truncated range
            cut = int(rng.integers(1, len(a)))
            a = a[cut:] if rng.integers(0, 2) else a[:cut]
        else:
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(0, len(a)))
                byte = int(rng.integers(26, 42)) if rng.integers(0, 3) == 0 else int(rng.integers(0, SHARE))
                a[j, byte] ^= 1 << int(rng.integers(0, 8))
        out.append([a[j].tobytes() for j in range(len(a))])
    return out


CORPUS_SEED = 1


def honest(ns, units):
    return SL.compact_shares(ns, units)


def as_array(shares):
    return np.frombuffer(b"".join(shares), np.uint8).reshape(-1, SHARE)
