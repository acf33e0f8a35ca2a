"""Hand-made sparse shares for the blob parser's tests (test_blob_parse.py on the host,
test_gpu_blobs.py on the device): block_inputs.expand of a hand-made layout, then byte edits.
A case gives its shares and either the error kind of parseSparseShares or the blobs it returns,
written down here from the layout, not computed by a parser."""
import numpy as np

import block_inputs as B

EVERSION, ENOSTART, ESHORT = 1, 2, 3
INFO, LEN = B.NS, B.NS + 1  # the info byte; the big-endian sequence length of a start share


def blob_shares(lengths, seed):
    """-> (shares of the blobs alone [n][512], [(ns, data, first share, shares)])"""
    raw, segs = B.blob_layout(lengths, 64, seed)
    segs = [s for s in segs if s.kind == B.SEG_BLOB]
    n = segs[-1].start + segs[-1].count
    shares = B.expand(raw, 64, segs, None)[:n].copy()
    return shares, [(bytes(s.ns)[:B.NS], raw[s.off:s.off + s.len], s.start, s.count) for s in segs]


def padding(ns, n=1):
    """Namespace padding (a sequence start of length 0) or, with the padding namespaces, tail /
    primary reserved padding."""
    out = np.zeros((n, B.SHARE), np.uint8)
    out[:, :B.NS] = np.frombuffer(ns, np.uint8)
    out[:, INFO] = 1
    return out


def set_len(share, n):
    share[LEN:LEN + 4] = np.frombuffer(int(n).to_bytes(4, "big"), np.uint8)


class Case:
    def __init__(self, name, build, error=0):
        self.name, self._build, self.error = name, build, error

    def shares(self):
        return self._build()[0]

    def want(self):
        return self._build()[1]


def _continuation_first():
    sh, _ = blob_shares([1000], 11)
    return sh[1:], None


def _one_beyond():
    sh, _ = blob_shares([B.FIRST + B.CONT], 12)  # two full shares
    set_len(sh[0], B.FIRST + B.CONT + 1)
    return sh, None


def _trimmed():
    sh, blobs = blob_shares([1400], 13)  # three shares
    set_len(sh[0], 500)
    ns, data, _, _ = blobs[0]
    return sh, [(ns, data[:500], 0, 3)]


def _ns_padding_between():
    sh, blobs = blob_shares([600, 300], 14)
    (ns0, d0, _, _), (ns1, d1, _, _) = blobs
    out = np.concatenate([sh[:2], padding(ns0, 2), sh[2:]])
    return out, [(ns0, d0, 0, 2), (ns1, d1, 4, 1)]


def _padding_inside():
    sh, blobs = blob_shares([1000], 15)
    ns, data, _, _ = blobs[0]
    out = np.concatenate([sh[:1], padding(ns), padding(B.PRIMARY_PAD_NS), padding(B.TAIL_PAD_NS), sh[1:]])
    return out, [(ns, data, 0, 3)]


def _tail_only():
    return padding(B.TAIL_PAD_NS, 4), []


def _empty():
    return np.zeros((0, B.SHARE), np.uint8), []


def _other_namespace():
    sh, blobs = blob_shares([1000, 20], 16)
    (ns0, d0, _, _), (ns1, d1, _, _) = blobs
    sh[1, :B.NS] = np.frombuffer(bytes(19) + b"\xab" * 10, np.uint8)
    return sh, [(ns0, d0, 0, 3), (ns1, d1, 3, 1)]


def _len_max():
    sh, _ = blob_shares([700, 30], 17)
    set_len(sh[0], 0xFFFFFFFF)
    return sh, None


def _version_in_padding():
    sh, _ = blob_shares([100], 18)
    pad = padding(B.TAIL_PAD_NS)
    pad[0, INFO] = (1 << 1) | 1
    return np.concatenate([sh, pad]), None


def _version_after_start():
    sh, _ = blob_shares([1000], 19)
    sh[1, INFO] = 2 << 1
    return sh, None


def _continuation_before_version():
    sh, _ = blob_shares([1000, 40], 20)
    sh[2, INFO] |= 1 << 1
    return sh[1:], None


def _trailing_extra_share():
    """More shares than the length needs at the end of the range: trimmed."""
    sh, blobs = blob_shares([1400], 21)
    set_len(sh[0], 1)
    ns, data, _, _ = blobs[0]
    return sh, [(ns, data[:1], 0, 3)]


CASES = [Case("continuation_first", _continuation_first, ENOSTART),
         Case("length_one_beyond", _one_beyond, ESHORT),
         Case("length_shorter_is_trimmed", _trimmed),
         Case("namespace_padding_between_blobs", _ns_padding_between),
         Case("padding_between_start_and_continuation", _padding_inside),
         Case("tail_padding_only", _tail_only),
         Case("empty_range", _empty),
         Case("continuation_of_another_namespace", _other_namespace),
         Case("length_0xffffffff", _len_max, ESHORT),
         Case("bad_version_in_padding", _version_in_padding, EVERSION),
         Case("bad_version_after_start", _version_after_start, EVERSION),
         Case("continuation_before_bad_version", _continuation_before_version, ENOSTART),
         Case("one_byte_in_three_shares", _trailing_extra_share)]
