"""Checker for blob share commitments: go-square v1.1.0 inclusion.CreateCommitment restated
with hashlib, from the blob bytes (sparse share splitting included). Test code only: the
product computes every hash on the device."""
import hashlib
import math

NS = 29
SHARE = 512
FIRST = SHARE - NS - 1 - 4  # 478 data bytes in a blob's first share
CONT = SHARE - NS - 1       # 482 in the others
PARITY_NS = b"\xff" * NS


def _sha(b):
    return hashlib.sha256(b).digest()


def sparse_shares_needed(length):
    return 0 if length == 0 else 1 if length <= FIRST else 1 + -(-(length - FIRST) // CONT)


def split_blob(ns, data, share_version=0):
    """shares.SparseShareSplitter.Write: ns || info || [sequence length] || data, zero padded."""
    assert len(ns) == NS and len(data) > 0
    out, pos, first = [], 0, True
    while pos < len(data):
        head = ns + bytes([share_version << 1 | first]) + (len(data).to_bytes(4, "big") if first else b"")
        take = SHARE - len(head)
        out.append((head + data[pos:pos + take]).ljust(SHARE, b"\x00"))
        pos += take
        first = False
    return out


def leaf(share):
    ns = share[:NS]
    return ns + ns + _sha(b"\x00" + ns + share)


def node(l, r):
    lmin, lmax, rmin, rmax = l[:NS], l[NS:2 * NS], r[:NS], r[NS:2 * NS]
    mx = lmax if rmin == PARITY_NS else max(lmax, rmax)  # IgnoreMaxNamespace
    return lmin + mx + _sha(b"\x01" + l + r)


def nmt_root(shares):
    level = [leaf(s) for s in shares]
    while len(level) > 1:
        level = [node(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
    return level[0]


def rfc6962(items):
    """merkle.HashFromByteSlices: split at the largest power of two below the count."""
    if len(items) == 1:
        return _sha(b"\x00" + items[0])
    k = 1
    while k * 2 < len(items):
        k *= 2
    return _sha(b"\x01" + rfc6962(items[:k]) + rfc6962(items[k:]))


def _pow2ceil(n):
    return 1 << (n - 1).bit_length()


def subtree_width(n, threshold=64):
    return min(_pow2ceil(-(-n // threshold)), _pow2ceil(math.isqrt(n - 1) + 1))


def mountain_range(n, w):
    sizes, left = [], n
    while left:
        t = w if left >= w else 1 << (left.bit_length() - 1)
        sizes.append(t)
        left -= t
    return sizes


def commitment_of_shares(shares, threshold=64):
    roots, c = [], 0
    for t in mountain_range(len(shares), subtree_width(len(shares), threshold)):
        roots.append(nmt_root(shares[c:c + t]))
        c += t
    return rfc6962(roots)


def create_commitment(ns, data, share_version=0, threshold=64):
    return commitment_of_shares(split_blob(ns, data, share_version), threshold)


def blob_len_for_shares(n):
    """The largest blob length that needs exactly n shares."""
    return FIRST + CONT * (n - 1)


# --- inputs the commitment tests share ----------------------------------------------------

def random_namespace(rng):
    """A version-0 namespace: 18 zero bytes, then 10 random ones (rng: numpy Generator)."""
    return bytes(19) + rng.integers(0, 256, 10, "uint8").tobytes()


def random_bytes(rng, n):
    return rng.integers(0, 256, n, "uint8").tobytes()


def rfc_level_sizes(count, lds=1024):
    """The digest counts of the bottom-up RFC-6962 levels (an unpaired last node moves up)
    from `count` down to the first that is at most `lds`."""
    sizes = [count]
    while sizes[-1] > lds:
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


# --- the reference-held vector: block 408's blob tx -------------------------------------

def _fields(buf):
    """protobuf fields of a message: [(number, wire type, value)] (varint or bytes)."""
    out, i = [], 0

    def varint():
        nonlocal i
        v = s = 0
        while True:
            b = buf[i]
            i += 1
            v |= (b & 0x7F) << s
            s += 7
            if not b & 0x80:
                return v

    while i < len(buf):
        key = varint()
        num, wire = key >> 3, key & 7
        if wire == 0:
            out.append((num, wire, varint()))
        elif wire == 2:
            n = varint()
            out.append((num, wire, bytes(buf[i:i + n])))
            i += n
        elif wire == 5:
            i += 4
        elif wire == 1:
            i += 8
        else:
            raise ValueError("wire type")
    return out


def _first(fields, num):
    return next(v for n, _, v in fields if n == num)


def blob_tx_blobs(tx):
    """The blobs of a BlobTx, in order: [(ns29, data, share_version)]."""
    blobs = []
    for n, _, v in _fields(tx):
        if n == 2:
            f = _fields(v)
            ns_id = _first(f, 1)
            ver = next((x for m, _, x in f if m == 4), 0)
            blobs.append((bytes([ver]) + ns_id, _first(f, 2), next((x for m, _, x in f if m == 3), 0)))
    return blobs


def blob_tx_parts(tx):
    """A BlobTx -> (blobs [(ns29, data, share_version)], signed share_commitments): BlobTx.tx
    -> Tx.body -> TxBody.messages[0] (Any) -> MsgPayForBlobs.share_commitments (field 4)."""
    top = _fields(tx)
    blobs = blob_tx_blobs(tx)
    body = _first(_fields(_first(top, 1)), 1)
    msg = _first(_fields(_first(_fields(body), 1)), 2)
    return blobs, [v for n, _, v in _fields(msg) if n == 4]
