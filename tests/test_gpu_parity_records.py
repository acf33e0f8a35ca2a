"""The batch commit's split levels (nmt_kernels.hip): a node whose subtree lies outside Q0 is
known from its position (tree, index, level), kept as its 32-byte digest and hashed by
hash_parity_node (nmt_device.hpp) from a message whose 30 literal words are folded at compile
time; Q0 nodes stay 96-byte records under hash_node; a mixed tree's root joins the two.
What can go wrong, and the smallest widths at which it can:

  k = 1       the ROOTS path: the join is inside the one 2x2 block, all through hash_node
  k = 2       level 1 has one Q0 node and one parity node per mixed tree: the join is level 2
  k = 4, 8    a wave's tile mixes Q0 and parity lanes: the class is taken per lane
  k = 16      the first width whose tiles are wholly inside or outside Q0
  k = 32      several tiles per quadrant; the Q0 and the parity lanes of a level end in partial
              workgroups (level 2: 512 Q0 nodes, 1536 parity nodes; the roots: 64 + 64 lanes)

Every batch goes through cel_dev_extend_batch as one chunk (CEL_FLAG_CALLER_STREAM), two or
three squares, so every square takes the quad kernel and the split levels. Row roots, column
roots, DAH and status are the oracle's extend_and_commit; for a square that breaks the push
order the oracle's call refuses it (CEL_EORDER) and the roots are oracle.roots without the
check. The device's bad_axis word is not visible through the C ABI: the status is what it
becomes.
"""
import hashlib
import os
import re
import struct

import numpy as np
import pytest

import test_gpu_order_check as oc
from eds_inputs import random_ods

NS, SHARE, NODE = oc.NS, oc.SHARE, oc.NODE
EORDER = oc.EORDER
WIDTHS = [1, 2, 4, 8, 16, 32]

_WANT = {}


def want(oracle, key, ods):
    """(status, row roots, column roots, DAH) of the oracle for `ods`, once per key: the
    status is extend_and_commit's (0, or CEL_EORDER when it refuses the square); a refused
    square's roots and DAH are those of oracle.roots without the push-order check."""
    if key not in _WANT:
        try:
            _, rr, cr, dah = oracle.extend_and_commit(ods, want_eds=False)
            rc = 0
        except ValueError as e:
            assert f"rc={EORDER}" in str(e), e
            rc, (_, rr, cr) = EORDER, oracle.roots(oracle.extend(ods), check_order=False)
            dah = oracle.dah_hash(rr, cr)
        _WANT[key] = (rc, rr, cr, dah)
    return _WANT[key]


def run(ctx, odss, flags):
    dev = oc.DevBatch(ctx, len(odss), odss.shape[1])
    dev.load(odss)
    return dev.run("caller", flags)


def assert_all(got, wants, what, checked):
    """Roots and DAH of every square, refused or not; the status with the check on (the
    oracle's) and off (0)."""
    st, rr, cr, dah = got
    assert st.tolist() == [w[0] if checked else 0 for w in wants], f"{what}: status"
    for i, (_, w_rr, w_cr, w_dah) in enumerate(wants):
        assert np.array_equal(rr[i], w_rr), f"{what}: square {i} row roots"
        assert np.array_equal(cr[i], w_cr), f"{what}: square {i} column roots"
        assert dah[i].tobytes() == w_dah, f"{what}: square {i} DAH"


def both_ways(ctx, oracle, name, odss):
    from celestia_eds import _lib
    wants = [want(oracle, (name, i), odss[i]) for i in range(len(odss))]
    assert_all(run(ctx, odss, _lib.FLAG_ORDER_CHECK), wants, f"{name} checked", True)
    assert_all(run(ctx, odss, 0), wants, f"{name} unchecked", False)
    return wants


# ------------------------------------------------------------------------------------ shapes

@pytest.mark.gpu
@pytest.mark.parametrize("nsq", [2, 3])
@pytest.mark.parametrize("k", WIDTHS)
def test_shapes(ctx, oracle, k, nsq):
    """Random sorted namespaces (the reference's test factory), distinct squares."""
    odss = np.stack([random_ods(k, 8100 + 10 * k + i) for i in range(nsq)])
    assert len({o.tobytes() for o in odss}) == nsq
    wants = both_ways(ctx, oracle, f"shape k={k} n={nsq}", odss)
    assert [w[0] for w in wants] == [0] * nsq


# -------------------------------------------------------------------------------------- data

def max_at_edges(k, seed):
    """A random sorted square whose last Q0 row and last Q0 column carry the largest
    namespace present (one above the largest drawn): every mixed tree's Q0 half ends in it,
    so the join's max namespace is the Q0 half's and not the parity half's 0xFF*29."""
    ods = random_ods(k, seed).copy()
    top = bytes(18) + b"\x01" + bytes(10)  # above every version-0 namespace 0x00 || 0x00*18 || id(10)
    assert max(bytes(n) for n in ods[:, :, :NS].reshape(-1, NS)) < top
    ods[k - 1, :, :NS] = np.frombuffer(top, np.uint8)
    ods[:, k - 1, :NS] = np.frombuffer(top, np.uint8)
    row, col = oc.violations(ods)
    assert not row.any() and not col.any()
    return ods


def all_parity_namespace(k, seed):
    """Every Q0 share carries 0xFF*29: by value every node of the square looks like a parity
    node; by position the Q0 nodes are records under hash_node all the same."""
    ods = random_ods(k, seed).copy()
    ods[:, :, :NS] = 0xFF
    return ods


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_namespaces_at_the_join(ctx, oracle, k):
    odss = np.stack([max_at_edges(k, 8300 + k), all_parity_namespace(k, 8400 + k), random_ods(k, 8500 + k)])
    wants = both_ways(ctx, oracle, f"join k={k}", odss)
    assert [w[0] for w in wants] == [0, 0, 0]
    # the max namespace of a mixed tree's root is the edge namespace, not 0xFF*29
    edge = odss[0, k - 1, k - 1, :NS]
    assert np.array_equal(wants[0][1][0, NS:2 * NS], edge) and np.array_equal(wants[0][2][0, NS:2 * NS], edge)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 16, 32])
def test_order_violations(ctx, oracle, k):
    """One row-only violation in a Q0 row, a valid square, one column-only violation in a Q0
    column (test_gpu_order_check.lowered asserts that each square has exactly that one)."""
    odss = np.stack([oc.lowered(k, "row", k // 2, k - 1), oc.graded(k, "col"), oc.lowered(k, "col", k - 1, k // 2 - 1)])
    wants = both_ways(ctx, oracle, f"order k={k}", odss)
    assert [w[0] for w in wants] == [EORDER, 0, EORDER]


# ----------------------------------------------------------------------- two batches in flight

@pytest.mark.gpu
def test_two_batches_on_caller_streams(oracle):
    """k = 16, two batches of three squares on their own streams and workspaces, stepped in
    turn twice each (the second step of a batch waits for the other batch's extension)."""
    import torch
    from celestia_eds.device import SquareBatch
    k, B = 16, 3
    distinct = [random_ods(k, 8100 + 10 * k + i) for i in range(3)] + [max_at_edges(k, 8300 + k)]
    keys = [(f"shape k={k} n=3", i) for i in range(3)] + [(f"join k={k}", 0)]
    wants = [want(oracle, key, d) for key, d in zip(keys, distinct)]
    sbs = []
    for j in range(2):
        sb = SquareBatch(B, k, ods_in_eds=True)
        sb.load_ods(torch.from_numpy(np.stack([distinct[(i + j) % 4] for i in range(B)])))
        sb.status.fill_(0x7F7F7F7F)
        sbs.append(sb)
    torch.cuda.synchronize()
    for i in range(4):
        sbs[i % 2].extend_and_commit(caller_stream=True)
    torch.cuda.synchronize()
    for j, sb in enumerate(sbs):
        got = (sb.status.cpu().numpy(), sb.row_roots.cpu().numpy(), sb.col_roots.cpu().numpy(), sb.dah.cpu().numpy())
        assert_all(got, [wants[(i + j) % 4] for i in range(B)], f"batch {j}", True)


# ------------------------------------------------------------ the literal words, no GPU needed

def _table():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "celestia-app_amd", "csrc",
                       "nmt_device.hpp")
    with open(src) as f:
        body = re.search(r"kParNodeWords\[48\]\s*=\s*\{(.*?)\};", f.read(), re.S).group(1)
    return [int(np.prod([int(f.strip().rstrip("u"), 0) for f in t.split("*")])) for t in body.split(",")]


def _perm(s0, s1, sel):
    """v_perm_b32: result byte b is byte sel[b] of {s0:s1} (0-3 s1, 4-7 s0, 12 zero)."""
    src = struct.pack("<II", s1, s0)
    return int.from_bytes(bytes(0 if (sel >> 8 * b) & 0xFF == 12 else src[(sel >> 8 * b) & 0xFF] for b in range(4)),
                          "little")


def _node_word(L, R, q):
    """nmt_device.hpp's node_word over two records of 24 little-endian dwords."""
    if q == 0:
        return _perm(1, L[0], 0x04000102)
    if q <= 21:
        return _perm(L[q - 1], L[q], 0x07000102)
    if q == 22:
        return _perm(L[21], L[22], 0x0700010C) | (R[0] & 0xFF)
    if q <= 44:
        return _perm(R[q - 23], R[q - 22], 0x05060700)
    if q == 45:
        return _perm(R[22], 0x80, 0x05000C0C)
    return 181 * 8 if q == 47 else 0


def _record(digest):
    return list(struct.unpack("<24I", b"\xff" * 58 + digest + bytes(6)))


def _padded(dl, dr):
    msg = b"\x01" + b"\xff" * 58 + dl + b"\xff" * 58 + dr
    assert len(msg) == 181
    msg += b"\x80" + bytes(192 - 8 - 182) + struct.pack(">Q", 181 * 8)
    return list(struct.unpack(">48I", msg))


def test_literal_words():
    """kParNodeWords is the padded message 0x01 || 0xFF*58 || dl || 0xFF*58 || dr with both
    digests zero, word for word what node_word makes of two all-0xFF records; digest bytes
    reach exactly words 14..22 and 37..45; with digests in place the words are HashNode's
    message 0x01 || L || R again."""
    tab = _table()
    assert len(tab) == 48
    zero, ones = bytes(32), b"\xff" * 32
    assert tab == _padded(zero, zero)
    assert tab == [_node_word(_record(zero), _record(zero), q) for q in range(48)]
    full = _padded(ones, ones)
    assert [q for q in range(48) if full[q] != tab[q]] == list(range(14, 23)) + list(range(37, 46))
    assert all(tab[q] & ~full[q] == 0 for q in range(48))  # the digest bits are or-ed in
    dl, dr = hashlib.sha256(b"l").digest(), hashlib.sha256(b"r").digest()
    words = [_node_word(_record(dl), _record(dr), q) for q in range(48)]
    assert words == _padded(dl, dr)
    node = b"\x01" + b"\xff" * 58 + dl + b"\xff" * 58 + dr  # 0x01 || L(90) || R(90)
    assert struct.pack(">48I", *words)[:181] == node
