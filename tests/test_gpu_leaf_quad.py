"""The batch commit's first kernel, k_leaf_quad: one lane hashes the four leaves of a 2x2
block of EDS cells and the two row and two column level-1 nodes over them. Every batch of
more than one square takes it (launch_commit, nmt_kernels.hip); one square keeps k_leaf and
k_level<true>. What can go wrong in it, and what the cases here aim at:

  - which cells are Q0 (their namespace is the share's) and which carry 0xFF*29, decided per
    cell of a block; at k = 1 one block holds all four kinds and its level-1 nodes are the roots;
  - which leaf is the left and which the right child of each of the four nodes, and where a
    node lands in the level-1 array (row tree / column tree, index);
  - HashNode's IgnoreMaxNamespace on a Q0 share that itself carries 0xFF*29;
  - the push-order check, whose neighbour may lie in the same block or in another one.

Every expectation is the CPU oracle's: status, row roots, column roots and DAH of the whole
square. Batches are three distinct squares, run as one chunk (CEL_FLAG_CALLER_STREAM, and
cel_dev_extend_only + cel_dev_commit_only), so all three go through the quad kernel.
"""
import numpy as np
import pytest

import test_gpu_order_check as oc
from eds_inputs import random_ods

NS, SHARE, NODE = oc.NS, oc.SHARE, oc.NODE
EORDER = oc.EORDER
MODES = ["caller", "commit"]  # one chunk each: launch_commit over all three squares

_WANT = {}


def want(oracle, key, ods, check_order=True):
    """(status, row roots, column roots, DAH) of the oracle for `ods`, once per key."""
    key = (key, check_order)
    if key not in _WANT:
        rc, rr, cr = oracle.roots(oracle.extend(ods), check_order=check_order)
        _WANT[key] = (rc, rr, cr, oracle.dah_hash(rr, cr))
    return _WANT[key]


def run3(ctx, odss, mode, flags):
    dev = oc.DevBatch(ctx, len(odss), odss.shape[1])
    dev.load(odss)
    return dev.run(mode, flags)


def assert_roots(got, wants, what):
    """Roots and DAH of every square against the oracle's, whatever its status."""
    _, rr, cr, dah = got
    for i, (_, w_rr, w_cr, w_dah) in enumerate(wants):
        assert np.array_equal(rr[i], w_rr), f"{what}: square {i} row roots"
        assert np.array_equal(cr[i], w_cr), f"{what}: square {i} column roots"
        assert dah[i].tobytes() == w_dah, f"{what}: square {i} DAH"


# ------------------------------------------------------------------------------------ sizes

def size_squares(k):
    """Three distinct valid squares of width k. At k = 1 the third one's only Q0 share
    carries 0xFF*29 itself."""
    odss = np.stack([random_ods(k, 7100 + 10 * k + i) for i in range(3)])
    if k == 1:
        odss[2, 0, 0, :NS] = 0xFF
    assert len({o.tobytes() for o in odss}) == 3
    return odss


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2, 4, 32])
def test_sizes(ctx, oracle, k, mode):
    """k = 1: a single block whose level-1 nodes are the four roots (the kernel writes the
    packed roots and the DAH leaf digests itself). k = 2, 4: the Q0 boundary falls on a block
    edge and a wave holds several block rows. k = 32: four 8x8 tiles of blocks per row band,
    the Q0 tiles and the parity tiles apart. With the push-order check on: status 0."""
    from celestia_eds import _lib
    odss = size_squares(k)
    wants = [want(oracle, ("size", k, i), odss[i]) for i in range(3)]
    assert [w[0] for w in wants] == [0, 0, 0]
    got = run3(ctx, odss, mode, _lib.FLAG_ORDER_CHECK)
    oc.assert_batch(*got, wants, f"k={k} {mode}")
    assert_roots(got, wants, f"k={k} {mode}")
    assert_roots(run3(ctx, odss, mode, 0), wants, f"k={k} {mode} unchecked")


# ------------------------------------------------------------------- namespace runs, k = 32

K = 32


def stepped(k, row_steps, col_steps, seed):
    """A valid square whose namespace rises by one grade at every row in row_steps (byte 28)
    and at every column in col_steps (byte 1): constant runs between the steps, ordered
    along every row and down every column."""
    ods = np.random.default_rng(seed).integers(0, 256, (k, k, SHARE), dtype=np.uint8)
    ods[:, :, :NS] = 0
    gr = sum((np.arange(k) >= t).astype(np.uint8) for t in row_steps) if row_steps else np.zeros(k, np.uint8)
    gc = sum((np.arange(k) >= t).astype(np.uint8) for t in col_steps) if col_steps else np.zeros(k, np.uint8)
    ods[:, :, 28] = 1 + gr[:, None]
    ods[:, :, 1] = 1 + gc[None, :]
    row, col = oc.violations(ods)
    assert not row.any() and not col.any()
    return ods


def run_squares():
    """inside: every step between the two rows / columns of a block (odd index), the last
    one at k - 1, so the last Q0 row and column are a run of their own up to k - 1 | k.
    edge: every step on a block edge (even index), 8 and 16 also on a tile edge.
    one_run: a single namespace over all of Q0, which ends at k - 1 | k."""
    k = K
    return np.stack([stepped(k, [1, 5, k - 1], [3, 9, k - 1], 7201),
                     stepped(k, [2, 8, 16], [6, 16, k - 2], 7202),
                     stepped(k, [], [], 7203)])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_namespace_runs_k32(ctx, oracle, mode):
    """Namespace runs that change inside a 2x2 block, on a block edge, and at k - 1 | k: the
    min / max namespaces of the level-1 nodes differ from node to node, in rows and columns."""
    from celestia_eds import _lib
    odss = run_squares()
    wants = [want(oracle, ("runs", i), odss[i]) for i in range(3)]
    assert [w[0] for w in wants] == [0, 0, 0]
    got = run3(ctx, odss, mode, _lib.FLAG_ORDER_CHECK)
    oc.assert_batch(*got, wants, f"runs {mode}")
    assert_roots(got, wants, f"runs {mode}")


# ------------------------------------------------- a Q0 share that carries 0xFF*29, k = 32

def parity_ns_squares():
    """Random valid squares with single Q0 shares set to the namespace 0xFF*29:
    0: one at each of the four positions of a block (four different blocks);
    1: the last Q0 cell of a row and the last Q0 cell of a column;
    2: the last Q0 cell of the last row, which is also the last of its column (a valid square)."""
    k = K
    odss = np.stack([random_ods(k, 7300 + i) for i in range(3)])
    for r, c in ((4, 6), (8, 11), (13, 20), (17, 25)):  # positions 00, 01, 10, 11
        odss[0, r, c, :NS] = 0xFF
    assert {(r & 1, c & 1) for r, c in ((4, 6), (8, 11), (13, 20), (17, 25))} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    odss[1, 5, k - 1, :NS] = 0xFF
    odss[1, k - 1, 9, :NS] = 0xFF
    odss[2, k - 1, k - 1, :NS] = 0xFF
    return odss


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_parity_namespace_in_q0(ctx, oracle, mode):
    """IgnoreMaxNamespace sees a Q0 share's own 0xFF*29: the level-1 node over it (and the
    nodes above) keep the left sibling's max. Roots and DAH without the push-order check
    against the oracle's unchecked roots; with the check, the oracle's status per square
    (a lower namespace after 0xFF*29 is a violation; the last cell of the square is not)."""
    from celestia_eds import _lib
    odss = parity_ns_squares()
    free = [want(oracle, ("pns", i), odss[i], check_order=False) for i in range(3)]
    assert_roots(run3(ctx, odss, mode, 0), free, f"parity ns {mode}")
    wants = [want(oracle, ("pns", i), odss[i]) for i in range(3)]
    assert [w[0] for w in wants] == [EORDER, EORDER, 0]
    oc.assert_batch(*run3(ctx, odss, mode, _lib.FLAG_ORDER_CHECK), wants, f"parity ns checked {mode}")


# -------------------------------------------------------------------- order violations, k = 32

ORDER_BATCHES = {
    # the offending pair inside one block: (6, 7) below its left neighbour (6, 6); (7, 6) below (6, 6) above it
    "inside": [("row", 6, 7), None, ("col", 7, 6)],
    # across two blocks: (6, 8) below (6, 7); (8, 6) below (7, 6); the same across a tile edge
    "across": [("row", 6, 8), ("col", 8, 6), None],
    "across_tiles": [None, ("col", 16, 15), ("row", 15, 16)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(ORDER_BATCHES))
def test_order_violations(ctx, oracle, name, mode):
    """CEL_EORDER per square of a batch of three: single row-only and column-only violations
    (test_gpu_order_check.lowered asserts that each square has exactly that one) whose pair
    lies inside one block or across two, and a valid square between them."""
    from celestia_eds import _lib
    k = K
    cases = ORDER_BATCHES[name]
    odss = np.stack([oc.lowered(k, *c) if c else oc.graded(k, "row" if i % 2 else "col")
                     for i, c in enumerate(cases)])
    wants = [want(oracle, ("order", c, i % 2), odss[i]) for i, c in enumerate(cases)]
    assert [w[0] for w in wants] == [EORDER if c else 0 for c in cases]
    got = run3(ctx, odss, mode, _lib.FLAG_ORDER_CHECK)
    oc.assert_batch(*got, wants, f"{name} {mode}")


# ------------------------------------------------------------------------------- one square

@pytest.mark.gpu
def test_one_square_host_call(ctx, oracle):
    """cel_extend_batch with n = 1 from host memory (one square: k_leaf and k_level<true>)
    gives the same roots as the batch gave for the same square."""
    from celestia_eds import _lib
    ods = np.ascontiguousarray(size_squares(K)[1])
    w = want(oracle, ("size", K, 1), ods)
    rc, st, rr, cr, dah = oc._one_square(ctx, ods, _lib.FLAG_ORDER_CHECK)
    assert rc == 0
    oc.assert_batch(st, rr, cr, dah, [w], "one square")


# --------------------------------------------------------------------------------- workspace

@pytest.mark.parametrize("k", [2, 32, 128, 512])
@pytest.mark.parametrize("n", [3, 128])
def test_batch_workspace_has_no_leaf_area(k, n):
    """A batch's workspace holds the levels from 1 up (W^2 / 2 + W^2 / 4 records of 96 bytes
    per square and tree family, plus a padding record per tree and level), the roots, the DAH
    leaf digests and the order flags: (1.5 W^2 + 6 W) * 96 + 64 W + 4 bytes per square, where
    the leaf area alone was W^2 * 96 more. A chunk of one square (n = 3 is split 2 + 1) keeps
    its leaf records. Each of a chunk's six areas and each chunk is aligned to 256 bytes."""
    import celestia_eds._lib as L
    lib = L.load()
    W = 2 * k
    per_sq = (3 * W * W // 2 + 6 * W) * 96 + 64 * W + 4
    leaf_one = W * W * 96 if n == 3 else 0
    ws = lib.cel_dev_workspace_size(k, n)
    assert n * per_sq <= ws <= n * per_sq + leaf_one + 16 * 256
