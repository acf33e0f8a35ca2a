"""GPU: the batched NMT proof verifier (csrc/nmt_verify.hip through cel_nmt_verify_batch and
cel_dev_nmt_verify_batch) against the host mirror in celestia_eds/proof.py, which
tests/test_proof.py pins to the reference's vectors. An exception inside the mirror counts
as "reject".

A range proof carries one namespace for all its leaves, so a range accepts only where its
leaves share one: on a row that runs from Q0 into the parity half, ranges that cross column k
reject in the mirror and on the device alike; everywhere else every range must accept."""
import numpy as np
import pytest

import verify_cases as vc
from verify_cases import Case

pytestmark = pytest.mark.gpu

PARITY = b"\xff" * 29


def _row_ns_ods(k, seed):
    """random_ods with one namespace per row (increasing downwards): every row and column of
    the ODS stays ordered and a range inside a row's ODS half shares one namespace."""
    from eds_inputs import random_ods
    ods = random_ods(k, seed)
    for r in range(k):
        ods[r, :, :29] = np.frombuffer(bytes(19) + bytes([1 + r // 200, 1 + r % 200]) + bytes(8), np.uint8)
    return ods


def _axis_cases(eds, axis, index, ranges):
    """Cases over EDS row / column `index` with the tree exported by the device."""
    from celestia_eds import proof
    w = eds.Width()
    k = w // 2
    tree = proof.axis_trees(eds, axis, index, 1)[0]
    root = tree[-1].tobytes()
    cells = [eds.GetCell(index, j) if axis == 0 else eds.GetCell(j, index) for j in range(w)]
    out = []
    for s, e in ranges:
        r, c = (index, s) if axis == 0 else (s, index)
        ns = cells[s][:29] if r < k and c < k else PARITY
        out.append(Case(s, e, ns, cells[s:e], proof.nmt_prove_range(tree, s, e), root))
    return out


def _one_namespace(case, k, index):
    """Do the leaves of an axis range share the case's namespace (see the module docstring)?"""
    return index >= k or case.end <= k or case.start >= k


def _check(ctx, cases, must_accept=None, run=None):
    want = vc.mirror(cases)
    got = (run or vc.host_batch)(ctx, cases)
    bad = [i for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, [(i, cases[i].start, cases[i].end, len(cases[i].nodes), want[i]) for i in bad[:8]]
    if must_accept is not None:
        assert all(want[i] for i in range(len(cases)) if must_accept[i])
    return got


def test_every_range_2k8(ctx):
    from celestia_eds import da
    k = 4
    eds = da.ExtendShares(list(_row_ns_ods(k, 3).reshape(-1, 512)))
    ranges = [(s, e) for s in range(2 * k) for e in range(s + 1, 2 * k + 1)]
    for index in (1, 5):  # a Q0 | Q1 row and a parity row
        cases = _axis_cases(eds, 0, index, ranges)
        got = _check(ctx, cases, [_one_namespace(c, k, index) for c in cases])
        assert sum(got) == (len(ranges) if index >= k else 20)


@pytest.mark.parametrize("run", [vc.host_batch, vc.dev_batch], ids=["host", "dev"])
def test_trees_not_a_power_of_two(ctx, run):
    """Only these reach "right child absent" and the chain of trailing nodes."""
    cases, accept = [], []
    for n in (1, 2, 3, 5, 6, 7, 9, 13):
        one = vc.ref_tree(n, 100 + n, namespaces=[bytes(28) + b"\x09"] * n)
        mixed = vc.ref_tree(n, 200 + n)
        for t in (one, mixed):
            for s in range(n):
                for e in range(s + 1, n + 1):
                    cases.append(vc.range_case(t, s, e))
                    accept.append(len(set(t[0][s:e])) == 1)
    got = _check(ctx, cases, accept, run=run)
    # 210 ranges of the one-namespace trees and the 46 single leaves of the others, at least
    assert sum(got) >= sum(accept) >= 256


def _tamper_matrix():
    row0 = vc.ref_tree(8, 41, namespaces=[bytes(28) + b"\x21"] * 8)
    row1 = vc.ref_tree(8, 42, namespaces=[bytes(28) + b"\x22"] * 8)
    bases = [vc.range_case(row0, i, i + 1) for i in range(8)] + [vc.range_case(row0, 2, 7)]
    flips, others = [], []
    for c in bases:
        for byte in (0, 28, 29, 255, 511):
            flips.append(c._replace(leaves=[vc.flip(c.leaves[0], byte)] + list(c.leaves[1:])))
        for i in range(len(c.nodes)):
            for byte in (5, 29 + 5, 58 + 12):  # min namespace, max namespace, digest
                flips.append(c._replace(nodes=c.nodes[:i] + [vc.flip(c.nodes[i], byte)] + c.nodes[i + 1:]))
        nd = list(c.nodes)
        others += [c._replace(nodes=nd[1:]), c._replace(nodes=nd[:-1]), c._replace(nodes=nd + nd[-1:]),
                   c._replace(nodes=nd[1:2] + nd[0:1] + nd[2:]), c._replace(nodes=nd[:-2] + nd[-1:] + nd[-2:-1]),
                   c._replace(start=c.start + 1), c._replace(start=c.start - 1),
                   c._replace(start=c.start + 1, end=c.end + 1), c._replace(start=c.start - 1, end=c.end - 1),
                   c._replace(end=c.end + 1),
                   c._replace(ns=bytes(28) + b"\x20"), c._replace(ns=PARITY), c._replace(root=row1[2].root()),
                   c._replace(start=-1, end=-1 + len(c.leaves)), c._replace(end=c.start),
                   c._replace(start=c.end, end=c.start)]
    return bases, flips, others


def test_tamper_matrix(ctx):
    bases, flips, others = _tamper_matrix()
    cases = bases + flips + others
    got = _check(ctx, cases)
    assert all(got[:len(bases)]), "a base proof rejects"
    assert not any(got[len(bases):len(bases) + len(flips)]), "a flipped bit accepts"


def _mixed_pool():
    trees = [vc.ref_tree(n, 300 + n) for n in (8, 13, 64)]
    rng = np.random.default_rng(17)
    pool = []
    for t in trees:
        n = len(t[1])
        pool += [vc.range_case(t, i, i + 1) for i in range(n)]
        for length in range(1, 17):
            for _ in range(2):
                if length <= n:
                    s = int(rng.integers(0, n - length + 1))
                    pool.append(vc.range_case(t, s, s + length))
    return pool, trees[0][2].root()


@pytest.mark.parametrize("n", [65, 257])
def test_mixed_wave(ctx, n):
    """Single leaves and ranges of length 1..16 from trees of 8, 13 and 64 leaves, valid and
    tampered interleaved, in partial waves whose lanes run different trip counts; a shuffled
    copy of the batch gives the same verdicts, shuffled."""
    pool, other_root = _mixed_pool()
    rng = np.random.default_rng(n)
    cases = []
    for i in range(n):
        c = pool[int(rng.integers(0, len(pool)))]
        cases.append(vc.tampered(c, rng, other_root) if i % 3 == 1 else c)
    got = _check(ctx, cases, run=vc.dev_batch)
    assert 0.2 * n < sum(got) < 0.8 * n
    perm = rng.permutation(n)
    assert vc.dev_batch(ctx, [cases[i] for i in perm], node_shift=1) == [got[i] for i in perm]
    assert vc.host_batch(ctx, cases) == got


def test_k128_depth(ctx):
    from celestia_eds import da
    k = 128
    eds = da.ExtendShares(list(_row_ns_ods(k, 9).reshape(-1, 512)))
    singles = [(i, i + 1) for i in range(2 * k)]
    cases, accept = [], []
    for axis, index in ((0, 0), (0, 200), (1, 77)):
        rng_ = singles + ([(0, k), (0, 2 * k)] if axis == 0 else [])
        cs = _axis_cases(eds, axis, index, rng_)
        cases += cs
        # a column of Q0 | Q2 holds one namespace per row: its single leaves all accept
        accept += [c.end - c.start == 1 or _one_namespace(c, k, index) for c in cs]
    got = _check(ctx, cases, accept)
    assert sum(got) == 3 * 256 + 3  # row 0's [0, 256) crosses from Q0 into parity


def test_verify_share_proofs_block408(ctx, golden):
    from celestia_eds import CelError, da, proof, square
    from square_inputs import block408_txs
    from test_gpu_proof import _ranges
    ods = square.Construct(block408_txs())
    eds = da.ExtendShares(list(ods))
    root = bytes.fromhex(golden["block408"]["data_hash"])
    sps = [proof.NewShareInclusionProofFromEDS(eds, ns, s, e) for ns, s, e in _ranges(ods)]
    assert len(sps) >= 3
    for p in sps:
        p.Validate(root)
    assert proof.VerifyShareProofs(sps, root, ctx=ctx) == [True] * len(sps)
    victim = len(sps) // 2
    sps[victim].Data[-1] = vc.flip(sps[victim].Data[-1], 300)
    with pytest.raises(CelError):
        sps[victim].Validate(root)
    assert proof.VerifyShareProofs(sps, root, ctx=ctx) == [i != victim for i in range(len(sps))]
    assert proof.VerifyShareProofs(sps, bytes(32), ctx=ctx) == [False] * len(sps)


def test_call_errors(ctx):
    from celestia_eds import _lib
    one = [bytes(28) + b"\x05"] * 5
    f = vc.flatten([vc.range_case(vc.ref_tree(5, 1, one), 1, 3), vc.range_case(vc.ref_tree(5, 2, one), 0, 1)])
    ok = np.full(2, 7, np.uint8)
    P = vc._p

    def call(n=2, leaf_off=f["leaf_off"], node_off=f["node_off"], nroots=2, root_idx=f["root_idx"]):
        return ctx.lib.cel_nmt_verify_batch(ctx.handle, n, P(f["starts"]), P(f["ends"]), P(f["ns"]), P(f["leaves"]),
                                            P(leaf_off), P(f["nodes"]), P(node_off), P(f["roots"]), nroots,
                                            P(root_idx), P(ok))

    assert call() == _lib.OK and ok.tolist() == [1, 1]
    assert call(leaf_off=np.array([0, 2, 1], np.uint64)) == _lib.EINVAL
    assert call(node_off=np.array([3, 2, 4], np.uint64)) == _lib.EINVAL
    assert call(nroots=1) == _lib.EINVAL
    assert call(root_idx=np.array([0, 2], np.uint32)) == _lib.EINVAL
    assert ctx.lib.cel_nmt_verify_batch(ctx.handle, 2, None, P(f["ends"]), P(f["ns"]), P(f["leaves"]),
                                        P(f["leaf_off"]), P(f["nodes"]), P(f["node_off"]), P(f["roots"]), 2,
                                        P(f["root_idx"]), P(ok)) == _lib.EINVAL
    assert call(n=0) == _lib.OK
    assert ctx.lib.cel_nmt_verify_batch(ctx.handle, 0, None, None, None, None, None, None, None, None, 0, None,
                                        None) == _lib.OK
    assert ctx.lib.cel_dev_nmt_verify_batch(ctx.handle, 0, None, None, None, None, None, None, None, None, 0, None,
                                            None, None, None) == _lib.OK
