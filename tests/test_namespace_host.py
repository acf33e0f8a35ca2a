"""CPU: the host mirror of the namespace queries (proof.nmt_prove_namespace,
proof.verify_namespace / NMTProof.VerifyNamespace) against brute force on nmt_ref.Tree rows, its
rejections, and what the new C-ABI entry points decide without a device. nmt is a dependency
outside the reference tree, so no vector pins these rules; VerifyInclusion, which the reference's
proof vectors do pin, must accept every inclusion proof the producer gives."""
import ctypes

import numpy as np
import pytest

import namespace_inputs as ni
import nmt_ref

WIDTHS = [2, 4, 8, 16, 32, 64]


def _row(w, seed):
    rng = np.random.default_rng(seed)
    vals = [1 + int(v) for v in rng.integers(0, 3, w // 2).cumsum()]
    return vals, ni.row_tree(vals, seed)


@pytest.mark.parametrize("w", WIDTHS)
def test_producer_and_verifier_against_brute_force(w):
    from celestia_eds import proof
    for seed in range(3):
        vals, (nss, shares, tree) = _row(w, 100 * w + seed)
        table = ni.tree_table(tree.leaves)
        root = tree.root()
        assert table[-1].tobytes() == root
        for v in range(0, max(vals) + 2):
            nid = ni.small_ns(v)
            p = proof.nmt_prove_namespace(table, w, nid)
            empty = proof.NMTProof(Start=0, End=0, Nodes=[])
            assert empty.IsEmptyProof() and not empty.IsOfAbsence()
            if v < min(vals) or v > max(vals):
                assert p is None
                assert empty.VerifyNamespace(nid, [], root)
                continue
            assert not empty.VerifyNamespace(nid, [], root)
            at = [i for i, x in enumerate(vals) if x == v]
            if at:
                assert (p.Start, p.End) == (at[0], at[-1] + 1) and not p.IsOfAbsence()
                assert p.Nodes == tree.prove_range(p.Start, p.End)
                leaves = shares[p.Start:p.End]
                assert p.VerifyNamespace(nid, leaves, root)
                assert p.VerifyInclusion(nid, leaves, root)
            else:
                succ = next(i for i, x in enumerate(vals) if x > v)
                assert (p.Start, p.End) == (succ, succ + 1) and p.IsOfAbsence()
                assert p.LeafHash == tree.leaves[succ] and p.Nodes == tree.prove_range(succ, succ + 1)
                assert p.VerifyNamespace(nid, [], root)
                assert not p.VerifyNamespace(nid, [shares[succ]], root)


def test_parity_row_and_parity_query():
    """A row of parity leaves alone holds no data namespace; a namespace above every data leaf of
    a row is outside its root's range (IgnoreMaxNamespace keeps the parity leaves out of it)."""
    from celestia_eds import proof
    nss, shares, tree = ni.row_tree([], 5, w=8)
    table = ni.tree_table(tree.leaves)
    assert proof.nmt_prove_namespace(table, 8, ni.small_ns(3)) is None
    nss, shares, tree = ni.row_tree([2, 2, 4, 4], 6)
    table = ni.tree_table(tree.leaves)
    assert proof.nmt_prove_namespace(table, 8, ni.small_ns(5)) is None
    assert proof.nmt_prove_namespace(table, 8, ni.small_ns(3)).LeafHash == tree.leaves[2]


def test_named_cases():
    cases = ni.proof_cases() + ni.malformed_cases()
    assert sum(c.want for c in cases) == 6
    for c in cases:
        assert c.mirror() is c.want, c.name


def test_completeness_is_the_rule_that_rejects():
    """The two short ranges are sound inclusion proofs: VerifyInclusion accepts them."""
    from celestia_eds import proof
    short = [c for c in ni.proof_cases() if c.name.startswith("one leaf short")]
    assert len(short) == 2
    for c in short:
        p = proof.NMTProof(Start=c.start, End=c.end, Nodes=c.nodes)
        assert p.VerifyInclusion(c.ns, c.leaves, c.root), c.name
        assert not p.VerifyNamespace(c.ns, c.leaves, c.root), c.name


def test_prefix_is_the_rule_that_rejects():
    from celestia_eds import proof
    c = next(c for c in ni.proof_cases() if c.name == "a share with another prefix")
    p = proof.NMTProof(Start=c.start, End=c.end, Nodes=c.nodes)
    assert p.VerifyInclusion(c.ns, c.leaves, c.root) and not p.VerifyNamespace(c.ns, c.leaves, c.root)


def test_object_form_matches_flat_form():
    from celestia_eds import proof
    for c in ni.proof_cases():
        if c.kind > 1 or (c.kind == 1 and not c.nodes):
            continue
        absent = c.kind == 1
        p = proof.NMTProof(Start=c.start, End=c.end, Nodes=c.nodes[:-1] if absent else c.nodes,
                           LeafHash=c.nodes[-1] if absent else None)
        assert p.VerifyNamespace(c.ns, c.leaves, c.root) is c.want, c.name


# ------------------------------------------------------------------------ ABI, no device
def test_workspace_sizes():
    import celestia_eds._lib as L
    lib = L.load()
    for k in (1, 8, 128, 512):
        sizes = [lib.cel_dev_namespace_workspace_size(k, n) for n in (0, 1, 2, 64, 1024)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        # the pair table and the entry table for n * 2k pairs, at the least
        assert sizes[-1] >= 1024 * 2 * k * (16 + 40)
    for k in (0, 3, 1024):
        assert lib.cel_dev_namespace_workspace_size(k, 4) == 0
    assert lib.cel_dev_namespace_workspace_size(512, 1 << 22) == 0  # n * 2k = 2^32
    sizes = [lib.cel_dev_nmt_verify_namespace_workspace_size(10 * n, 8 * n, n) for n in (0, 1, 2, 100, 5000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # one more leaf record per proof than the inclusion verifier
    assert sizes[3] >= lib.cel_dev_nmt_verify_workspace_size(1000, 800, 100) + 100 * 96


def test_entry_points_reject_without_a_context():
    import celestia_eds._lib as L
    lib = L.load()
    cnt = ctypes.c_uint64(77)
    ns = (ctypes.c_uint8 * 29)(*([0xFF] * 29))
    assert lib.cel_dev_namespace_plan(None, None, 8, 1, ns, 0, *([None] * 7), ctypes.byref(cnt), None, None) == L.EINVAL
    assert lib.cel_dev_namespace_prove(None, None, None, 8, 1, None, None, None, None) == L.EINVAL
    assert lib.cel_namespace_rows(None, None, 8, 1, ns, 0, 0, 0, *([None] * 9), ctypes.byref(cnt), None, None) == L.EINVAL
    assert lib.cel_nmt_verify_namespace_batch(None, 1, *([None] * 9), 1, None, None) == L.EINVAL
    assert lib.cel_dev_nmt_verify_namespace_batch(None, 1, *([None] * 9), 1, None, None, None, None) == L.EINVAL
    assert cnt.value == 77
    assert (L.NS_INCLUSION, L.NS_ABSENCE) == (0, 1)
