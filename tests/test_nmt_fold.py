"""CPU: the bottom-up fold that csrc/nmt_verify.hip runs (tests/nmt_ref.fold_verify) gives the
verdict of the recursive mirror (celestia_eds.proof.NMTProof.VerifyInclusion, pinned to the
reference's vectors by tests/test_proof.py) on every range of every tree of 1..17 leaves and
on each of those proofs with one node dropped, one appended, the nodes reversed, the range
shifted left or right and the leaves reversed. The new entry points reject a nil context
before any device call."""
import ctypes

import numpy as np
import pytest

import nmt_ref


def _trees():
    """Per leaf count two trees: one namespace throughout (every range accepts), and
    several namespaces ending in parity leaves (ranges inside one namespace accept)."""
    rng = np.random.default_rng(5)
    out = []
    for n in range(1, 18):
        shares = [rng.integers(0, 256, 8, dtype=np.uint8).tobytes() for _ in range(n)]
        one = [bytes(28) + b"\x07"] * n
        mixed = nmt_ref.sorted_namespaces(n, rng, parity_from=n - n // 3)
        for nss in (one, mixed):
            out.append((nss, shares, nmt_ref.Tree.from_shares(nss, shares)))
    return out


def _variants(start, end, shares, nodes):
    yield "base", start, end, shares, nodes
    for i in range(len(nodes)):
        yield f"drop{i}", start, end, shares, nodes[:i] + nodes[i + 1:]
    yield "append", start, end, shares, nodes + [nodes[-1] if nodes else bytes(90)]
    yield "reversed", start, end, shares, nodes[::-1]
    yield "left", start - 1, end - 1, shares, nodes
    yield "right", start + 1, end + 1, shares, nodes
    yield "leaves", start, end, shares[::-1], nodes


def test_fold_equals_recursive_mirror():
    cases = accepted = 0
    for nss, shares, tree in _trees():
        n, root = len(shares), tree.root()
        uniform = len(set(nss)) == 1
        for start in range(n):
            for end in range(start + 1, n + 1):
                nodes = tree.prove_range(start, end)
                for name, s, e, sh, nd in _variants(start, end, shares[start:end], nodes):
                    want = nmt_ref.mirror_verify(s, e, nss[start], sh, nd, root)
                    got = nmt_ref.fold_verify(s, e, nss[start], sh, nd, root)
                    assert got == want, (n, start, end, name, want)
                    cases += 1
                    accepted += want
                    if name == "base" and (uniform or len(set(nss[start:end])) == 1):
                        assert want, (n, start, end)
    assert cases > 8000 and accepted > 1000, (cases, accepted)


def test_fold_rejects_malformed_ranges():
    nss, shares, tree = _trees()[14]  # 8 leaves, one namespace
    root, ns = tree.root(), nss[0]
    nodes = tree.prove_range(2, 3)
    assert nmt_ref.fold_verify(2, 3, ns, shares[2:3], nodes, root)
    for s, e, sh in ((-1, 0, shares[:1]), (2, 2, []), (3, 2, shares[:1]), (2, 3, shares[2:4]), (2, 4, shares[2:3])):
        assert not nmt_ref.fold_verify(s, e, ns, sh, nodes, root)
        assert not nmt_ref.mirror_verify(s, e, ns, sh, nodes, root)
    # a namespace that differs from the share's own prefix hashes with the given one
    other = bytes(28) + b"\x08"
    assert not nmt_ref.fold_verify(2, 3, other, shares[2:3], nodes, root)


def test_verify_entry_points_validate_without_a_device():
    """Nil context: CEL_EINVAL before any device call (no GPU here); the workspace size is
    host arithmetic."""
    import celestia_eds._lib as L
    lib = L.load()
    one = (ctypes.c_uint8 * 512)()
    assert lib.cel_nmt_verify_batch(None, 1, None, None, None, None, None, None, None, None, 1, None, None) == L.EINVAL
    assert lib.cel_nmt_verify_batch(None, 0, None, None, None, None, None, None, None, None, 0, None, None) == L.EINVAL
    assert lib.cel_dev_nmt_verify_batch(None, 1, None, None, None, None, None, None, None, None, 1, None, None,
                                        None, None) == L.EINVAL
    assert lib.cel_dev_place_samples(None, None, None, 8, None, None, 1, None, None, None, one, None, None,
                                     None) == L.EINVAL
    assert lib.cel_repair_samples(None, 8, None, None, 1, None, None, None, one, None, None, None, None, None,
                                  None, None, None, None) == L.EINVAL
    small = lib.cel_dev_nmt_verify_workspace_size(1, 8, 1)
    big = lib.cel_dev_nmt_verify_workspace_size(36000, 8 * 36000, 36000)
    # 96-byte records of every leaf and node and one root per proof, plus the proof table
    assert small >= 96 * (1 + 8 + 1) and big >= 96 * (36000 * 10) and big < 2 * 96 * (36000 * 10)


def test_verify_workspace_layouts():
    """The two workspace sizes are part of the ABI (a caller allocates by them): the proof
    table, a 32-byte namespace and a dword per leaf, 96-byte records of the leaves and of the
    nodes with one root per proof, each part rounded up to 256 bytes. The namespace verifier
    keeps one more leaf record per proof and one byte per leaf (at least one)."""
    import celestia_eds._lib as L
    lib = L.load()
    a = lambda x: (x + 255) // 256 * 256

    def inclusion(tl, tn, n):
        return a(40 * n) + a(32 * n) + a(4 * tl) + a(96 * tl) + a(96 * (tn + n))

    for n in (0, 1, 2, 100):
        for tl in (0, 1, 63, 1000):
            for tn in (0, 8, 800):
                assert lib.cel_dev_nmt_verify_workspace_size(tl, tn, n) == inclusion(tl, tn, n), (n, tl, tn)
                assert lib.cel_dev_nmt_verify_namespace_workspace_size(tl, tn, n) == \
                    inclusion(tl + n, tn, n) + a(max(tl, 1)), (n, tl, tn)


@pytest.mark.parametrize("n", [3, 13])
def test_prove_range_matches_device_tree_order(n):
    """nmt_ref.Tree.prove_range lists nodes as nmt does: left siblings largest first (one per
    set bit of start), then right siblings smallest first."""
    rng = np.random.default_rng(n)
    shares = [rng.integers(0, 256, 8, dtype=np.uint8).tobytes() for _ in range(n)]
    tree = nmt_ref.Tree.from_shares([bytes(29)] * n, shares)
    for start in range(n):
        nodes = tree.prove_range(start, start + 1)
        assert len(nodes) >= bin(start).count("1")
        assert nmt_ref.fold_verify(start, start + 1, bytes(29), shares[start:start + 1], nodes, tree.root())
