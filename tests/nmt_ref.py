"""Host reference for the NMT proof verifier's tests (hashlib only, no device):

  * Tree: an NMT over any number of leaves, split at the largest power of two below n as
    nmt does, with prove_range(start, end) giving the proof nodes in nmt order;
  * fold_verify: nmt Proof.VerifyInclusion run bottom-up, the way csrc/nmt_verify.hip runs
    it: the run of nodes covering [start, end) is folded level by level in place, with one
    hash per step, so no stack is needed. tests/test_nmt_fold.py checks it against the
    recursive mirror (celestia_eds.proof.NMTProof.VerifyInclusion).
"""
from celestia_eds.proof import NMTProof, PARITY_NS, _nmt_leaf, _nmt_node, _split_point

NS = 29


def leaf_record(ns, share):
    return _nmt_leaf(ns, share)


class Tree:
    """NMT over leaf records (90 bytes each, namespaces non-decreasing)."""

    def __init__(self, records):
        self.leaves = list(records)
        self._memo = {}

    @classmethod
    def from_shares(cls, namespaces, shares):
        return cls([_nmt_leaf(ns, sh) for ns, sh in zip(namespaces, shares)])

    def _root(self, s, e):
        if e - s == 1:
            return self.leaves[s]
        if (s, e) not in self._memo:
            k = _split_point(e - s)
            self._memo[s, e] = _nmt_node(self._root(s, s + k), self._root(s + k, e))
        return self._memo[s, e]

    def root(self):
        return self._root(0, len(self.leaves))

    def prove_range(self, start, end):
        """The proof nodes of leaves [start, end): the roots of the maximal subtrees outside
        the range, left to right (nmt ProveRange)."""
        out = []

        def walk(s, e):
            if e <= start or s >= end:
                out.append(self._root(s, e))
                return
            if e - s == 1:
                return
            k = _split_point(e - s)
            walk(s, s + k)
            walk(s + k, e)

        walk(0, len(self.leaves))
        return out


def fold_verify(start, end, namespace, shares, nodes, root):
    """Bottom-up VerifyInclusion. Malformed proofs are False, never an exception."""
    if start < 0 or end <= start or len(shares) != end - start:
        return False
    if any(len(n) != 90 for n in nodes) or len(root) != 90:
        return False
    nl = bin(start).count("1")
    if len(nodes) < nl:
        return False
    levels = 0
    while (1 << levels) < end:
        levels += 1
    rec = [_nmt_leaf(namespace, s) for s in shares]  # the proof's own records, folded in place
    cnt, lo, li, ri = len(rec), start, nl, nl

    def hash_into(j, a, b):
        rec[j] = _nmt_node(a, b)

    try:
        for _ in range(levels):
            pre = lo & 1
            if pre:
                li -= 1
            m = cnt + pre
            app = (m & 1) == 1 and ri < len(nodes)
            if app:
                right = nodes[ri]
                ri += 1
                m += 1
            for j in range(m // 2):
                ea, eb = 2 * j, 2 * j + 1
                a = nodes[li] if pre and ea == 0 else rec[ea - pre]
                b = right if app and eb == m - 1 else rec[eb - pre]
                hash_into(j, a, b)
            if m & 1:  # no right sibling left: the last node moves up unchanged
                rec[m // 2] = rec[m - 1 - pre]
            cnt = m // 2 + (m & 1)
            lo >>= 1
        while ri < len(nodes):
            hash_into(0, rec[0], nodes[ri])
            ri += 1
    except ValueError:  # unordered children
        return False
    return rec[0] == root


def mirror_verify(start, end, namespace, shares, nodes, root):
    """The recursive mirror's verdict; an exception inside it counts as reject."""
    try:
        return bool(NMTProof(Start=start, End=end, Nodes=list(nodes)).VerifyInclusion(namespace, list(shares), root))
    except Exception:
        return False


def sorted_namespaces(n, rng, parity_from=None):
    """n non-decreasing 29-byte namespaces in runs of equal ones; from index parity_from on, 0xFF*29."""
    vals = [1 + int(v) for v in rng.integers(0, 3, n).cumsum()]
    out = [bytes(27) + bytes([v >> 8 & 0xFF, v & 0xFF]) for v in vals]
    if parity_from is not None:
        out[parity_from:] = [PARITY_NS] * (n - parity_from)
    return out
