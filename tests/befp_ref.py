"""Host reference for the bad-encoding fraud proof tests: the verdict rule of
include/celestia_eds.h restated with pieces the tests already trust, and the squares the
cases are cut from. No device.

  * entries verify through nmt_ref.mirror_verify (the recursive VerifyInclusion mirror);
  * the rebuild is oracle.rs_decode, oracle.rs_encode of the data half, and
    oracle.axis_root(..., check_order=False);
  * squares that are not codewords get their roots from oracle.roots(eds, check_order=False).

An entry is (position, share, nodes, entry_axis); a proof is (axis, index, entries).
"""
import numpy as np

import oracle
from celestia_eds.proof import PARITY_NS
from nmt_ref import Tree, mirror_verify

NOT_FRAUD, FRAUD, BAD_SHARE, TOO_FEW, MALFORMED = range(5)
SHARE, NODE = 512, 90


def structural(k, axis, index, entries):
    """Steps 1 and 2: MALFORMED, TOO_FEW or None."""
    w = 2 * k
    if axis > 1 or index >= w:
        return MALFORMED
    seen = set()
    for pos, _, _, ea in entries:
        if pos >= w or ea > 1 or pos in seen:
            return MALFORMED
        seen.add(pos)
    return TOO_FEW if len(entries) < k else None


def entry_ok(k, axis, index, entry, row_roots, col_roots):
    """Step 3 for one entry: its single-leaf proof in the cell's row tree (entry_axis 0) or
    column tree (1), the namespace by the wrapper's rule."""
    pos, share, nodes, ea = entry
    row, col = (pos, index) if axis else (index, pos)
    root = bytes(col_roots[col]) if ea else bytes(row_roots[row])
    leaf = row if ea else col
    if len(share) != SHARE:
        return False
    ns = bytes(share[:29]) if row < k and col < k else PARITY_NS
    return mirror_verify(leaf, leaf + 1, ns, [bytes(share)], [bytes(x) for x in nodes], root)


def rebuild_root(k, index, entries):
    """Step 4: the root of the axis rebuilt from the entries."""
    w = 2 * k
    shards = np.zeros((w, SHARE), np.uint8)
    present = np.zeros(w, np.uint8)
    for pos, share, _, _ in entries:
        shards[pos] = np.frombuffer(bytes(share), np.uint8)
        present[pos] = 1
    full = shards if present.all() else oracle.rs_decode(shards, present)
    full = np.concatenate([full[:k], oracle.rs_encode(full[:k])])
    rc, root = oracle.axis_root(full, k, index, check_order=False)
    assert rc == 0
    return root


def verdict(k, axis, index, entries, row_roots, col_roots):
    """(verdict, rebuilt root or None) of one proof."""
    v = structural(k, axis, index, entries)
    if v is not None:
        return v, None
    if not all(entry_ok(k, axis, index, e, row_roots, col_roots) for e in entries):
        return BAD_SHARE, None
    root = rebuild_root(k, index, entries)
    accused = bytes(col_roots[index]) if axis else bytes(row_roots[index])
    return (FRAUD if root != accused else NOT_FRAUD), root


# ------------------------------------------------------------------- squares


def roots_of(eds):
    """Every root of a square that need not be a codeword (no push-order check)."""
    rc, rr, cr = oracle.roots(eds, check_order=False)
    assert rc == 0
    return [r.tobytes() for r in rr], [c.tobytes() for c in cr]


def honest_square(k, seed=31):
    from eds_inputs import random_ods
    eds = oracle.extend(random_ods(k, seed))
    return (eds,) + roots_of(eds)


def malicious_square(k, cell, seed=31, byte=100):
    """Extend, flip one byte of `cell` (past the namespace), then every root over the result."""
    eds = honest_square(k, seed)[0].copy()
    eds[cell[0], cell[1], byte] ^= 0x5A
    return (eds,) + roots_of(eds)


def axis_tree(eds, k, axis, index):
    """The wrapper tree of one axis of `eds` (hashlib, for small squares)."""
    w = 2 * k
    cells = [eds[j, index].tobytes() if axis else eds[index, j].tobytes() for j in range(w)]
    nss = [c[:29] if index < k and j < k else PARITY_NS for j, c in enumerate(cells)]
    return Tree.from_shares(nss, cells)


def host_entry(eds, k, axis, index, pos, entry_axis):
    """Entry `pos` of accused (axis, index) proved in direction entry_axis, by hashlib."""
    row, col = (pos, index) if axis else (index, pos)
    tree = axis_tree(eds, k, entry_axis, col if entry_axis else row)
    leaf = row if entry_axis else col
    return (pos, eds[row, col].tobytes(), tree.prove_range(leaf, leaf + 1), entry_axis)
