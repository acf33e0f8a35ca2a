"""Inputs of the namespace query tests: squares whose shares carry sorted version-0 namespaces in
runs of given lengths, the host mirror's answer for a batch of queries in the flat layout the
device gives, and row trees in proof.axis_trees' layout built with hashlib alone."""
import numpy as np

NS = 29
SHARE = 512
PARITY = b"\xff" * NS


def ns_value(v):
    """The version-0 namespace 0x00 || 0x00*18 || v (10 bytes, big endian)."""
    return bytes(19) + int(v).to_bytes(10, "big")


def run_ods(k, runs, seed):
    """(ods, present, absent): a k x k ODS whose shares, row-major, carry namespace 2 * (i + 1)
    for the run i of length runs[i] (sum k * k), random bodies. present[i] is run i's namespace;
    absent[i] = 2 * (i + 1) + 1 lies between run i and run i + 1 and is in no share."""
    assert sum(runs) == k * k and all(r > 0 for r in runs)
    ods = np.random.default_rng(seed).integers(0, 256, (k, k, SHARE), dtype=np.uint8)
    flat = ods.reshape(-1, SHARE)
    at = 0
    for i, r in enumerate(runs):
        flat[at:at + r, :NS] = np.frombuffer(ns_value(2 * (i + 1)), np.uint8)
        at += r
    return ods, [ns_value(2 * (i + 1)) for i in range(len(runs))], [ns_value(2 * (i + 1) + 1) for i in range(len(runs))]


BELOW_ALL = ns_value(1)
ABOVE_ALL = bytes([0]) + bytes(18) + b"\xff" * 10  # the largest version-0 namespace


def seeded_runs(k, seed, longest):
    """Run lengths 1 .. longest drawn until they fill the k * k shares."""
    rng = np.random.default_rng(seed)
    out, left = [], k * k
    while left:
        r = min(int(rng.integers(1, longest + 1)), left)
        out.append(r)
        left -= r
    return out


def tree_table(records):
    """Every node of the NMT over `records` (a power of two of 90-byte leaf records) in
    proof.axis_trees' layout: [2n - 1][90], level-major from the leaves, the root last."""
    from celestia_eds.proof import _nmt_node
    level, out = [bytes(r) for r in records], []
    while True:
        out += level
        if len(level) == 1:
            break
        level = [_nmt_node(level[i], level[i + 1]) for i in range(0, len(level), 2)]
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 90)


def mirror_flat(row_trees, cells, namespaces):
    """The host mirror's answer to cel_dev_namespace_plan + cel_dev_namespace_prove:
    proof.nmt_prove_namespace on every row tree (row_trees: proof.axis_trees of all 2k rows) for
    every namespace, in (namespace index, row) order, flattened as the device flattens it."""
    from celestia_eds import proof
    w = cells.shape[0]
    ns_idx, rows, starts, ends, kinds, leaf_off, node_off, leaves, nodes = [], [], [], [], [], [0], [0], [], []
    roots = [row_trees[r][-1].tobytes() for r in range(w)]
    for i, ns in enumerate(namespaces):
        ns = bytes(ns)
        for r in range(w):
            if not roots[r][:NS] <= ns <= roots[r][NS:2 * NS]:
                continue  # nmt_prove_namespace says None as well; this only saves its scan
            p = proof.nmt_prove_namespace(row_trees[r], w, ns)
            if p is None:
                continue
            absent = p.IsOfAbsence()
            ns_idx.append(i)
            rows.append(r)
            starts.append(p.Start)
            ends.append(p.End)
            kinds.append(1 if absent else 0)
            nodes += list(p.Nodes) + ([p.LeafHash] if absent else [])
            if not absent:
                leaves += [cells[r, c].tobytes() for c in range(p.Start, p.End)]
            leaf_off.append(len(leaves))
            node_off.append(len(nodes))
    return dict(ns_idx=np.array(ns_idx, np.uint32), rows=np.array(rows, np.uint32), starts=np.array(starts, np.int32),
                ends=np.array(ends, np.int32), kinds=np.array(kinds, np.uint8), leaf_off=np.array(leaf_off, np.uint64),
                node_off=np.array(node_off, np.uint64),
                leaves=np.frombuffer(b"".join(leaves), np.uint8).reshape(-1, SHARE),
                nodes=np.frombuffer(b"".join(nodes), np.uint8).reshape(-1, 90))


# --------------------------------------------------- namespaces that differ at every byte
LADDER_VALUES = (0x01, 0x02, 0x7E, 0x7F, 0x80, 0x81, 0xFC, 0xFD)  # both sides of 0x80
SHORT_RUNS = (1, 1, 1, 2, 2, 3)
SIGN_BYTES = frozenset(range(0, NS, 4)) | {NS - 1}  # the top byte of each compare word
ABOVE_LADDER = b"\xfd" + b"\xff" * (NS - 1)         # above every ladder value, below N_0


def near_parity(b):
    """N_b: the parity namespace with byte b lowered to 0xFE. N_28 is the tail-padding namespace."""
    return b"\xff" * b + b"\xfe" + b"\xff" * (NS - 1 - b)


def byte_ladder(k, seed, longest=3, row_ends=None, tail=None):
    """(namespaces, transitions): the k * k namespaces of an ODS, row-major and sorted, in runs of
    1 .. longest, none the parity namespace; and for every two consecutive distinct namespaces
    x < y the tuple (pos, b, x, y): pos the flat index of the first share of y, b the first byte
    at which x and y differ.

    The ladder starts at 0x7F * 29. A transition at byte b bumps x[b] (by 2 at the last byte, so
    that a namespace lies between x and y) and redraws every later byte from LADDER_VALUES; that
    always ascends. What chance would leave open is chosen:
      * b goes round all 29 bytes (stride 7) among the transitions inside a row, and in ascending
        order among the transitions that fall on a row end, each until every byte has had its turn;
      * y[b + 1] is drawn below x[b + 1], a later byte that points the other way;
      * a byte of SIGN_BYTES is redrawn as 0x7F until a bump has taken it across to 0x80.
    row_ends (default: k >= 32 and runs of at most 3) ends every run at its row's end, so each
    row end is a transition. tail (default: k == 32) fills the last two rows with N_0 .. N_28,
    ascending, in runs of 3 (the first six) and 2."""
    rng = np.random.default_rng(seed)
    short = longest <= 3
    row_ends = (short and k >= 32) if row_ends is None else row_ends
    tail = (k == 32) if tail is None else tail
    n = k * k - (2 * k if tail else 0)
    order = [(7 * i) % NS for i in range(NS)]
    cur = bytearray([0x7F] * NS)
    need_sign, done, done_row = set(SIGN_BYTES), set(), set()
    out, trans = [], []
    while True:
        r = int(rng.choice(SHORT_RUNS)) if short else int(rng.integers(1, longest + 1))
        r = min(r, n - len(out))
        if row_ends:
            r = min(r, k - len(out) % k)
        out += [bytes(cur)] * r
        pos = len(out)
        if pos == n:
            break
        at_end = pos % k == 0
        had = done_row if at_end else done
        if len(had) == NS:
            had.clear()
        b = next(b for b in (range(NS) if at_end else order) if b not in had)
        step = 2 if b == NS - 1 else 1
        while cur[b] + step > 0xFF:  # cannot be bumped: the byte before it
            b -= 1
            step = 1
        assert b >= 0
        x = bytes(cur)
        if cur[b] == 0x7F:
            need_sign.discard(b)
        cur[b] += step
        for j in range(b + 1, NS):
            cur[j] = 0x7F if j in need_sign else int(rng.choice(LADDER_VALUES))
        contrary = b == NS - 1
        if b + 1 < NS and x[b + 1] > 0:
            lower = [v for v in LADDER_VALUES if v < x[b + 1]] or [0]
            cur[b + 1] = 0x7F if b + 1 in need_sign and 0x7F in lower else int(rng.choice(lower))
            contrary = True
        if contrary:
            had.add(b)
        trans.append((pos, b, x, bytes(cur)))
    assert out[-1] < ABOVE_LADDER
    if tail:
        for b in range(NS):
            trans.append((len(out), 0 if b == 0 else b - 1, out[-1], near_parity(b)))
            out += [near_parity(b)] * (3 if b < 6 else 2)
    assert len(out) == k * k and PARITY not in out
    return out, trans


def absentees(x, y, b):
    """The namespaces strictly between the neighbours x < y (first differing at byte b) that sit
    at the tails' extremes: x[:b + 1] || 0xFF.. just above x's prefix and y[:b + 1] || 0x00.. just
    below y's. Each differs from one neighbour in late bytes only and from the other at byte b
    with every later byte pointing the wrong way. One that equals x or y is dropped, both if
    either is the parity namespace. At the last byte there is no tail: the value between."""
    if b == NS - 1:
        return [x[:b] + bytes([x[b] + 1])] if x[b] + 1 < y[b] else []
    hi, lo = x[:b + 1] + b"\xff" * (NS - 1 - b), y[:b + 1] + bytes(NS - 1 - b)
    if PARITY in (hi, lo):
        return []
    out = [q for q in (hi, lo) if q not in (x, y)]
    assert all(x < q < y for q in out)
    return out


def ladder_queries(namespaces, trans):
    """(queries, notes) for a ladder: every present namespace, the absentees of every transition,
    one namespace below the ladder and ABOVE_LADDER. notes[i] = (what, bytes, pos): "present" with
    the bytes at which the namespace is decided against its two neighbours, "absent" with the
    transition's byte and pos, "outside"."""
    sides = {}
    for pos, b, x, y in trans:
        sides.setdefault(x, set()).add(b)
        sides.setdefault(y, set()).add(b)
    queries, notes = [], []
    for p in sorted(set(namespaces)):
        queries.append(p)
        notes.append(("present", sides.get(p, set()), None))
    for pos, b, x, y in trans:
        for q in absentees(x, y, b):
            queries.append(q)
            notes.append(("absent", {b}, pos))
    queries += [BELOW_ALL, ABOVE_LADDER]
    notes += [("outside", set(), None)] * 2
    assert len(set(queries)) == len(queries) and BELOW_ALL < namespaces[0]
    return queries, notes


def ladder_square(k, seed, **kw):
    """(cells, namespaces, transitions): a 2k x 2k square whose Q0 carries byte_ladder(k, seed)
    in its shares' first 29 bytes; every other byte of the square is random (no codeword)."""
    nss, trans = byte_ladder(k, seed, **kw)
    cells = np.random.default_rng([seed, k]).integers(0, 256, (2 * k, 2 * k, SHARE), dtype=np.uint8)
    cells[:k, :k, :NS] = np.frombuffer(b"".join(nss), np.uint8).reshape(k, k, NS)
    return cells, nss, trans


def square_row_tree(cells, r):
    """nmt_ref.Tree of row r of any square by the wrapper's rule: a leaf's namespace is its
    share's first 29 bytes inside Q0 and the parity namespace elsewhere. hashlib alone."""
    import nmt_ref
    w = cells.shape[0]
    nss = [cells[r, c, :NS].tobytes() if r < w // 2 and c < w // 2 else PARITY for c in range(w)]
    return nmt_ref.Tree.from_shares(nss, [cells[r, c].tobytes() for c in range(w)])


def square_row_tables(cells):
    """tree_table of every row of the square, as mirror_flat takes them."""
    return [tree_table(square_row_tree(cells, r).leaves) for r in range(cells.shape[0])]


def pair_rule(row, q, w):
    """What row (its k sorted ODS namespaces; the other w - k leaves are parity) yields for the
    namespace q, by counting with bytes comparisons: None, or (start, end, kind)."""
    if not row[0] <= q <= row[-1]:
        return None  # the root's range, parity ignored
    lt, le = sum(x < q for x in row), sum(x <= q for x in row)
    return (lt, le, 0) if le > lt else (lt, lt + 1, 1)


# ----------------------------------------------------------------- single rows, proof cases
def small_ns(v):
    return bytes(27) + bytes([v >> 8 & 0xFF, v & 0xFF])


def row_tree(values, seed, w=None):
    """(namespaces, shares, nmt_ref.Tree) of a row of w = 2 * len(values) leaves (or w given): the
    left leaves carry small_ns(values[i]) in their shares' first 29 bytes, the rest are parity."""
    import nmt_ref
    w = w or 2 * len(values)
    rng = np.random.default_rng(seed)
    nss = [small_ns(v) for v in values] + [PARITY] * (w - len(values))
    shares = []
    for i in range(w):
        body = rng.integers(0, 256, SHARE, dtype=np.uint8).tobytes()
        shares.append(nss[i] + body[NS:] if i < len(values) else body)
    return nss, shares, nmt_ref.Tree.from_shares(nss, shares)


class NsCase:
    """One proof as the verifier takes it: an absence proof's leaf hash is the last node."""

    def __init__(self, name, start, end, kind, ns, leaves, nodes, root, want):
        self.name, self.start, self.end, self.kind, self.ns = name, start, end, kind, bytes(ns)
        self.leaves, self.nodes, self.root, self.want = list(leaves), list(nodes), bytes(root), want

    def mirror(self):
        from celestia_eds import proof
        return proof.verify_namespace(self.start, self.end, self.kind, self.ns, self.leaves, self.nodes, self.root)


def flip(b, byte, bit=0x10):
    x = bytearray(b)
    x[byte] ^= bit
    return bytes(x)


def proof_cases():
    """Accepted proofs and every rejection of the namespace verifier, each by a named
    construction, with the verdict it must get. Row of 16 leaves: namespaces 1 2 2 2 3 3 5 6 and
    eight parity leaves, so namespace 2 is [1, 4), 3 is [4, 6) and 4 is absent before leaf 6."""
    nss, shares, tree = row_tree([1, 2, 2, 2, 3, 3, 5, 6], 11)
    root = tree.root()
    rec = tree.leaves
    pr = tree.prove_range
    two, three, four = small_ns(2), small_ns(3), small_ns(4)
    out = []
    add = lambda *a: out.append(NsCase(*a))
    add("inclusion", 1, 4, 0, two, shares[1:4], pr(1, 4), root, True)
    add("inclusion from an even leaf", 4, 6, 0, three, shares[4:6], pr(4, 6), root, True)
    add("inclusion of one leaf", 0, 1, 0, small_ns(1), shares[0:1], pr(0, 1), root, True)
    add("absence", 6, 7, 1, four, [], pr(6, 7) + [rec[6]], root, True)
    add("empty proof below the root's range", 0, 0, 0, small_ns(0), [], [], root, True)
    add("empty proof above the root's range", 0, 0, 0, small_ns(7), [], [], root, True)
    # completeness: the last leaf of namespace 2 left out; it is itself the first right node
    assert pr(1, 3)[1] == rec[3]
    add("one leaf short at the right end", 1, 3, 0, two, shares[1:3], pr(1, 3), root, False)
    # the first leaf of namespace 3 left out; it is itself the last left node
    assert pr(5, 6)[1] == rec[4]
    add("one leaf short at the left end", 5, 6, 0, three, shares[5:6], pr(5, 6), root, False)
    # a tree hashed under namespace 2 over a share that begins with another namespace
    odd = list(shares)
    odd[2] = small_ns(9) + shares[2][NS:]
    import nmt_ref
    t2 = nmt_ref.Tree.from_shares(nss, odd)
    add("a share with another prefix", 1, 4, 0, two, odd[1:4], t2.prove_range(1, 4), t2.root(), False)
    # the absence proof of 4 offered for 5, the namespace of the leaf hash itself
    add("absence with leaf hash min == nid", 6, 7, 1, small_ns(5), [], pr(6, 7) + [rec[6]], root, False)
    # ... and for 6, above it (the leaf hash min < nid)
    add("absence with leaf hash min < nid", 6, 7, 1, small_ns(6), [], pr(6, 7) + [rec[6]], root, False)
    add("absence with a leaf", 6, 7, 1, four, shares[6:7], pr(6, 7) + [rec[6]], root, False)
    add("absence without its leaf hash", 6, 7, 1, four, [], pr(6, 7), root, False)
    add("absence over two leaves", 6, 8, 1, four, [], pr(6, 8) + [rec[6]], root, False)
    add("kind 2", 1, 4, 2, two, shares[1:4], pr(1, 4), root, False)
    add("a node bit flipped", 1, 4, 0, two, shares[1:4], [flip(pr(1, 4)[0], 70)] + pr(1, 4)[1:], root, False)
    add("the leaf hash bit flipped", 6, 7, 1, four, [], pr(6, 7) + [flip(rec[6], 80)], root, False)
    add("the root bit flipped", 1, 4, 0, two, shares[1:4], pr(1, 4), flip(root, 60), False)
    add("empty proof inside the root's range", 0, 0, 0, four, [], [], root, False)
    add("empty proof of kind absence", 0, 0, 1, small_ns(0), [], [], root, False)
    add("start == end with a node", 3, 3, 0, small_ns(0), [], [rec[0]], root, False)
    return out


def malformed_cases():
    """Proofs whose structure is wrong: verdict 0, never an error of the call."""
    nss, shares, tree = row_tree([1, 2, 2, 2, 3, 3, 5, 6], 11)
    root, pr = tree.root(), tree.prove_range
    two = small_ns(2)
    return [NsCase("start < 0", -1, 2, 0, two, shares[1:4], pr(1, 4), root, False),
            NsCase("end < start", 4, 1, 0, two, shares[1:4], pr(1, 4), root, False),
            NsCase("a leaf too many", 1, 4, 0, two, shares[1:5], pr(1, 4), root, False),
            NsCase("a leaf too few", 1, 4, 0, two, shares[1:3], pr(1, 4), root, False),
            NsCase("too few nodes", 3, 4, 0, two, shares[3:4], pr(3, 4)[:1], root, False),
            NsCase("absence with too few nodes", 7, 8, 1, small_ns(4), [], pr(7, 8)[:3], root, False)]
