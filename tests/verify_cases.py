"""Shared plumbing of the GPU tests of the batched NMT verifier: a proof case is
(start, end, namespace, leaves, nodes, root); run them through the host entry
(proof.VerifyInclusionBatch) or the device-resident one (cel_dev_nmt_verify_batch), and
through the host mirror."""
import ctypes
from collections import namedtuple

import numpy as np

import nmt_ref

Case = namedtuple("Case", "start end ns leaves nodes root")


def mirror(cases):
    return [nmt_ref.mirror_verify(c.start, c.end, c.ns, c.leaves, c.nodes, c.root) for c in cases]


def host_batch(ctx, cases):
    from celestia_eds import proof
    return proof.VerifyInclusionBatch([proof.NMTProof(Start=c.start, End=c.end, Nodes=list(c.nodes)) for c in cases],
                                      [c.ns for c in cases], [list(c.leaves) for c in cases],
                                      [c.root for c in cases], ctx=ctx)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def flatten(cases):
    """The flat arrays of cel_nmt_verify_batch for `cases`, every root its own entry."""
    buf = lambda parts: np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy()
    return dict(
        n=len(cases),
        starts=np.array([c.start for c in cases], np.int32), ends=np.array([c.end for c in cases], np.int32),
        ns=buf(c.ns for c in cases), leaves=buf(x for c in cases for x in c.leaves),
        leaf_off=np.cumsum([0] + [len(c.leaves) for c in cases]).astype(np.uint64),
        nodes=buf(x for c in cases for x in c.nodes),
        node_off=np.cumsum([0] + [len(c.nodes) for c in cases]).astype(np.uint64),
        roots=buf(c.root for c in cases), root_idx=np.arange(len(cases), dtype=np.uint32))


def dev_batch(ctx, cases, node_shift=2):
    """cel_dev_nmt_verify_batch over device buffers; the packed nodes start node_shift bytes
    into their buffer and the roots 90 bytes into theirs, so neither is dword aligned
    throughout."""
    from celestia_eds import _lib
    from hipmem import DeviceBuffer, synchronize
    f = flatten(cases)
    d_leaves = DeviceBuffer(f["leaves"].nbytes)
    d_leaves.upload(f["leaves"])
    d_nodes = DeviceBuffer(f["nodes"].nbytes + node_shift)
    d_nodes.upload_at(node_shift, f["nodes"])
    d_roots = DeviceBuffer(f["roots"].nbytes + 90)
    d_roots.upload_at(90, f["roots"])
    d_ok = DeviceBuffer(f["n"], fill=0xEE)
    tl, tn = int(f["leaf_off"][-1]), int(f["node_off"][-1])
    d_work = DeviceBuffer(ctx.lib.cel_dev_nmt_verify_workspace_size(tl, tn, f["n"]))
    st = ctx.lib.cel_dev_nmt_verify_batch(
        ctx.handle, f["n"], _p(f["starts"]), _p(f["ends"]), _p(f["ns"]), d_leaves.ptr, _p(f["leaf_off"]),
        ctypes.c_void_p(d_nodes.ptr.value + node_shift), _p(f["node_off"]), ctypes.c_void_p(d_roots.ptr.value + 90),
        f["n"], _p(f["root_idx"]), d_ok.ptr, d_work.ptr, None)
    assert st == _lib.OK, ctx.lib.cel_last_error(ctx.handle).decode()
    synchronize()
    ok = d_ok.download((f["n"],))
    assert set(ok.tolist()) <= {0, 1}
    return [bool(v) for v in ok]


def ref_tree(n, seed, namespaces=None):
    """(namespaces, 512-byte shares, nmt_ref.Tree) of n leaves."""
    rng = np.random.default_rng(seed)
    shares = [rng.integers(0, 256, 512, dtype=np.uint8).tobytes() for _ in range(n)]
    nss = namespaces or nmt_ref.sorted_namespaces(n, rng, parity_from=n - n // 3)
    return nss, shares, nmt_ref.Tree.from_shares(nss, shares)


def range_case(tree_tuple, start, end):
    nss, shares, tree = tree_tuple
    return Case(start, end, nss[start], shares[start:end], tree.prove_range(start, end), tree.root())


def flip(b, byte, bit=0x10):
    x = bytearray(b)
    x[byte] ^= bit
    return bytes(x)


def tampered(c, rng, other_root):
    """One random tampering of case c (rejects, or at least must match the mirror)."""
    kind = int(rng.integers(0, 6))
    if kind == 0 or not c.nodes:
        return c._replace(leaves=[flip(c.leaves[0], int(rng.integers(0, 512)))] + list(c.leaves[1:]))
    if kind == 1:
        i = int(rng.integers(0, len(c.nodes)))
        return c._replace(nodes=c.nodes[:i] + [flip(c.nodes[i], int(rng.integers(0, 90)))] + c.nodes[i + 1:])
    if kind == 2:
        return c._replace(nodes=c.nodes[:-1])
    if kind == 3:
        return c._replace(nodes=c.nodes[::-1])
    if kind == 4:
        return c._replace(root=other_root)
    return c._replace(start=c.start + 1, end=c.end + 1)
