"""A batch's leaves and level 1 by tile class (nmt_kernels.hip): for k >= 16 a wave's 8x8 tile
of 2x2 cell blocks lies wholly inside or outside Q0, and each class has a kernel of its own,
k_leaf_quad_q0 (records through hash_node, the push-order check) and k_leaf_quad_par (digests
through hash_parity_node, no namespace reads at all), each indexing its tiles through
quad_tiles.hpp; below 16 the mixed kernel k_leaf_quad runs as before. What can go wrong, and
the smallest widths at which it can:

  k = 8    the last width on the mixed kernel's side of the dispatch
  k = 16   one Q0 tile and three parity tiles: both launches end in a partial workgroup
           (64 and 192 lanes of 256)
  k = 32   4 + 12 tiles: whole workgroups, several tiles per quadrant, the parity numbering's
           two ranges (right of Q0: 4 tiles, 2 a tile row; below it: 8 tiles, 4 a row)
  k = 64   the first tile rows and columns that touch no quadrant edge

A tile placed wrongly, twice or not at all shows in a root: every level-1 node is written by
exactly one lane. Every batch goes through cel_dev_extend_batch as one chunk on the caller's
stream, two or three distinct squares, with the order check on and off; row roots, column
roots, DAH and status are the oracle's extend_and_commit (test_gpu_parity_records.want), the
status for each square of the batch separately. The squares, seeds and keys of the shape and
namespace cases are those of test_gpu_parity_records, so the oracle computes each once.
"""
import numpy as np
import pytest

import test_gpu_order_check as oc
import test_gpu_parity_records as pr
from eds_inputs import random_ods

EORDER = oc.EORDER


@pytest.mark.gpu
@pytest.mark.parametrize("nsq", [2, 3])
@pytest.mark.parametrize("k", [8, 16, 32, 64])
def test_shapes(ctx, oracle, k, nsq):
    """Random sorted namespaces (the reference's test factory), distinct squares."""
    odss = np.stack([random_ods(k, 8100 + 10 * k + i) for i in range(nsq)])
    assert len({o.tobytes() for o in odss}) == nsq
    wants = pr.both_ways(ctx, oracle, f"shape k={k} n={nsq}", odss)
    assert [w[0] for w in wants] == [0] * nsq


@pytest.mark.gpu
@pytest.mark.parametrize("nsq", [2, 3])
@pytest.mark.parametrize("k", [16, 32])
def test_namespaces(ctx, oracle, k, nsq):
    """The largest namespace on Q0's last row and column (the Q0 kernel's last tile row and
    column carry it into every mixed tree's max); every Q0 share carrying 0xFF*29 (by value
    the Q0 kernel's nodes look like parity nodes: it must still write records, with the
    reference's bytes, from its one form of block 0); a random square."""
    odss = np.stack([pr.max_at_edges(k, 8300 + k), pr.all_parity_namespace(k, 8400 + k), random_ods(k, 8500 + k)])
    wants = pr.both_ways(ctx, oracle, f"join k={k}", odss[:nsq])  # the oracle's keys are (name, square)
    assert [w[0] for w in wants] == [0] * nsq
    edge = odss[0, k - 1, k - 1, :pr.NS]
    assert np.array_equal(wants[0][1][0, pr.NS:2 * pr.NS], edge) and np.array_equal(wants[0][2][0, pr.NS:2 * pr.NS], edge)


def order_batches(k):
    """name -> (squares, the statuses their construction implies). One push-order break per
    broken square, row-only (the cell is below its left neighbour only) or column-only (below
    the cell above only), which test_gpu_order_check.lowered asserts with numpy compares; a
    valid square stands in each batch of three."""
    m = {
        # the first cells that have a left neighbour / a cell above, in the Q0 kernel's tile 0
        "first": ([oc.lowered(k, "row", 0, 1), oc.graded(k, "row"), oc.lowered(k, "col", 1, 0)], [EORDER, 0, EORDER]),
        # Q0's last cell: the last lane of the Q0 launch's last tile, row-only and column-only
        "last": ([oc.lowered(k, "col", k - 1, k - 1), oc.lowered(k, "row", k - 1, k - 1)], [EORDER, EORDER]),
    }
    if k >= 32:
        # across an 8-block (16-cell) tile edge inside Q0: the neighbour's share belongs to
        # another wave's tile. Columns 15 -> 16, rows 15 -> 16, and the corner cell (16, 16)
        # against both neighbouring tiles.
        m["tile_edge"] = ([oc.lowered(k, "row", 7, 16), oc.graded(k, "col"), oc.lowered(k, "col", 16, 9)],
                          [EORDER, 0, EORDER])
        m["tile_corner"] = ([oc.lowered(k, "col", 16, 16), oc.lowered(k, "row", 16, 16)], [EORDER, EORDER])
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("k,name", [(16, "first"), (16, "last"), (32, "first"), (32, "last"), (32, "tile_edge"),
                                    (32, "tile_corner")])
def test_order_breaks(ctx, oracle, k, name):
    squares, statuses = order_batches(k)[name]
    odss = np.stack(squares)
    assert len({o.tobytes() for o in odss}) == len(odss) in (2, 3)
    wants = pr.both_ways(ctx, oracle, f"split order k={k} {name}", odss)
    assert [w[0] for w in wants] == statuses
