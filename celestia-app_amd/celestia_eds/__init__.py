"""celestia_eds — MI355X-native extended-data-square hot path of celestia-app.

Python view of libcelestia_eds.so (HIP kernels for gfx950 + C ABI), with the
reference's package names: `da` (pkg/da), `wrapper` (pkg/wrapper), `rsmt2d`
(github.com/celestiaorg/rsmt2d), plus `device` for the device-resident batch API
used by bench.py and `block` for the block path from txs (ExtendBlock, ProcessProposal,
PrepareProposal over cel_block_extend) and `blob` for blobs by namespace out of a square
(celestia-node's blob service: GetAll, Get, Included, GetProof) and `fraud` for bad-encoding
fraud proofs (celestia-node's share/eds/byzantine).
"""
from . import _lib, blob, block, da, fraud, rsmt2d, wrapper  # noqa: F401
from .blob import Blob, parse_sparse_shares  # noqa: F401
from ._lib import CelError, Context, default_context, load  # noqa: F401
from .block import ExtendBlock, ExtendBlocks, PrepareProposal, ProcessProposal, ProcessProposals  # noqa: F401
