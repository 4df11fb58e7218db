"""``(A A')^-1`` for sparse A whose ``A A'`` has a half bandwidth of 65 to 256: the block cyclic
reduction of blocktri.py with blocks of 128 or 256, worked on as tiles of 64 x 64
(csrc/blocktri.hip, second part).

Staged problems with d states per stage have half bandwidth 2 d - 1: blocktri.py ends at
d = 32, this solver at d = 128.  Opt-in (``projector.wide_band("block-tridiagonal-wide")``,
``options={"wide_band": ...}``), which also keeps everything "block-tridiagonal" does.
"""
from .blocktri import BlockTridiagonalNormalSolver

BLOCK_SIZES = (128, 256)       # (the largest is ipx_blockwide_kmax())


def block_size(k):
    """The block edge for half bandwidth k: 128 for 65 ... 128 (and below, should the class be
    given such a matrix), 256 for 129 ... 256."""
    for b in BLOCK_SIZES:
        if k <= b:
            return b
    raise NotImplementedError("A A' has half bandwidth %d after reordering; the wide "
                              "block-tridiagonal solver handles <= %d" % (k, BLOCK_SIZES[-1]))


class WideBlockTridiagonalNormalSolver(BlockTridiagonalNormalSolver):
    """(A A')^-1 by block cyclic reduction in blocks of 128 / 256; attributes and behaviour as
    ``BlockTridiagonalNormalSolver``."""

    _ABI = "blockwide"
    _NAME = "wide block-tridiagonal"
    _block_size = staticmethod(block_size)
