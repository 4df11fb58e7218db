"""Which direct solver takes a band: the one place that maps a half bandwidth of ``A A'`` and the
wide-band policy in force (solver_options.py) to the banded, the block-tridiagonal or the wide
block-tridiagonal solver."""
from . import _hip
from .banded import BandedNormalSolver, _symbolic_for
from .blocktri import BlockTridiagonalNormalSolver
from .blockwide import WideBlockTridiagonalNormalSolver
from .solver_options import current


def border_reach():
    """The largest half bandwidth of ``A A'`` that a direct band solver takes under the policy in
    force (the banded solver's, the block-tridiagonal solver's, the wide one's): what the band of
    a bordered or linked matrix may have."""
    lib = _hip.load()
    policy = current().wide_band
    if policy == "block-tridiagonal-wide":
        return lib.ipx_blockwide_kmax()
    return lib.ipx_blocktri_kmax() if policy == "block-tridiagonal" else lib.ipx_banded_kmax()


def direct_solver_class(k):
    """The direct band solver for half bandwidth k: banded, block tridiagonal, or wide block
    tridiagonal (which itself refuses k past ``ipx_blockwide_kmax()``), whatever the policy."""
    lib = _hip.load()
    if k <= lib.ipx_banded_kmax():
        return BandedNormalSolver
    return BlockTridiagonalNormalSolver if k <= lib.ipx_blocktri_kmax() \
        else WideBlockTridiagonalNormalSolver


def direct_band_solver(B, whatever_the_policy=False, banded_has_refused=False):
    """The direct solver of ``B B'`` for a caller with no other use for B, factored; None when
    the half bandwidth (after B's own reordering) is past ``border_reach()``.  Errors of the
    factorization (``LinAlgError``, ``BandedNotDecoupled``) are the caller's.

    ``whatever_the_policy``: the reach is not asked -- the bordered solver, whose split was made
    under that condition or by a caller who chose the columns.

    ``banded_has_refused``: the banded solver is not offered; half bandwidths up to its limit go
    to the block-tridiagonal solver (blocks of 16) where the policy allows that solver at all, and
    to nobody under "iterative".  For the inner solver of the box-Schur elimination of any
    sparsity: a Schur complement this narrow comes there only after the banded solver has refused
    it as ``BandedNotDecoupled`` (selection.py, (W1)), and would be refused again."""
    if banded_has_refused and current().wide_band == "iterative":
        return None                     # (before any analysis of B: nobody is offered)
    k = _symbolic_for(B.pattern).k
    if not whatever_the_policy and k > border_reach():
        return None
    if banded_has_refused and k <= _hip.load().ipx_banded_kmax():
        return BlockTridiagonalNormalSolver(B)
    return direct_solver_class(k)(B)
