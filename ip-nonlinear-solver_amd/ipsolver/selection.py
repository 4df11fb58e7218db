"""Which ``(A A')^-1`` solver takes a device matrix: an ordered list of rules (DESIGN.md section
4 has the same list as a table).  A rule looks at the matrix and at pattern facts that are
computed on first use, and returns a factored solver or None: the next rule's turn.
"""
import functools

from . import _hip
from .band_solver import border_reach, direct_band_solver
from .banded import BandedNormalSolver, BandedNotDecoupled, _symbolic_for, half_bandwidth_of_aat
from .blocktri import BlockTridiagonalNormalSolver
from .bordered import BorderedNormalSolver, _border_split_for, bordered_solver
from .boxschur import BoxSchurNormalSolver, analysis_for, general_rows_pattern
from .dense import DenseNormalSolver, DeviceDense
from .iterative import IterativeNormalSolver
from .linked import LinkedRowsNormalSolver, _link_split_for, link_solver
from .nested import nested_dissection_solver
from .solver_options import current

_last_solver = [None]
_fact = functools.cached_property


class _Facts:
    """Pattern facts of one sparse matrix under the options in force.  Host work only, each fact
    computed when a rule first asks for it (the order matters: the symbolic analysis of a 1e6-row
    barrier Jacobian costs 0.1 s and is skipped when an earlier rule takes the matrix) and cached
    on the pattern by the functions called here."""

    def __init__(self, A):
        self.pattern = A.pattern
        self.kmax = _hip.load().ipx_banded_kmax()
        self.wide = current().wide_band != "iterative"
        self.reach = border_reach()     # the widest band a direct solver takes under the policy

    @_fact
    def natural_k(self):
        """half bandwidth of A A' in the caller's row order: O(nnz)"""
        return half_bandwidth_of_aat(self.pattern)

    @_fact
    def symbolic(self):
        return _symbolic_for(self.pattern)

    @property
    def k(self):
        """half bandwidth of A A' after reordering"""
        return self.symbolic.k

    @_fact
    def box_any(self):
        """the box-Schur elimination applies, the general rows being of any sparsity"""
        return analysis_for(self.pattern).worthwhile

    @property
    def general(self):
        """pattern of the rows the box-Schur elimination leaves to its inner solver (not kept
        here: the device selection's pattern takes the host pattern's place once it exists)"""
        return general_rows_pattern(self.pattern)

    @_fact
    def general_k(self):
        """half bandwidth (after reordering) of A_R A_R', A_R the general rows"""
        return _symbolic_for(self.general).k

    @_fact
    def box_banded(self):
        """the box-Schur elimination applies and the general rows alone are banded"""
        return self.box_any and self.general_k <= self.kmax

    @_fact
    def border_split(self):
        return _border_split_for(self.pattern)

    @_fact
    def link_split(self):
        return _link_split_for(self.pattern)


def _band_plus_rule(limit, solver_for, split_for, solver_class):
    """(L1)/(L2) and (D1)/(D2): a band plus a few dense rows (linked.py) or columns (bordered.py)
    -- the matrix itself, or the general rows under the box-Schur elimination (a linking
    inequality of a barrier problem with a box).  A refusal in either place is the next rule's
    turn."""
    def rule(A, f, deferred):
        if getattr(current(), limit) < 1:
            return None
        solver = solver_for(A)                                              # (L1) (D1)
        if solver is None and f.box_any and split_for(f.general) is not None:
            solver = BoxSchurNormalSolver(A, any_sparsity=True)             # (L2) (D2)
            if not isinstance(solver.inner, solver_class):
                return None
        return solver
    return rule


_rule_link_rows = _band_plus_rule("link_rows", link_solver, _link_split_for, LinkedRowsNormalSolver)
_rule_border_columns = _band_plus_rule("border_columns", bordered_solver, _border_split_for,
                                       BorderedNormalSolver)


def _box_schur_banded(A, f):
    """Bound rows eliminated analytically, the Schur complement of the general rows to the banded
    solver.  When that one finds the complement a coupled wide band (``BandedNotDecoupled``):
    (W1) under a wide-band policy the complement is a band for the block-tridiagonal solver;
    else the elimination buys nothing and the rules below solve with A itself."""
    try:
        return BoxSchurNormalSolver(A)
    except BandedNotDecoupled:
        return BoxSchurNormalSolver(A, any_sparsity=True) if f.wide else None


def _rule_barrier_jacobian(A, f, deferred):
    """The barrier problem's augmented Jacobian: a general row couples with the two bound rows of
    each of its variables, no reordering of A A' is narrow -- its symbolic analysis is not even
    tried."""
    if f.natural_k > f.kmax and f.box_banded:
        return _box_schur_banded(A, f)


def _rule_box_over_wide_band(A, f, deferred):
    """(W2) bound rows eliminated in closed form, the general rows' Schur complement
    J (I - W) J' + S^2 (the pattern of A_R A_R') factored directly, for any m."""
    if f.wide and f.box_any and f.kmax < f.general_k <= f.reach:
        return BoxSchurNormalSolver(A, any_sparsity=True)


def _rule_banded(A, f, deferred):
    if f.k > f.kmax:
        return None
    try:
        return BandedNormalSolver(A, deferred=deferred)
    except BandedNotDecoupled:
        # Half bandwidths 5-8 on a long band run the single-launch decoupled solve (the
        # separator system, half bandwidth 2k-1, is only formed to test that its blocks
        # decouple).  When they do not, a serial sweep would take 80-100 ms per solve at
        # m = 1e5: the device-resident preconditioned CG is 20x faster and as accurate
        # after the projector's refinement (profiles/r02_banded_by_bandwidth.txt).
        if f.wide:
            return BlockTridiagonalNormalSolver(A)                          # (W1) blocks of 16, any m
        if A.shape[0] > DenseNormalSolver.MAX_ROWS_FROM_SPARSE:
            return IterativeNormalSolver(A)


def _rule_box_schur(A, f, deferred):
    if f.box_banded:
        return _box_schur_banded(A, f)


def _rule_wide_band(A, f, deferred):
    """(W3) block cyclic reduction, any m"""
    if f.k > f.kmax:
        return direct_band_solver(A)


def _rule_sparse_direct(A, f, deferred):
    """Under the option sparse_direct: the nested-dissection multifrontal Cholesky for a matrix no
    band solver took, of any m.  A matrix with worthwhile box rows stays with the box-Schur
    elimination below (whose inner choice gets this solver under the option); a matrix past the
    solver's limits is the next rule's turn."""
    if not f.box_any:
        return nested_dissection_solver(A)


def _rule_dense(A, f, deferred):
    if A.shape[0] <= DenseNormalSolver.MAX_ROWS_FROM_SPARSE:
        return DenseNormalSolver(A)             # wide band: dense Cholesky of A A'


def _rule_box_schur_any_sparsity(A, f, deferred):
    """A barrier problem with a Jacobian of general sparsity (the reference factors any pattern
    with SuperLU, projections.py:93-172): the bound rows -- two thirds of the matrix, and the ones
    whose slacks ruin the conditioning of A A' late in the barrier run -- are still eliminated in
    closed form; what is left to the dense / iterative solver is the Schur complement of the
    general rows, J (I - W) J' + S^2."""
    if f.box_any:
        return BoxSchurNormalSolver(A, any_sparsity=True)


def _rule_iterative(A, f, deferred):
    return IterativeNormalSolver(A)             # general sparsity: matrix-free solve


# (a rule put before ``_rule_banded`` that takes matrices whose A A' a row order makes narrow has to
# be mirrored in ``_banded_row_order`` below, which predicts the banded rule's turn from the facts;
# ``_rule_sparse_direct`` sits after ``_rule_banded`` and needs no mirror there)
RULES = (_rule_link_rows, _rule_border_columns, _rule_barrier_jacobian, _rule_box_over_wide_band,
         _rule_banded, _rule_box_schur, _rule_wide_band, _rule_sparse_direct, _rule_dense,
         _rule_box_schur_any_sparsity, _rule_iterative)


def _pick_normal_solver(A, deferred=None):
    if isinstance(A, DeviceDense):
        return DenseNormalSolver(A)
    facts = _Facts(A)
    for rule in RULES:
        solver = rule(A, facts, deferred)
        if solver is not None:
            return solver


def normal_solver_for(A, deferred=None):
    """The ``(A A')^-1`` solver ``projections`` picks for a full-row-rank device matrix."""
    solver = _pick_normal_solver(A, deferred)
    _last_solver[0] = solver_name(solver)
    return solver


def _banded_row_order(A):
    """The row order in which A A' is banded when the natural one is not and the banded solver
    would be the choice of ``normal_solver_for``: not the box-Schur elimination, which has its
    own row bookkeeping, nor the bordered or the linked solver, whose band has its own order (A A'
    is full).  None otherwise."""
    f = _Facts(A)
    if f.natural_k <= f.kmax or f.box_banded or f.border_split is not None \
            or f.link_split is not None:
        return None
    return f.symbolic.perm if f.k <= f.kmax else None


def solver_name(solver):
    """Class name of a normal-equation solver; ``Outer/Inner`` (recursively) for a solver that
    sits on an inner one: the box-Schur elimination, the bordered and the linked solver."""
    if solver is None:
        return None
    name = type(solver).__name__
    inner = getattr(solver, "inner", None)
    return name if inner is None else "%s/%s" % (name, solver_name(inner))


def last_normal_solver():
    """``solver_name`` of the factorization ``projections`` handed out last, made then or taken
    from its cache ("SVDProjector" for the SVD exit); None: none yet, or a Jacobian without
    rows, which has nothing to factor."""
    return _last_solver[0]
