"""Projection operators Z, LS, Y on the device (reference projections.py).

Formulation: normal equations, the reference's ``NormalEquation`` method
(projections.py:58-90) -- ``v = (AA')^-1 A x``; ``z = x - A'v`` with the same
orthogonality-driven refinement loop (:69-78) and the same measure
``||A z|| / (||A||_F ||z||)`` (:23-55).  The reference's default sparse method
(AugmentedSystem, SuperLU) and dense method (pivoted QR) compute the same
three operators; SURVEY.md section 7 records agreement to <= 4e-16 on the
benchmark problems.

``(AA')^-1`` on MI355X:
  * sparse A whose ``AA'`` is banded (after a bandwidth-reducing row order found
    once per sparsity pattern on the host -- symbolic work only): partitioned
    banded LDL' kernels (csrc/banded.hip);
  * dense A: Gram matrix + dense Cholesky kernels (csrc/dense.hip); under the option
    ``dense_factorization = "householder-qr"`` the reference's own dense method instead, a
    Householder QR of ``A'`` on the device (``DenseQRProjector``, dense_qr.py) -- a sparse A
    ignores the option.
All numeric work of the full-rank path runs on the GPU.  A numerically rank-deficient
Jacobian (a pivot of the device factorization lost against its diagonal) takes the
reference's own exit: a warning and the SVD projections (projections.py:101-108,
181-187,236-287) -- the thin SVD of the (small, dense) matrix is LAPACK on the host as in
the reference, its factors are uploaded once and every operator application is device
matvecs (``SVDProjector``).  Under the option ``rank_deficient = "pivoted-qr"`` a dense device
Jacobian with ``1 <= m <= n`` stays on the device instead: a column-pivoted QR and a complete
orthogonal decomposition (``DenseCODProjector``, dense_cod.py).  Under the option
``sparse_rank_deficient = "skip-pivots"`` a sparse Jacobian stays on the device too: the
nested-dissection Cholesky in pivot-skipping mode and a Woodbury correction over the dropped rows
(``SparseDeficientProjector``, sparse_deficient.py).
"""
from warnings import warn

import ctypes

import numpy as np
import torch

from . import _hip
from . import device as dv
from . import solver_options
from .device import DVec, DeviceCSR, _p, stream_ptr, ctx
from .dense import DenseNormalSolver, DeviceDense
from .factored_projector import FactoredProjector, _Op, operator_triple  # noqa: F401
from .dense_qr import DenseQRProjector
from .dense_cod import DenseCODProjector
from .sparse_deficient import SparseDeficientProjector
from .device_mode import RowSelection
# The solvers, their selection and its options live in modules of their own, layered
#   solver_options < banded < blocktri, blockwide, iterative, nested < band_solver < bordered
#   < linked < boxschur < selection < this one;
# their names stay public here.  (dense < factored_projector < dense_qr < dense_cod < this one:
# the operator object ``_Op`` and the refinement loop the factored projectors share.)
from .solver_options import (WIDE_BAND_POLICIES, wide_band, border_columns, link_rows,  # noqa: F401
                             wide_band_policy, border_columns_limit, link_rows_limit,
                             check_wide_band, check_border_columns, check_link_rows,
                             ITERATIVE_PRECONDS, iterative_precond, iterative_precond_choice,
                             check_iterative_precond, SPARSE_DIRECT, sparse_direct,
                             sparse_direct_choice, check_sparse_direct,
                             DENSE_FACTORIZATIONS, dense_factorization,
                             dense_factorization_choice, check_dense_factorization,
                             RANK_DEFICIENT, rank_deficient, rank_deficient_choice,
                             check_rank_deficient, SPARSE_RANK_DEFICIENT, sparse_rank_deficient,
                             sparse_rank_deficient_choice, check_sparse_rank_deficient)
from .banded import (BandedNormalSolver, BandedNotDecoupled, HANDLE_STATS, _Symbolic,  # noqa: F401
                     _SYMBOLIC_ATTR, _symbolic_for, half_bandwidth_of_aat)
from .blocktri import BlockTridiagonalNormalSolver, block_size  # noqa: F401
from .blockwide import WideBlockTridiagonalNormalSolver  # noqa: F401
from .iterative import IterativeNormalSolver, PcgArgs  # noqa: F401
from .nested import (NestedDissectionNormalSolver, NestedDissectionRefused,  # noqa: F401
                     PivotSkippingNestedSolver, nested_dissection_solver)
from .band_solver import border_reach, direct_band_solver, direct_solver_class  # noqa: F401
from .bordered import (BorderedNormalSolver, BorderedRefused, border_split,  # noqa: F401
                       bordered_solver, _border_split_for)
from .linked import (LinkedRowsNormalSolver, LinkedRefused, link_split, link_solver,  # noqa: F401
                     _link_split_for)
from .boxschur import BoxSchurNormalSolver, wide_band_inner  # noqa: F401
from .selection import (normal_solver_for, solver_name, last_normal_solver,  # noqa: F401
                        _last_solver, _pick_normal_solver, _banded_row_order)

_F64 = torch.float64


def note_solver(ops):
    P = getattr(ops[0], "projector", None)
    if isinstance(P, (NormalEquationProjector, SparseDeficientProjector)):
        _last_solver[0] = solver_name(P.solver)
    else:
        _last_solver[0] = None if P is None else type(P).__name__


class NormalEquationProjector:
    """Z, LS, Y for a device matrix ``A`` with an ``(AA')^-1`` solver object.

    ``stats`` counts solves / refinement steps (SURVEY.md 3.3 measured 0
    refinements on the benchmark; the counters let tests assert the same).
    """

    def __init__(self, A, solver, orth_tol=1e-12, max_refin=3, row_perm=None, lazy_norm=False):
        """``row_perm`` (host ints, or None): ``A`` is the caller's matrix with its rows taken in
        this order (``A = A_caller[row_perm]``: the order in which A A' is banded, see
        ``projections``).  Z does not see the order of the rows; LS returns its multipliers in
        the caller's order and Y takes its right-hand side in it (``rows_in`` for callers that
        hand constraint-space vectors to kernels themselves: cg_fused's priming)."""
        self.A, self.solver = A, solver
        self.orth_tol, self.max_refin = orth_tol, max_refin
        self.m, self.n = A.shape
        self.row_perm = None
        if row_perm is not None:
            inv = np.empty(len(row_perm), dtype=np.int32)
            inv[np.asarray(row_perm)] = np.arange(len(row_perm), dtype=np.int32)
            dev = ctx().device
            self.row_perm = torch.from_numpy(np.ascontiguousarray(row_perm, dtype=np.int32)).to(dev)
            self._row_iperm = torch.from_numpy(inv).to(dev)
        # ||A||_F: computed on first use (a blocking read) -- or handed over by the outer
        # iteration's chain, which folds it into the block it reads anyway (norm_partials)
        self._norm_A = None if (lazy_norm and self.m > 0) else \
            (A.frobenius_norm() if self.m > 0 else 0.0)
        self.stats = {"solves": 0, "refinements": 0, "cancellation_steps": 0}

    @property
    def norm_A(self):
        if self._norm_A is None:
            self._norm_A = self.A.frobenius_norm()
        return self._norm_A

    @norm_A.setter
    def norm_A(self, value):
        self._norm_A = value

    def norm_partials(self):
        """First stage of ``A.frobenius_norm()`` enqueued: (partials, count) -- the fold
        (ipx_sum_partials' order: the bits of the blocking form) is the reader's."""
        val = self.A.val
        g = dv._reduce_grid(val.numel())
        part = dv._empty(2 * g)
        _hip.call("ipx_norms_partials", val.numel(), _p(val), _p(part), stream_ptr())
        return part, g

    # -- reference projections.py:23-55, with ||A z|| from the fused SpMV epilogue
    def _orthogonality(self, z):
        """z's ||z||^2 was left in slot 0 by the SpMV that produced it; A z
        goes to slot 1 so one read-back serves both norms."""
        Az = self.A.spmv(z, reduce=True, slot=1)
        red = self._red = dv.read_slots(7)           # (slot 6: ||x||^2 of null_space's input)
        norm_z, norm_Az = float(np.sqrt(red[0])), float(np.sqrt(red[2]))
        if norm_z == 0 or self.norm_A == 0:
            return 0.0, Az
        return norm_Az / (self.norm_A * norm_z), Az

    def _apply_inv(self, w):
        self.stats["solves"] += 1
        return self.solver.solve(w)

    # x lost this many bits to the row space in z = x - A'v before a correction step is added
    CANCELLATION = 2.0 ** -10

    def null_space(self, x):
        if self.m == 0:
            return x.copy()
        c = dv.ctx()
        # ||x||^2 -> slot 6 (read below together with the orthogonality measure's norms)
        _hip.call("ipx_norms", len(x), dv._p(x.t), ctypes.c_void_p(c.out.data_ptr() + 8 * 6),
                  dv._p(c.ws), dv.stream_ptr())
        v = self._apply_inv(self.A.dot(x))
        z = self.A.rmatvec_sub(v, x, reduce=True)    # x - A'v, ||z||^2 -> slot 0
        k = 0
        while True:                                  # projections.py:72-78
            orth, Az = self._orthogonality(z)
            if k == 0:
                red = self._red
                # Accuracy beyond the reference's loop.  When x lies almost entirely in the row
                # space of A (late barrier subproblems: |Z c| = 1e-6 |c|) the ONE subtraction
                # x - A'v cancels most of x and leaves an error of eps |x| -- 1e-10 of |z| --
                # that the orthogonality measure does not see (it is 1e-13 of ||A||_F |z|):
                # measured 7-9x the reference's augmented-system error on its own late-barrier
                # calls (tests/golden/late_barrier_*.npz).  One correction step on z itself,
                # whose own rounding is eps |z|, removes it: z <- z - A'(A A')^-1 (A z).
                cancelled = red[0] < (self.CANCELLATION ** 2) * red[6]
            else:
                cancelled = False
            if k >= self.max_refin or not (orth > self.orth_tol or cancelled):
                break
            v = self._apply_inv(Az)
            z = self.A.rmatvec_sub(v, z, reduce=True)
            k += 1
            self.stats["refinements" if orth > self.orth_tol else "cancellation_steps"] += 1
        return z

    def null_space_enqueue(self, x, base):
        """``null_space`` without its read-back: z = x - A'(A A')^-1 A x enqueued, and
        ||x||^2, ||z||^2, ||A z||^2 left at doubles ``base + 4``, ``base``, ``base + 2`` of the
        context's reduction block -- the caller (cg_fused.projected_cg's priming) has the
        DEVICE decide from them whether the refinement / cancellation steps above are needed,
        and falls back to ``null_space`` when they are.  (slot = base / 2: 16 bytes each.)"""
        c = dv.ctx()
        _hip.call("ipx_norms", len(x), dv._p(x.t), ctypes.c_void_p(c.out.data_ptr() + 8 * (base + 4)),
                  dv._p(c.ws), dv.stream_ptr())
        v = self._apply_inv(self.A.dot(x))
        z = self.A.rmatvec_sub(v, x, reduce=True, slot=base // 2)
        self.A.spmv(z, reduce=True, slot=base // 2 + 1)
        return z

    def _gather_rows(self, v, idx):
        out = dv._empty(idx.numel())
        _hip.call("ipx_gather", idx.numel(), dv._p(v.t), dv._p(idx), None, None, dv._p(out),
                  dv.stream_ptr())
        return DVec(out)

    def rows_in(self, b):
        """A constraint-space vector of the caller in this projector's row order."""
        return b if self.row_perm is None else self._gather_rows(b, self.row_perm)

    def least_squares(self, x):
        if self.m == 0:
            return DVec.zeros(0)
        v = self._apply_inv(self.A.dot(x))
        for _ in range(getattr(self.solver, "refine_steps", 0)):     # ill-conditioned dense A
            v = v + self._apply_inv(self.A.dot(self.A.rmatvec_sub(v, x)))
        return v if self.row_perm is None else self._gather_rows(v, self._row_iperm)

    def row_space(self, x):
        if self.m == 0:
            return DVec.zeros(self.n)
        x = self.rows_in(x)
        y = self.A.T.dot(self._apply_inv(x))
        for _ in range(getattr(self.solver, "refine_steps", 0)):
            y = y + self.A.T.dot(self._apply_inv(x - self.A.dot(y)))
        return y

    def operators(self):
        return operator_triple(self)


class SVDProjector(FactoredProjector):
    """Z, LS, Y from a thin SVD ``A = U diag(s) Vt`` with the singular values ``<= tol``
    dropped -- the reference's ``svd_factorization_projections`` (projections.py:236-287)
    statement by statement, on device vectors.  Reached for rank-deficient Jacobians (with
    the reference's warning) and for ``method='SVDFactorization'``."""

    MAX_ELEMENTS = 1 << 25      # dense copy of A on the host: 256 MiB

    def __init__(self, A, orth_tol, max_refin, tol):
        import scipy.linalg
        FactoredProjector.__init__(self, A, orth_tol, max_refin)
        if self.m * self.n > self.MAX_ELEMENTS:
            raise np.linalg.LinAlgError(
                "Singular Jacobian matrix (%d x %d): too large for the dense SVD fallback"
                % (self.m, self.n))
        Ah = A.to_scipy().toarray() if isinstance(A, DeviceCSR) else A.to_host()
        U, sv, Vt = scipy.linalg.svd(Ah, full_matrices=False)       # :240
        keep = sv > tol                                             # :243-245
        self.rank = int(np.count_nonzero(keep))
        self.U = DeviceDense.from_host(U[:, keep])
        self.Vt = DeviceDense.from_host(Vt[keep, :])
        self.inv_s = DVec.from_host(1.0 / sv[keep])
        self._measure_norm_A()

    def _apply_inv(self, x):
        """v = U 1/s V' x = pinv(A') x  (:250-253)"""
        self.stats["solves"] += 1
        if self.rank == 0:
            return DVec.zeros(self.m)
        return self.U.dot(self.inv_s * self.Vt.dot(x))

    def row_space(self, x):                                         # :281-286
        if self.rank == 0:
            return DVec.zeros(self.n)
        return self.Vt.T.dot(self.inv_s * self.U.T.dot(x))


def orthogonality(A, g):
    """``||A g|| / (||A||_F ||g||)`` (reference projections.py:23-55)."""
    A = as_device_matrix(A)
    g = g if isinstance(g, DVec) else DVec.from_host(g)
    norm_g = dv.norm(g)
    norm_A = A.frobenius_norm()
    if norm_g == 0 or norm_A == 0:
        return 0
    return dv.norm(A.dot(g)) / (norm_A * norm_g)


def as_device_matrix(A):
    """Upload a scipy sparse matrix / ndarray (device matrices pass through).
    An empty matrix is forced to the sparse representation like the
    reference does (projections.py:368-369)."""
    import scipy.sparse as sps
    if isinstance(A, DeviceCSR):
        return A.with_sorted_indices()
    if isinstance(A, DeviceDense):
        return A
    m, n = np.shape(A)
    if sps.issparse(A) or m * n == 0:
        return DeviceCSR.from_scipy(sps.csr_matrix(A))
    return DeviceDense.from_host(np.asarray(A, dtype=float))


def _rows_in_order(A, perm):
    """``A[perm]`` as a value refresh on a pattern derived once from A's (cached on it)."""
    sel = getattr(A.pattern, "_ipx_rows_in_order", None)
    if sel is None:
        sel = A.pattern._ipx_rows_in_order = RowSelection(A.pattern, np.asarray(perm, dtype=np.int64), None)
    return sel.apply(A)


def projections(A, method=None, orth_tol=1e-12, max_refin=3, tol=1e-15, deferred=None):
    """Device counterpart of ``projections`` (projections.py:290-406).

    ``A`` is a DeviceCSR / DeviceDense (or a scipy / numpy matrix, uploaded).
    ``method`` accepts the reference's names; every one maps to the device
    normal-equation solve (the operators are the same; see module docstring).
    """
    A = as_device_matrix(A)
    # The SAME matrix object with unchanged values: the factorization made for it is returned.
    # Values declared immutable (``constant``: linear constraints, N1) are factored once per
    # solve; any other matrix is recognised by its value tensor's version counter -- the
    # barrier method hands the Jacobian of its last accepted point to the next subproblem
    # (tr_interior_point.py:338-340: the reference refactors it, 11 of config 3's 25
    # factorizations).
    #
    # What the version counter does NOT see: writes through raw pointers (a user kernel, or this
    # library's own ipx_* entry points called on ``A.val`` directly).  A callback that refills a
    # preallocated value tensor that way must say so -- ``projector.invalidate(A)`` -- or go
    # through torch ops (``A.val.copy_(...)``), which bump the counter.  The entry keeps a
    # reference to the tensor it was made for: a reassigned ``A.val`` can then never collide
    # with a collected tensor's id.
    t, version = _values_version(A)
    key = (method, orth_tol, max_refin, tol, version, solver_options.current().key())
    cached = getattr(A, "_ipx_projections", None)
    if cached is not None and version is not None and cached[0] == key and cached[2] is t:
        # (a caller that cannot take a pending verdict along gets it settled first)
        if deferred is not None or confirm(A, cached[1]):
            note_solver(cached[1])           # (a factorization reused is still the last one)
            return cached[1]
    out = _projections(A, method, orth_tol, max_refin, tol, deferred)
    note_solver(out)
    try:
        A._ipx_projections = (key, out, t)
    except AttributeError:
        pass
    return out


def confirm(A, ops):
    """Settle a factorization whose verdict is still pending (``BandedNormalSolver.pending``)
    by a blocking read of its own; a verdict that differs from the assumed one forgets the
    factorization (the next ``projections(A)`` factors again, blocking).  True: ``ops`` stand."""
    P = getattr(ops[0], "projector", None)
    solver = getattr(P, "solver", None)
    if solver is None or not getattr(solver, "pending", False):
        return True
    bad = dv.read_doubles(solver._verdict, 1)[0] != 0
    solver.pending = False
    if bad:
        invalidate(A)
    return not bad


def invalidate(A):
    """Forget the factorization cached on a device matrix (its values were rewritten in place
    behind torch's back: see ``projections``)."""
    try:
        A._ipx_projections = None
    except AttributeError:
        pass


def _values_version(A):
    """(tensor that holds a device matrix's values, its version counter); (None, None) for an
    unknown type: never cached."""
    t = getattr(A, "val", None)
    if t is None:
        t = getattr(A, "t", None)
    return t, getattr(t, "_version", None)


def _projections(A, method, orth_tol, max_refin, tol, deferred=None):
    sparse = isinstance(A, DeviceCSR)
    if sparse:
        if method not in (None, "NormalEquation", "AugmentedSystem"):
            raise ValueError("Method not allowed for sparse matrix.")
    else:
        if method not in (None, "QRFactorization", "SVDFactorization"):
            raise ValueError("Method not allowed for dense array.")
    m, n = A.shape
    if method == "SVDFactorization":
        return SVDProjector(A, orth_tol, max_refin, tol).operators()
    A_caller, row_perm, solver = A, None, None
    # the device exit for a rank-deficient sparse Jacobian (whatever ``sparse_direct`` says: that
    # option decides the first attempt only)
    skip_pivots = sparse and m >= 1 \
        and solver_options.current().sparse_rank_deficient == "skip-pivots"
    ill = ("Ill-conditioned Jacobian matrix (a pivot of A A' lost 43 bits); too large for "
           "the dense SVD fallback: keeping the factorization under iterative refinement.")
    try:
        if sparse and m > 0:
            # A A' banded only after a reordering of the rows (equality rows stacked on
            # inequality rows: _canonical_constraint.py:169-360): factor the matrix WITH ITS ROWS
            # IN THAT ORDER instead of permuting inside every solve -- the projections do not see
            # the order of the rows, and the device-resident CG loop (cg_fused) takes any matrix
            # whose natural order is banded
            row_perm = _banded_row_order(A)
            if row_perm is not None:
                A = _rows_in_order(A, row_perm)
        if isinstance(A, DeviceDense) and m > 0 \
                and solver_options.current().dense_factorization == "householder-qr":
            # (LinAlgError when min |R_jj| / ||a_j|| < 2^-43: the exits below, as for a lost
            # pivot of the Cholesky factorization)
            return DenseQRProjector(A, orth_tol, max_refin).operators()
        solver = None if m == 0 else (normal_solver_for(A) if deferred is None
                                      else normal_solver_for(A, deferred))
        inner = getattr(solver, "inner", solver)           # (box-Schur: its banded Schur solve)
        if getattr(inner, "ill_conditioned", False):
            if skip_pivots or m * n <= SVDProjector.MAX_ELEMENTS:
                raise np.linalg.LinAlgError("numerically rank deficient")
            warn(ill)
    except np.linalg.LinAlgError:
        # the reference's exits: projections.py:101-108 (sparse), :181-187 (dense)
        if solver_options.current().rank_deficient == "pivoted-qr" \
                and isinstance(A_caller, DeviceDense) and 1 <= m <= n:
            # (whichever dense factorization raised: a lost Cholesky pivot, ``ill_conditioned``,
            # the Householder pivot ratio)
            warn("Singular Jacobian matrix. Using a pivoted QR decomposition on the device to "
                 "perform the factorizations.")
            return DenseCODProjector(A_caller, orth_tol, max_refin).operators()
        if skip_pivots:
            try:
                P = SparseDeficientProjector(A_caller, orth_tol, max_refin)
            except (NestedDissectionRefused, np.linalg.LinAlgError):
                P = None         # past the nested solver's limits, or more than 32 dropped rows
            if P is not None:
                warn("Singular Jacobian matrix. Using a pivot-skipping sparse Cholesky "
                     "factorization on the device to perform the factorizations.")
                return P.operators()
            if solver is not None and m * n > SVDProjector.MAX_ELEMENTS:
                # (``ill_conditioned`` past the host exit's cap: as without the option)
                warn(ill)
                return NormalEquationProjector(A, solver, orth_tol, max_refin, row_perm=row_perm,
                                               lazy_norm=deferred is not None).operators()
        warn("Singular Jacobian matrix. Using dense SVD decomposition to perform the "
             "factorizations." if sparse else
             "Singular Jacobian matrix. Using SVD decomposition to perform the "
             "factorizations.")
        return SVDProjector(A_caller, orth_tol, max_refin, tol).operators()
    return NormalEquationProjector(A, solver, orth_tol, max_refin, row_perm=row_perm,
                                   lazy_norm=deferred is not None).operators()

