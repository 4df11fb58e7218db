"""User-facing constraint classes (host-side plumbing of the drop-in boundary).

Same constructors, ``kind`` grammar, feasibility rules and error messages as
the reference's ``ipsolver/_constraints.py`` (cited per function); nothing
here is on the GPU hot path -- these objects only wrap the user's callbacks
and hand their values to the canonical form (``canonical.py``).
"""
from warnings import warn

import numpy as np
import scipy.sparse as sps

from .fd import FiniteDifferenceOperator, FD_METHODS
from .fd_hessian import SparseFD, FDTerm, Memo
from . import quasi_newton as _qn

__all__ = ['NonlinearConstraint', 'LinearConstraint', 'BoxConstraint']

_INFEASIBLE = ("Unfeasible initial point. Either set ``enforce_feasibility=False`` "
               "or choose a new feasible initial point ``x0``.")


def _is_operator(H):
    """LinearOperator-like: has .dot/.matvec but is neither ndarray nor sparse."""
    return (not sps.issparse(H) and not isinstance(H, (np.ndarray, list, tuple))
            and (hasattr(H, "matvec") or hasattr(H, "dot")) and hasattr(H, "shape"))


def wrap_hessian(hess, sample, nargs):
    """Normalise a user Hessian callback by the type of its first return value
    (reference _constraints.py:117-134, _minimize_constrained.py:395-412):
    sparse -> csr_matrix, operator -> as is, anything else -> 2-D ndarray."""
    if sps.issparse(sample):
        return lambda *a: sps.csr_matrix(hess(*a))
    if _is_operator(sample):
        return lambda *a: hess(*a)
    return lambda *a: np.atleast_2d(np.asarray(hess(*a)))


def canonical_csr(M):
    """``M`` as a CSR matrix in canonical format: column indices sorted within every row and
    no (row, column) entry stored twice.  scipy defines repeated entries as summed; the device
    assembly of ``A A'`` (merge joins of sorted rows) and every symbolic analysis of a pattern
    assume each entry once, so repeats are summed here, on a copy: the caller's matrix is never
    changed.  A matrix that is canonical already is returned as is (no copy of its arrays)."""
    M = sps.csr_matrix(M)
    if not M.has_canonical_format:
        M = M.copy()
        M.sum_duplicates()
    return M


def check_kind(kind, m):
    """Validate / broadcast ``kind`` (reference _constraints.py:370-411)."""
    if not isinstance(kind, (tuple, list, str)):
        raise ValueError("The parameter `kind` should be a tuple,  a list, or a string.")
    if isinstance(kind, str):
        kind = (kind,)
    if len(kind) == 0:
        raise ValueError("The parameter `kind` should not be empty.")
    keyword, nargs = kind[0], len(kind)
    if keyword not in ("greater", "less", "equals", "interval"):
        raise ValueError("Keyword `%s` not available." % keyword)
    one_sided = keyword in ("greater", "less", "equals")
    if (nargs in (1, 2) and not one_sided) or (nargs == 3 and keyword != "interval"):
        raise ValueError("Invalid `kind` format.")
    if nargs == 1:
        kind = (keyword, 0)

    def bound(value, label):
        value = np.asarray(value, dtype=float)
        if np.size(value) not in (1, m):
            raise ValueError("`%s` has the wrong dimension." % label)
        # (np.resize of a scalar to 1e5 rows is a 5 ms concatenate loop)
        return np.full(m, float(value.reshape(-1)[0])) if np.size(value) == 1 \
            else np.array(value).reshape(m)

    if one_sided:
        label = {"greater": "lb", "less": "ub", "equals": "c"}[keyword]
        return (keyword, bound(kind[1], label))
    lb, ub = bound(kind[1], "lb"), bound(kind[2], "ub")
    if (lb > ub).any():
        raise ValueError("lb[i] > ub[i].")
    return (keyword, lb, ub)


def check_enforce_feasibility(flag, m):
    """Reference _constraints.py:414-426."""
    if isinstance(flag, bool):
        return np.full(m, flag, dtype=bool)
    flag = np.array(flag, dtype=bool)
    if flag.size != m:
        raise ValueError("The parameter 'enforce_feasibility' has the wrong "
                         "number of elements.")
    return flag


def kind_bounds(kind):
    """(lb, ub) arrays implied by a checked ``kind``."""
    keyword = kind[0]
    if keyword == "equals":
        return kind[1], kind[1]
    if keyword == "greater":
        return kind[1], np.full_like(kind[1], np.inf)
    if keyword == "less":
        return np.full_like(kind[1], -np.inf), kind[1]
    if keyword == "interval":
        return kind[1], kind[2]
    raise RuntimeError("Never be here.")


def is_feasible(kind, enforce, f0):
    """Only rows with enforce_feasibility are tested (reference :429-447)."""
    lb, ub = kind_bounds(kind)
    return bool((lb[enforce] <= f0[enforce]).all() and (f0[enforce] <= ub[enforce]).all())


def reinforce_box(kind, enforce, x0, rtol=0.01, atol=0.01):
    """Move enforced coordinates strictly inside their bounds (reference
    :450-477): margin min(atol, rtol*(ub-lb)) from each finite bound."""
    lb, ub = kind_bounds(kind)
    x = np.array(x0, dtype=float)
    for i in np.flatnonzero(enforce):
        if not np.isinf(lb[i]):
            x[i] = max(x[i], min(lb[i] + atol, lb[i] + rtol * (ub[i] - lb[i])))
        if not np.isinf(ub[i]):
            x[i] = min(x[i], max(ub[i] - atol, ub[i] - rtol * (ub[i] - lb[i])))
    return x


class _Initialised:
    """Fields every constraint exposes after ``evaluate_and_initialize``."""
    isinitialized = False

    def _finish(self, x0, f0):
        self.x0, self.f0 = x0, f0
        self.n, self.m = x0.size, f0.size
        self.kind = check_kind(self.kind, self.m)
        self.enforce_feasibility = check_enforce_feasibility(self.enforce_feasibility, self.m)


def check_fd_jacobian_arguments(jac, hess, sparsity, rel_step):
    """Construction-time checks of ``NonlinearConstraint``'s finite-difference arguments."""
    if isinstance(jac, str):
        if jac not in FD_METHODS:
            raise ValueError("`jac` must be callable or one of %r, got %r" % (FD_METHODS, jac))
        if isinstance(hess, SparseFD):
            raise ValueError("hess=%r cannot be combined with a finite-difference `jac` (%r): it "
                             "would difference a differenced Jacobian; pass a callable `jac`, or "
                             "use the operator form hess='2-point' / '3-point'" % (hess, jac))
        if jac == 'cs' and isinstance(hess, str) and hess in FD_METHODS:
            raise ValueError("jac='cs' cannot be combined with a finite-difference `hess` (%r): "
                             "complex steps do not nest; pass a callable `hess`, None, or use "
                             "jac='2-point' / '3-point'" % (hess,))
    elif sparsity is not None or rel_step is not None:
        raise ValueError("`finite_diff_jac_sparsity` and `finite_diff_rel_step` apply to a "
                         "finite-difference `jac` ('2-point', '3-point', 'cs') only; `jac` is "
                         "callable")


class _FDJacobian:
    """``jac(x)`` by finite differences of ``fun`` (numpy callbacks): ``approx_derivative`` on a
    plan built once.  ``nfev`` counts the calls of ``fun`` spent on differences: G per
    evaluation (2 G for '3-point') plus one for ``f0`` at every point but ``x0`` ('2-point' and
    '3-point'; 'cs' needs none)."""

    def __init__(self, fun, method, sparsity, rel_step, n, m):
        from ._numdiff import _plan_for
        self.fun, self.method, self.rel_step = fun, method, rel_step
        self.plan, self.dense = _plan_for(sparsity, n, m)

    @property
    def nfev(self):
        return self.plan.nfev

    def __call__(self, x, f0=None):
        from ._numdiff import approx_derivative
        if self.method == 'cs' and f0 is None:
            f0 = np.zeros(self.plan.m)          # (not used by the complex step: spare the call)
        return approx_derivative(self.fun, x, self.method, self.rel_step, f0,
                                 sparsity=self.plan)


class NonlinearConstraint(_Initialised):
    """``lb <= fun(x) <= ub`` style constraint (reference _constraints.py:14-167).

    ``NonlinearConstraint(fun, kind, jac, hess='2-point', enforce_feasibility=False,
    finite_diff_jac_sparsity=None, finite_diff_rel_step=None)``

    ``jac`` is a callable or '2-point' / '3-point' / 'cs': the Jacobian by finite differences of
    ``fun`` (``_numdiff.approx_derivative``; scipy's keyword names).  ``finite_diff_jac_sparsity``
    is a sparsity structure or ``(structure, groups)``; without it the difference is dense (n
    evaluations; refused in device-callback mode).

    ``hess`` is a callable ``hess(x, v)``, None, '2-point' / '3-point' / 'cs' (the operator form:
    differences of ``x -> J(x)' v`` inside every CG iteration), ``SparseFD(...)`` (the same
    difference assembled into a CSR term once per accepted point) or a quasi-Newton strategy,
    ``ipsolver.LBFGS(...)`` / ``ipsolver.LSR1(...)``, in both callback modes and with any
    ``jac``.  With a strategy the constraint's curvature is a term of ONE limited-memory
    approximation of the Lagrangian's Hessian (``quasi_newton.LagrangianQN``): its pair takes
    ``(J(x+) - J(x))' v`` from the Jacobians the solver evaluates anyway -- no extra calls of
    ``jac`` -- and the CG loops apply it as one low-rank term.  Every constraint with a strategy,
    and the objective if ``minimize_constrained(hess=...)`` is one, must carry EQUAL strategies
    (a ``ValueError`` otherwise).  The Lagrangian's Hessian is usually indefinite, so ``LSR1``
    is the rule to prefer here; ``LBFGS`` skips every pair with ``s'y <= min_curvature ||s||
    ||y||``.
    """

    def __init__(self, fun, kind, jac, hess='2-point', enforce_feasibility=False,
                 finite_diff_jac_sparsity=None, finite_diff_rel_step=None):
        check_fd_jacobian_arguments(jac, hess, finite_diff_jac_sparsity, finite_diff_rel_step)
        self._fun, self._jac, self._hess = fun, jac, hess
        self.kind = kind
        self.enforce_feasibility = enforce_feasibility
        self.finite_diff_jac_sparsity = finite_diff_jac_sparsity
        self.finite_diff_rel_step = finite_diff_rel_step

    def evaluate_and_initialize(self, x0, sparse_jacobian=None):
        x0 = np.atleast_1d(x0).astype(float)
        f0 = np.atleast_1d(self._fun(x0))
        if isinstance(self._jac, str):
            user_jac = self.fd_jacobian = _FDJacobian(
                lambda x: np.atleast_1d(self._fun(x)), self._jac, self.finite_diff_jac_sparsity,
                self.finite_diff_rel_step, x0.size, f0.size)
            J0 = user_jac(x0, f0)
        else:
            user_jac = self._jac
            J0 = user_jac(x0)

        self.fun = lambda x: np.atleast_1d(self._fun(x))
        self.sparse_jacobian = bool(sparse_jacobian
                                    or (sparse_jacobian is None and sps.issparse(J0)))
        if isinstance(self._hess, SparseFD):
            # the Jacobian the solver evaluated at the Hessian's point is the f0 of the difference
            self.fd_hessian = FDTerm(self._hess, x0.size, "constraint")
            user_jac = memo = Memo(user_jac, x0, J0)
        elif _qn.is_strategy(self._hess):
            # a term of the Lagrangian's one quasi-Newton memory: its request carries the
            # Jacobian the solver evaluated at the Hessian's point
            self.qn_hessian = self._hess
            user_jac = memo = Memo(user_jac, x0, J0, reuse=True)
        if self.sparse_jacobian:
            self.jac = lambda x: canonical_csr(user_jac(x))
            self.J0 = canonical_csr(J0)
        else:
            def dense_jac(x):
                J = user_jac(x)
                return J.toarray() if sps.issparse(J) else np.atleast_2d(J)
            self.jac = dense_jac
            self.J0 = J0.toarray() if sps.issparse(J0) else np.atleast_2d(J0)

        if callable(self._hess):
            self.hess = wrap_hessian(self._hess, self._hess(x0, np.zeros_like(f0)), 2)
        elif self._hess in FD_METHODS:
            method, jac = self._hess, self.jac

            def fd_hess(x, v):          # d/dx [J(x)' v] by differences (:136-146)
                return FiniteDifferenceOperator(lambda y: jac(y).T.dot(v), x, method)
            self.hess = fd_hess
        elif isinstance(self._hess, SparseFD):
            term, raw_jac = self.fd_hessian, memo.fun

            def sparse_fd_hess(x, v):   # the same difference, grouped, as one CSR term
                return term.request(lambda y: raw_jac(y).T.dot(v),
                                    lambda: memo.lookup(x).T.dot(v))
            self.hess = sparse_fd_hess
        elif _qn.is_strategy(self._hess):
            n, sparse = x0.size, self.sparse_jacobian

            def qn_hess(x, v):          # the Jacobian in the form ``self.jac`` gives it
                J = memo.lookup(x)
                if sparse:
                    J = canonical_csr(J)
                else:
                    J = J.toarray() if sps.issparse(J) else np.atleast_2d(J)
                return _qn.QNRequest(n, J=J, v=v)
            self.hess = qn_hess
        else:
            self.hess = self._hess
        self._finish(x0, f0)
        if not is_feasible(self.kind, self.enforce_feasibility, f0):
            raise ValueError(_INFEASIBLE)
        self.isinitialized = True
        return x0


class LinearConstraint(_Initialised):
    """``lb <= A x <= ub`` (reference _constraints.py:170-270)."""

    def __init__(self, A, kind, enforce_feasibility=False):
        self.A = A
        self.kind = kind
        self.enforce_feasibility = enforce_feasibility

    def evaluate_and_initialize(self, x0, sparse_jacobian=None):
        self.sparse_jacobian = bool(sparse_jacobian
                                    or (sparse_jacobian is None and sps.issparse(self.A)))
        if self.sparse_jacobian:
            self.A = canonical_csr(self.A)
        else:
            self.A = self.A.toarray() if sps.issparse(self.A) else np.atleast_2d(self.A)
        x0 = np.atleast_1d(x0).astype(float)
        f0 = self.A.dot(x0)
        self.J0 = self.A
        self._finish(x0, f0)
        if not is_feasible(self.kind, self.enforce_feasibility, f0):
            raise ValueError(_INFEASIBLE)
        self.isinitialized = True
        return x0

    def to_nonlinear(self):
        if not self.isinitialized:
            raise RuntimeError("Trying to convert uninitialized constraint.")
        A = self.A
        nl = NonlinearConstraint(lambda x: A.dot(x), self.kind, lambda x: A, None,
                                 self.enforce_feasibility)
        nl.fun, nl.jac, nl.hess = nl._fun, nl._jac, None
        nl.isinitialized = True
        nl.constant_jac = True          # lets the solver keep one upload / factorization (N1)
        for name in ("m", "n", "sparse_jacobian", "x0", "f0", "J0"):
            setattr(nl, name, getattr(self, name))
        return nl


class BoxConstraint(_Initialised):
    """``lb <= x <= ub`` (reference _constraints.py:273-364)."""

    def __init__(self, kind, enforce_feasibility=False):
        self.kind = kind
        self.enforce_feasibility = enforce_feasibility

    def evaluate_and_initialize(self, x0, sparse_jacobian=None):
        x0 = np.atleast_1d(x0).astype(float)
        n = x0.size
        self.sparse_jacobian = bool(sparse_jacobian or sparse_jacobian is None)
        self.J0 = sps.eye(n).tocsr() if self.sparse_jacobian else np.eye(n)
        self._finish(x0, x0)
        self.isinitialized = True
        if not is_feasible(self.kind, self.enforce_feasibility, x0):
            warn("The initial point was changed in order to stay inside box constraints.")
            x0 = reinforce_box(self.kind, self.enforce_feasibility, x0)
            self.x0 = self.f0 = x0
        return x0

    def to_linear(self):
        if not self.isinitialized:
            raise RuntimeError("Trying to convert uninitialized constraint.")
        lin = LinearConstraint(self.J0, self.kind, self.enforce_feasibility)
        lin.isinitialized = True
        for name in ("m", "n", "sparse_jacobian", "x0", "f0", "J0"):
            setattr(lin, name, getattr(self, name))
        return lin

    def to_nonlinear(self):
        if not self.isinitialized:
            raise RuntimeError("Trying to convert uninitialized constraint.")
        return self.to_linear().to_nonlinear()
