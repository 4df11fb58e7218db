"""Sparse finite-difference constraint Jacobians on the device.

A Jacobian of known sparsity is a fixed ``CSRPattern`` whose refresh moves values only, and a
Curtis-Powell-Reid grouped difference (reference _numdiff.py:484-561) writes exactly those
values: columns that share no row are perturbed together, ``G`` groups cost ``G`` calls of the
user's ``fun`` (``2 G`` for '3-point') plus three kinds of HBM-bound kernels (csrc/fdjac.hip:
steps, one perturbed point per group, ONE assemble in CSR order), and nothing crosses PCIe.

``SparseFDPlan`` does the symbolic work once -- the sorted pattern, the group table, the check
that a one-pass assemble is possible -- and ``evaluate`` is the value refresh.  Every value is
the reference's ``df[i] / dx[j]`` bit for bit, given the same function values.

One deviation from the reference: two columns of ONE group that share a row are refused
(``ValueError`` naming the row and the columns).  The reference sums the two quotients into one
entry -- a number that is no derivative of anything; a one-pass assemble in CSR order writes each
entry once and cannot.  ``group_columns`` never produces such a grouping.
"""
import ctypes

import numpy as np
import scipy.sparse as sps

from . import _hip
from .fd import FD_METHODS, _REL_STEP

METHOD_CODE = {'2-point': 0, '3-point': 1, 'cs': 2}
F_BUDGET_BYTES = 256 << 20       # the planes of function values; above it: chunks of groups


def _host_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def steps_host(x0, method, rel_step=None, lb=None, ub=None):
    """(h, one_sided) of ``_compute_absolute_step`` + ``_adjust_scheme_to_bounds`` by the
    library's host entry (the kernel's arithmetic on host arrays)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    n = x0.size
    rel, rel_vec = _rel_step(rel_step, method, n)
    lb = None if lb is None else np.ascontiguousarray(lb, dtype=np.float64)
    ub = None if ub is None else np.ascontiguousarray(ub, dtype=np.float64)
    h, flags = np.empty(n), np.empty(n, dtype=np.uint8)
    _hip.load().ipx_fd_steps_host(n, METHOD_CODE[method], rel, _host_ptr(rel_vec), _host_ptr(x0),
                                  _host_ptr(lb), _host_ptr(ub), _host_ptr(h), _host_ptr(flags))
    return h, flags.astype(bool)


def perturb_host(x0, h, one_sided, groups, g, method, dx):
    """(x1, x2) of group ``g`` by the library's host entry; ``dx`` (n,) gets its members'."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64)
    flags = np.ascontiguousarray(one_sided, dtype=np.uint8)
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    x1, x2 = np.empty_like(x0), np.empty_like(x0)
    _hip.load().ipx_fd_perturb_host(x0.size, METHOD_CODE[method], int(g), _host_ptr(groups),
                                    _host_ptr(x0), _host_ptr(h), _host_ptr(flags), _host_ptr(x1),
                                    _host_ptr(x2), _host_ptr(dx))
    return x1, (x2 if method == '3-point' else None)


def _rel_step(rel_step, method, n):
    """(scalar, per-variable array or None) of the ``rel_step`` argument."""
    if rel_step is None:
        return float(_REL_STEP[method]), None
    if np.ndim(rel_step) == 0:
        return float(rel_step), None
    vec = np.array(np.broadcast_to(np.asarray(rel_step, dtype=np.float64), (n,)))
    return 0.0, vec


def _structure_csr(structure, m, n):
    """The nonzero pattern of ``structure`` as CSR arrays with sorted indices (zero entries of
    the structure -- stored or not -- are no entries, as for the reference's ``find``)."""
    if sps.issparse(structure):
        S = sps.csr_matrix(structure).copy()
        S.sum_duplicates()
        S.data = (S.data != 0).astype(np.int8)
    else:
        S = sps.csr_matrix((np.atleast_2d(np.asarray(structure)) != 0).astype(np.int8))
    if S.shape != (m, n):
        raise ValueError("the sparsity structure has shape %r, the Jacobian %r"
                         % (tuple(S.shape), (m, n)))
    S.eliminate_zeros()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32)


class SparseFDPlan:
    """Symbolic half of a sparse finite-difference Jacobian: ``structure`` (m x n, array or
    sparse) and ``groups`` (n,) as from ``_numdiff.group_columns``.  ``pattern`` is ONE
    ``CSRPattern`` object for the plan's life (stacking, the factorization pools and the chain
    stages key on pattern identity); ``evaluate`` returns a ``DeviceCSR`` on it."""

    dense = False          # (True for ``dense_plan``: the caller densifies the result)

    def __init__(self, structure, groups, n, m, budget_bytes=F_BUDGET_BYTES):
        self.n, self.m = int(n), int(m)
        self.shape = (self.m, self.n)
        self.indptr, self.indices = _structure_csr(structure, self.m, self.n)
        groups = np.atleast_1d(np.asarray(groups))
        if groups.shape != (self.n,):
            raise ValueError("`groups` has shape %r, expected (%d,)" % (groups.shape, self.n))
        if self.n and (groups.min() < 0 or not np.issubdtype(groups.dtype, np.integer)):
            raise ValueError("`groups` must hold non-negative integers")
        self.groups = np.ascontiguousarray(groups, dtype=np.int32)
        self.n_groups = int(self.groups.max()) + 1 if self.n else 0
        self.nnz = int(self.indptr[-1])
        self._check_grouping()
        self.budget_bytes = int(budget_bytes)
        self.nfev = 0                  # calls of ``fun`` made by ``evaluate`` (f0 included)
        self._pattern = None
        self._groups_dev = None
        self._planes = {}

    def _check_grouping(self):
        rows = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.indptr))
        key = rows * max(self.n_groups, 1) + self.groups[self.indices]
        check = np.sort(key)
        if not np.any(check[1:] == check[:-1]):
            return
        order = np.argsort(key, kind="stable")
        rep = np.flatnonzero(np.diff(key[order]) == 0)
        if len(rep):
            a, b = order[rep[0]], order[rep[0] + 1]
            raise ValueError(
                "SparseFDPlan: columns %d and %d are both in group %d and both have an entry in "
                "row %d; columns of one group must not share a row (use group_columns)"
                % (self.indices[a], self.indices[b], self.groups[self.indices[a]], rows[a]))

    # ---- device side ---------------------------------------------------------------------
    @property
    def pattern(self):
        if self._pattern is None:
            from .device import CSRPattern
            self._pattern = CSRPattern(self.indptr, self.indices, self.shape)
        return self._pattern

    @property
    def groups_dev(self):
        if self._groups_dev is None:
            import torch
            from .device import ctx
            self._groups_dev = torch.from_numpy(self.groups).to(ctx().device)
        return self._groups_dev

    def chunk_groups(self, method):
        """Groups per assemble launch: all of them while their planes fit the budget."""
        per_group = 8 * max(self.m, 1) * (2 if method == '3-point' else 1)
        return max(1, min(self.n_groups, self.budget_bytes // per_group))

    def _buffers(self, method):
        import torch
        from .device import ctx
        key = method == '3-point'
        hit = self._planes.get(key)
        if hit is None:
            rows = self.chunk_groups(method)
            dev = ctx().device
            F1 = torch.empty((rows, self.m), dtype=torch.float64, device=dev)
            F2 = torch.empty((rows, self.m), dtype=torch.float64, device=dev) if key else None
            hit = self._planes[key] = (F1, F2)
        return hit

    def _bound(self, b, x):
        """A bound as a device tensor, or None for none (an infinite scalar)."""
        import torch
        if b is None:
            return None
        if torch.is_tensor(b):
            b = b.to(device=x.device, dtype=torch.float64)
            return (b.expand(self.n) if b.dim() == 0 else b.reshape(-1)).contiguous()
        b = np.asarray(b, dtype=np.float64)
        if b.ndim == 0:
            if np.isinf(b):
                return None
            return torch.full((self.n,), float(b), dtype=torch.float64, device=x.device)
        return torch.from_numpy(np.ascontiguousarray(b.reshape(-1))).to(x.device)

    def steps(self, x, method, bounds=None, rel_step=None):
        """(h, one_sided) on the device: one launch."""
        import torch
        from .device import stream_ptr, _p
        lb, ub = (None, None) if bounds is None else (self._bound(bounds[0], x),
                                                      self._bound(bounds[1], x))
        for b in (lb, ub):
            if b is not None and b.numel() != self.n:
                raise ValueError("Inconsistent shapes between bounds and `x0`.")
        rel, rel_vec = _rel_step(rel_step, method, self.n)
        rel_dev = None if rel_vec is None else torch.from_numpy(rel_vec).to(x.device)
        h = torch.empty(self.n, dtype=torch.float64, device=x.device)
        flags = torch.empty(self.n, dtype=torch.uint8, device=x.device)
        _hip.call("ipx_fd_steps", self.n, METHOD_CODE[method], rel, _p(rel_dev), _p(x), _p(lb),
                  _p(ub), _p(h), _p(flags), stream_ptr())
        return h, flags

    def perturb(self, x, h, flags, g, method, dx):
        """The perturbed point(s) of group ``g`` in NEW tensors (a callback may remember its
        argument by storage); ``dx`` gets the members' entries."""
        import torch
        from .device import stream_ptr, _p
        x1 = torch.empty_like(x)
        x2 = torch.empty_like(x) if method == '3-point' else None
        _hip.call("ipx_fd_perturb", self.n, METHOD_CODE[method], int(g), _p(self.groups_dev),
                  _p(x), _p(h), _p(flags), _p(x1), _p(x2), _p(dx), stream_ptr())
        return x1, x2

    def assemble(self, method, g_lo, g_hi, f0, F1, F2, dx, flags, val):
        """One launch: the entries of groups [g_lo, g_hi) into ``val``."""
        from .device import stream_ptr, _p
        pat = self.pattern
        if pat.nnz == 0:
            return
        _hip.call("ipx_fd_assemble", self.m, self.n, _p(pat.indptr), _p(pat.indices),
                  _p(pat.tiles), pat.ntiles, METHOD_CODE[method], _p(self.groups_dev), int(g_lo),
                  int(g_hi), _p(f0), _p(F1), _p(F2), _p(dx), _p(flags), _p(val), stream_ptr())

    def _value(self, f, what):
        """A callback's return value as a 1-D device tensor of m entries."""
        import torch
        t = f.t if hasattr(f, "t") and not torch.is_tensor(f) else f
        if not torch.is_tensor(t):
            raise TypeError("finite-difference Jacobian: `fun` must return a CUDA tensor, got %r"
                            % type(f))
        if t.dim() == 0:
            t = t.reshape(1)
        if t.dim() > 1:
            raise RuntimeError("`fun` return value has more than 1 dimension.")
        if t.numel() != self.m:
            raise ValueError("finite-difference Jacobian: %s has %d entries, the sparsity "
                             "structure has %d rows" % (what, t.numel(), self.m))
        return t

    def evaluate(self, fun, x, method, f0=None, bounds=None, rel_step=None):
        """The Jacobian of ``fun`` (CUDA tensor -> CUDA tensor / DVec) at ``x`` (CUDA tensor or
        DVec) as a ``DeviceCSR`` on ``self.pattern``: one call of ``fun`` for ``f0`` unless it is
        given, then G calls (2 G for '3-point'), each result copied device-to-device into its
        plane; nothing is read back."""
        import torch
        from .device import DeviceCSR
        if method not in FD_METHODS:
            raise ValueError("Unknown method '%s'. " % method)
        x = x.t if hasattr(x, "t") and not torch.is_tensor(x) else x
        x = x.to(torch.float64).reshape(-1).contiguous()
        if x.numel() != self.n:
            raise ValueError("finite-difference Jacobian: x has %d entries, the sparsity "
                             "structure has %d columns" % (x.numel(), self.n))
        if method != 'cs':
            if f0 is None:
                f0 = fun(x)
                self.nfev += 1
            f0 = self._value(f0, "`f0`").to(torch.float64).contiguous()
        else:
            f0 = None
        h, flags = self.steps(x, method, bounds, rel_step)
        dx = torch.empty(self.n, dtype=torch.float64, device=x.device)
        val = torch.empty(self.nnz, dtype=torch.float64, device=x.device)
        F1, F2 = self._buffers(method)
        chunk = F1.shape[0] if self.n_groups else 1
        for g_lo in range(0, self.n_groups, chunk):
            g_hi = min(self.n_groups, g_lo + chunk)
            for g in range(g_lo, g_hi):
                x1, x2 = self.perturb(x, h, flags, g, method, dx)
                if method == 'cs':
                    f1 = fun(torch.complex(x, x1))
                    f1 = f1.t if hasattr(f1, "t") and not torch.is_tensor(f1) else f1
                    if not torch.is_tensor(f1) or not torch.is_complex(f1):
                        raise TypeError("jac='cs': `fun` returned a real value for a complex "
                                        "argument (it must be analytic in complex arithmetic)")
                    F1[g - g_lo].copy_(self._value(f1.imag, "`fun`'s value"))
                    self.nfev += 1
                    continue
                F1[g - g_lo].copy_(self._value(fun(x1), "`fun`'s value"))
                self.nfev += 1
                if x2 is not None:
                    F2[g - g_lo].copy_(self._value(fun(x2), "`fun`'s value"))
                    self.nfev += 1
            self.assemble(method, g_lo, g_hi, f0, F1, F2, dx, flags, val)
        return DeviceCSR(self.pattern, val)

    # ---- host twin (the library's host entries: CPU tests, no device) ----------------------
    def assemble_host(self, method, f0, F1, F2, dx, one_sided):
        """The assemble stage on host arrays (``F1`` / ``F2``: G x m) as a scipy ``csr_matrix``
        with the plan's pattern, explicit zeros kept."""
        val = np.zeros(self.nnz)
        c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, dtype=t)
        f0, F1, F2, dx = c(f0), c(F1), c(F2), c(dx)
        flags = c(one_sided, np.uint8)
        _hip.load().ipx_fd_assemble_host(self.m, self.n, _host_ptr(self.indptr),
                                         _host_ptr(self.indices), METHOD_CODE[method],
                                         _host_ptr(self.groups), 0, self.n_groups, _host_ptr(f0),
                                         _host_ptr(F1), _host_ptr(F2), _host_ptr(dx),
                                         _host_ptr(flags), _host_ptr(val))
        return sps.csr_matrix((val, self.indices.copy(), self.indptr.copy()), shape=self.shape)

    def to_scipy(self, J):
        """A ``DeviceCSR`` of this plan as a scipy ``csr_matrix`` (one copy to the host)."""
        return sps.csr_matrix((J.val.cpu().numpy(), self.indices.copy(), self.indptr.copy()),
                              shape=self.shape)


def dense_plan(n, m, budget_bytes=F_BUDGET_BYTES):
    """The plan of a dense difference: the full pattern, every column a group of its own."""
    if m * n >= 2 ** 31:
        raise ValueError("approx_derivative: a dense %d x %d finite-difference Jacobian has "
                         "2**31 entries or more; pass a sparsity structure" % (m, n))
    plan = SparseFDPlan.__new__(SparseFDPlan)
    plan.n, plan.m, plan.shape = int(n), int(m), (int(m), int(n))
    plan.indptr = (np.arange(m + 1, dtype=np.int64) * n).astype(np.int32)
    plan.indices = np.tile(np.arange(n, dtype=np.int32), m)
    plan.groups = np.arange(n, dtype=np.int32)
    plan.n_groups, plan.nnz = int(n), int(m * n)
    plan.budget_bytes, plan.nfev = int(budget_bytes), 0
    plan._pattern = plan._groups_dev = None
    plan._planes = {}
    plan.dense = True
    return plan


def densify(plan, J):
    """``DeviceCSR`` on the full pattern -> ``DeviceDense``: the values in CSR order ARE the
    row-major matrix (a view, no launch; adding the entries into a zeroed buffer with
    ``ipx_csr_rows_to_dense`` would turn a quotient of -0.0 into +0.0, which the reference
    keeps)."""
    from .dense import DeviceDense
    return DeviceDense(J.val.view(plan.m, plan.n))


def host_callback(fun, device):
    """A numpy ``fun`` as a device callback: the point goes down to the host for the call and
    the values come back up (documented round trip; the operator mode works the same way)."""
    import torch

    def wrapped(xt):
        f = np.atleast_1d(fun(xt.cpu().numpy()))
        if f.ndim > 1:
            raise RuntimeError("`fun` return value has more than 1 dimension.")
        if not np.iscomplexobj(f):
            f = np.asarray(f, dtype=np.float64)
        return torch.from_numpy(np.ascontiguousarray(f)).to(device)
    return wrapped
