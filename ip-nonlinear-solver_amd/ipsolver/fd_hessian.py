"""Sparse finite-difference Hessians assembled into CSR on the device.

A Hessian of known sparsity is the Jacobian of a gradient: ``hess=SparseFD(...)`` differences
``grad`` (the objective) or ``x -> J(x)' v`` (a constraint, ``v`` frozen) by Curtis-Powell-Reid
column groups of ``S | S'`` -- G gradient calls per outer iteration, none per CG iteration -- and
one launch of ``ipx_fd_assemble_sym`` writes ``0.5 (q_ij + q_ji)`` for every stored entry, an
exactly symmetric matrix.  The objective's and every constraint's term are added into ONE value
array on the union of their patterns (``LagrangianFDHessian``), which the solver's loops take as
the ``csr`` term of their Hessian operator, like an exact CSR Hessian on that pattern.

No bounds enter these differences (the reference's Hessian differences have none,
_numdiff.py:403-441).  Steps, perturbed points and the copies of callback results are the
kernels of csrc/fdjac.hip the Jacobian differences use.
"""
import numbers

import numpy as np
import scipy.sparse as sps

from . import _hip
from .fd import FD_METHODS
from .fd_jacobian import (SparseFDPlan, METHOD_CODE, F_BUDGET_BYTES, _host_ptr, _structure_csr,
                          host_callback)


def _pattern_arrays(p):
    """A ``device.CSRPattern``-like object as a scipy 0/1 matrix."""
    return sps.csr_matrix((np.ones(len(p.indices_h), dtype=np.int8), p.indices_h, p.indptr_h),
                          shape=p.shape)


class SparseFD:
    """``hess=SparseFD(method='2-point', sparsity=None, groups=None, rel_step=None)``: the
    Hessian by grouped differences of the gradient, assembled into a CSR matrix on the device.

    Accepted by ``minimize_constrained(..., hess=...)`` (differences of ``grad``) and by
    ``NonlinearConstraint(fun, kind, jac, hess=...)`` (differences of ``x -> J(x)' v``).  The
    object holds parameters only and is deliberately not callable.

    method : '2-point' | '3-point' | 'cs'
    sparsity : n x n structure (scipy sparse, a dense 0/1 array, a ``device.CSRPattern``); the
        plan uses ``S | S'``.  None: the full pattern, n gradient calls per Hessian (numpy
        callbacks only; a ``ValueError`` in device-callback mode).
    groups : (n,) group of every column, or None for ``_numdiff.group_columns(S | S')``
    rel_step : None (the method's default), a positive number, or one per variable
    """

    def __init__(self, method='2-point', sparsity=None, groups=None, rel_step=None):
        if not isinstance(method, str) or method not in FD_METHODS:
            raise ValueError("method must be one of %r, got %r" % (FD_METHODS, method))
        n = None
        if sparsity is not None:
            if hasattr(sparsity, "indptr_h") and hasattr(sparsity, "indices_h"):
                shape = tuple(sparsity.shape)
            elif sps.issparse(sparsity):
                shape = tuple(sparsity.shape)
            else:
                if isinstance(sparsity, (str, bytes)) or np.ndim(sparsity) != 2:
                    raise ValueError("sparsity must be an n x n structure (scipy sparse, a 2-D "
                                     "array or a CSRPattern), got %r" % (type(sparsity),))
                shape = np.shape(sparsity)
            if len(shape) != 2 or shape[0] != shape[1]:
                raise ValueError("sparsity must be square (n x n), got shape %r" % (shape,))
            n = int(shape[0])
        if groups is not None:
            g = np.asarray(groups)
            if isinstance(groups, (str, bytes)) or g.ndim != 1 \
                    or not np.issubdtype(g.dtype, np.integer) or (g.size and g.min() < 0):
                raise ValueError("groups must be a 1-D array of non-negative integers, got %r"
                                 % (groups,))
            if sparsity is None:
                raise ValueError("groups need a sparsity structure (without one every column is "
                                 "a group of its own)")
            if g.shape != (n,):
                raise ValueError("groups has shape %r, the sparsity structure %d columns"
                                 % (g.shape, n))
            groups = np.ascontiguousarray(g, dtype=np.int32)
        if rel_step is not None:
            r = np.asarray(rel_step)
            if isinstance(rel_step, (bool, str, bytes)) or r.ndim > 1 or r.dtype.kind not in "fiu" \
                    or not np.all(np.isfinite(r)) or not np.all(r > 0):
                raise ValueError("rel_step must be None, a positive finite number or one per "
                                 "variable, got %r" % (rel_step,))
            if r.ndim == 1 and n is not None and r.shape != (n,):
                raise ValueError("rel_step has shape %r, the sparsity structure %d columns"
                                 % (r.shape, n))
            rel_step = float(rel_step) if isinstance(rel_step, numbers.Real) else r.astype(float)
        self.method, self.sparsity, self.groups, self.rel_step = method, sparsity, groups, rel_step
        self._n = n

    def __repr__(self):
        sp = "None" if self.sparsity is None else "<%d x %d structure>" % (self._n, self._n)
        gr = "None" if self.groups is None else "<%d groups>" % (int(self.groups.max()) + 1
                                                                 if self.groups.size else 0)
        rs = self.rel_step if self.rel_step is None or np.ndim(self.rel_step) == 0 \
            else "<%d steps>" % len(self.rel_step)
        return "SparseFD(method=%r, sparsity=%s, groups=%s, rel_step=%s)" % (self.method, sp, gr, rs)


def is_sparse_fd(h):
    return isinstance(h, SparseFD)


class SparseFDHessianPlan(SparseFDPlan):
    """Symbolic half of one term: the symmetrised pattern ``S | S'`` (n x n), its groups and --
    on the device -- the planes of gradient values.  ``sparsity`` None: the full pattern with
    ``groups = arange(n)`` (as ``fd_jacobian.dense_plan``)."""

    def __init__(self, sparsity, groups, n, budget_bytes=F_BUDGET_BYTES):
        n = int(n)
        if sparsity is None:
            if n * n >= 2 ** 31:
                raise ValueError("SparseFD: a dense %d x %d finite-difference Hessian has 2**31 "
                                 "entries or more; pass a sparsity structure" % (n, n))
            S = sps.csr_matrix(np.ones((n, n), dtype=np.int8))
            groups = np.arange(n, dtype=np.int32) if groups is None else groups
        else:
            if hasattr(sparsity, "indptr_h"):
                sparsity = _pattern_arrays(sparsity)
            indptr, indices = _structure_csr(sparsity, n, n)
            S = sps.csr_matrix((np.ones(len(indices), dtype=np.int8), indices, indptr),
                               shape=(n, n))
            S = sps.csr_matrix(S + S.T)
            if groups is None:
                from ._numdiff import group_columns
                groups = group_columns(S)
        SparseFDPlan.__init__(self, S, groups, n, n, budget_bytes)

    @property
    def tpos(self):
        """Position of entry (j, i) for every stored entry (i, j)."""
        tag = sps.csr_matrix((np.arange(1, self.nnz + 1, dtype=np.float64), self.indices,
                              self.indptr), shape=self.shape)
        t = sps.csr_matrix(tag.T)
        t.sort_indices()
        return (t.data - 1).astype(np.int64)

    # ---- device side ---------------------------------------------------------------------
    def assemble_sym(self, method, g_lo, g_hi, f0, F1, F2, dx, flags, val, slot=None,
                     accumulate=False):
        """One launch: the halves of groups [g_lo, g_hi) into ``val`` (at ``slot``)."""
        from .device import stream_ptr, _p
        pat = self.pattern
        if pat.nnz == 0:
            return
        _hip.call("ipx_fd_assemble_sym", self.n, _p(pat.indptr), _p(pat.indices), _p(pat.tiles),
                  pat.ntiles, METHOD_CODE[method], _p(self.groups_dev), int(g_lo), int(g_hi),
                  _p(f0), _p(F1), _p(F2), _p(dx), _p(flags), _p(slot), int(bool(accumulate)),
                  _p(val), stream_ptr())

    def evaluate_into(self, fun, x, method, val, f0=None, rel_step=None, slot=None,
                      accumulate=False):
        """The symmetrised difference of ``fun`` (CUDA tensor -> CUDA tensor / DVec) at ``x``
        into ``val`` (at ``slot``; added when ``accumulate``): G calls of ``fun`` (2 G for
        '3-point'), counted in ``nfev``; ``f0`` is ``fun(x)`` or a callable giving it ('cs'
        needs none).  A term whose planes exceed the budget is assembled chunk by chunk into a
        scratch array of its own and added to ``val`` by ONE scatter-add, so the result carries
        the single launch's bits."""
        import torch
        from .device import stream_ptr, _p
        if method not in FD_METHODS:
            raise ValueError("Unknown method '%s'. " % method)
        x = x.t if hasattr(x, "t") and not torch.is_tensor(x) else x
        x = x.to(torch.float64).reshape(-1).contiguous()
        if x.numel() != self.n:
            raise ValueError("finite-difference Hessian: x has %d entries, the sparsity "
                             "structure has %d columns" % (x.numel(), self.n))
        if method != 'cs':
            if callable(f0):
                f0 = f0()
            if f0 is None:
                f0 = fun(x)
                self.nfev += 1
            f0 = self._value(f0, "`f0`").to(torch.float64).contiguous()
        else:
            f0 = None
        h, flags = self.steps(x, method, None, rel_step)
        dx = torch.empty(self.n, dtype=torch.float64, device=x.device)
        F1, F2 = self._buffers(method)
        chunk = F1.shape[0] if self.n_groups else 1
        chunked = chunk < self.n_groups
        indirect = chunked and (slot is not None or accumulate)
        target = torch.empty(self.nnz, dtype=torch.float64, device=x.device) if indirect else val
        for g_lo in range(0, self.n_groups, chunk):
            g_hi = min(self.n_groups, g_lo + chunk)
            for g in range(g_lo, g_hi):
                x1, x2 = self.perturb(x, h, flags, g, method, dx)
                if method == 'cs':
                    f1 = fun(torch.complex(x, x1))
                    f1 = f1.t if hasattr(f1, "t") and not torch.is_tensor(f1) else f1
                    if not torch.is_tensor(f1) or not torch.is_complex(f1):
                        raise TypeError("SparseFD('cs'): the callback returned a real value for "
                                        "a complex argument (it must be analytic in complex "
                                        "arithmetic)")
                    F1[g - g_lo].copy_(self._value(f1.imag, "the callback's value"))
                    self.nfev += 1
                    continue
                F1[g - g_lo].copy_(self._value(fun(x1), "the callback's value"))
                self.nfev += 1
                if x2 is not None:
                    F2[g - g_lo].copy_(self._value(fun(x2), "the callback's value"))
                    self.nfev += 1
            if indirect:
                self.assemble_sym(method, g_lo, g_hi, f0, F1, F2, dx, flags, target)
            else:
                self.assemble_sym(method, g_lo, g_hi, f0, F1, F2, dx, flags, val, slot, accumulate)
        if indirect and self.nnz:
            if slot is None:
                val.add_(target) if accumulate else val.copy_(target)
            else:
                _hip.call("ipx_scatter_add", self.nnz, _p(target), _p(slot), _p(val), stream_ptr())

    def evaluate(self, fun, x, method, f0=None, rel_step=None):
        """This term alone as a ``DeviceCSR`` on ``self.pattern``."""
        import torch
        from .device import DeviceCSR, ctx
        val = torch.empty(self.nnz, dtype=torch.float64, device=ctx().device)
        self.evaluate_into(fun, x, method, val, f0=f0, rel_step=rel_step)
        return DeviceCSR(self.pattern, val)

    # ---- host twin (the library's host entry: CPU tests, no device) ------------------------
    def assemble_sym_host(self, method, f0, F1, F2, dx, one_sided, val=None, slot=None,
                          accumulate=False, chunk=None):
        """The symmetric assemble on host arrays (``F1`` / ``F2``: G x n) into ``val`` (a new
        array of the plan's nnz when None), ``chunk`` groups per call of the host entry."""
        c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, dtype=t)
        f0, F1, F2, dx = c(f0), c(F1), c(F2), c(dx)
        flags, slot = c(one_sided, np.uint8), c(slot, np.int32)
        if val is None:
            val = np.zeros(self.nnz if slot is None else int(slot.max()) + 1)
        chunk = self.n_groups if chunk is None else max(1, int(chunk))
        lib = _hip.load()
        for g_lo in range(0, self.n_groups, chunk):
            g_hi = min(self.n_groups, g_lo + chunk)
            lib.ipx_fd_assemble_sym_host(
                self.n, _host_ptr(self.indptr), _host_ptr(self.indices), METHOD_CODE[method],
                _host_ptr(self.groups), g_lo, g_hi, _host_ptr(f0),
                _host_ptr(None if F1 is None else F1[g_lo:g_hi]),
                _host_ptr(None if F2 is None else F2[g_lo:g_hi]), _host_ptr(dx), _host_ptr(flags),
                _host_ptr(slot), int(bool(accumulate)), _host_ptr(val))
        return val


class Memo:
    """A numpy callback with its last point and value kept (compared by value): the Jacobian
    the solver evaluated at the Hessian's point is the ``f0`` of the difference there."""

    def __init__(self, fun, x0=None, f0=None, reuse=False):
        self.fun = fun
        self._x = None if x0 is None else np.array(x0, copy=True)
        self._f = f0
        self.misses = 0
        # reuse: a call at the kept point returns the kept value too (the barrier method
        # evaluates the Jacobian again where a subproblem ends, at the point it last evaluated)
        self.reuse = bool(reuse)

    def __call__(self, x):
        if self.reuse and self._x is not None and np.array_equal(x, self._x):
            return self._f
        f = self.fun(x)
        self._x, self._f = np.array(x, copy=True), f
        return f

    def lookup(self, x):
        if self._x is not None and np.array_equal(x, self._x):
            return self._f
        self.misses += 1
        return self(x)


class DeviceMemo:
    """Device-callback mode: a Jacobian callback with copies of its last few points and values
    (``quasi_newton.DeviceGradientMemo`` for matrices; a lookup compares the point by value)."""

    KEEP = 2

    def __init__(self, jac, check, reuse=False):
        self.jac, self.check = jac, check
        self._seen = []
        self.misses = 0
        self.reuse = bool(reuse)        # a call at the newest kept point returns its copy (Memo)

    def __call__(self, xt):
        import torch
        from .device import DeviceCSR
        if self.reuse and self._seen and xt.shape == self._seen[0][0].shape \
                and bool(torch.equal(xt, self._seen[0][0])):
            return self._seen[0][1]
        J = self.check(self.jac(xt))
        kept = DeviceCSR(J.pattern, J.val.detach().clone()) if isinstance(J, DeviceCSR) \
            else type(J)(J.t.detach().clone())
        self._seen = [(xt.detach().clone(), kept)] + self._seen[:self.KEEP - 1]
        return J

    def lookup(self, xt):
        import torch
        for x, J in self._seen:
            if xt.shape == x.shape and bool(torch.equal(xt, x)):
                return J
        self.misses += 1
        self(xt)
        return self._seen[0][1]


class FDTerm:
    """One term of the Lagrangian Hessian that is differenced: its plan, method and step, and
    ``calls`` -- the callback evaluations spent on its differences."""

    def __init__(self, spec, n, what, device_mode=False):
        if device_mode and spec.sparsity is None:
            raise ValueError(
                "device-callback mode: hess=%r needs `sparsity` (an n x n structure): a dense "
                "difference of a device gradient costs n = %d gradient calls per Hessian and is "
                "refused; pass SparseFD(sparsity=...) or use the operator form hess=%r"
                % (spec, n, spec.method))
        if spec._n is not None and spec._n != n:
            raise ValueError("SparseFD: the sparsity structure is %d x %d, the problem has %d "
                             "variables" % (spec._n, spec._n, n))
        self.spec, self.what = spec, what
        self.method, self.rel_step = spec.method, spec.rel_step
        self.plan = SparseFDHessianPlan(spec.sparsity, spec.groups, n)

    @property
    def calls(self):
        return self.plan.nfev

    def request(self, fun, f0):
        return FDRequest(self, fun, f0)


class FDRequest:
    """What a ``SparseFD`` Hessian callback returns: the term, the function to difference at
    this point (``v`` frozen inside it) and a callable giving its memoised value there.  The
    Lagrangian's requests are resolved together into ONE ``DeviceCSR``
    (``LagrangianFDHessian.evaluate``)."""

    def __init__(self, term, fun, f0):
        self.term, self.fun, self.f0 = term, fun, f0
        n = term.plan.n
        self.shape = (n, n)

    def dot(self, p):
        raise _hip.IpxError("a SparseFD Hessian term is assembled on the device "
                            "(LagrangianFDHessian); it has no product of its own")


class LagrangianFDHessian:
    """Every differenced term of the Lagrangian Hessian in ONE value array: the union pattern
    (ONE ``CSRPattern`` object for the solve's life: the factorization pools and the chain
    stages key on identity) and each term's slot table are built at the first evaluation, on
    the host.  ``host_callbacks``: the terms' functions take and return numpy arrays (points go
    down for the call and values come back)."""

    def __init__(self, host_callbacks=False):
        self.host_callbacks = bool(host_callbacks)
        self.terms = None
        self._pattern = None
        self.evaluations = 0

    def _plan(self, terms):
        self.terms = list(terms)
        plans = [t.plan for t in self.terms]
        self.n = plans[0].n
        if len(plans) == 1:
            self.indptr, self.indices = plans[0].indptr, plans[0].indices
            self.slots_h = [None]
            return
        keys = []
        for p in plans:
            rows = np.repeat(np.arange(p.n, dtype=np.int64), np.diff(p.indptr))
            keys.append(rows * self.n + p.indices.astype(np.int64))
        union = np.unique(np.concatenate(keys))
        counts = np.bincount((union // self.n).astype(np.int64), minlength=self.n)
        self.indptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        self.indices = (union % self.n).astype(np.int32)
        self.slots_h = [np.searchsorted(union, k).astype(np.int32) for k in keys]

    @property
    def pattern(self):
        if self._pattern is None:
            import torch
            from .device import CSRPattern, ctx
            if len(self.terms) == 1:
                self._pattern = self.terms[0].plan.pattern
                self._slots = [None]
            else:
                self._pattern = CSRPattern(self.indptr, self.indices, (self.n, self.n))
                self._slots = [torch.from_numpy(s).to(ctx().device) for s in self.slots_h]
        return self._pattern

    def evaluate(self, x, requests):
        """``requests`` (``FDRequest``, in hess_list order) at ``x`` (CUDA tensor, DVec or -- host
        callbacks -- a numpy array) -> one ``DeviceCSR`` on ``self.pattern``.  The terms are
        launched one after the other on the solve's stream; the array is zeroed before the
        first of several."""
        import torch
        from .device import DeviceCSR, ctx
        terms = [r.term for r in requests]
        if self.terms is None:
            self._plan(terms)
        elif len(terms) != len(self.terms) or any(a is not b for a, b in zip(terms, self.terms)):
            raise _hip.IpxError("SparseFD: the differenced Hessian terms changed during a solve")
        pat = self.pattern
        dev = ctx().device
        if self.host_callbacks:
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        single = len(requests) == 1
        val = (torch.empty if single else torch.zeros)(pat.nnz, dtype=torch.float64, device=dev)
        for r, slot in zip(requests, self._slots):
            fun, f0 = r.fun, r.f0
            if self.host_callbacks:
                fun = host_callback(fun, dev)
                if r.term.method != 'cs':
                    f0 = torch.from_numpy(np.ascontiguousarray(
                        np.atleast_1d(r.f0()), dtype=np.float64)).to(dev)
            r.term.plan.evaluate_into(fun, x, r.term.method, val, f0=f0,
                                      rel_step=r.term.rel_step, slot=slot, accumulate=not single)
        self.evaluations += 1
        return DeviceCSR(pat, val)

    def resolve(self, terms, x):
        """A list of Hessian terms with its ``FDRequest``s replaced by their one ``DeviceCSR``,
        put first (the Hessian operator's ``csr`` term); the other terms keep their order."""
        requests = [t for t in terms if isinstance(t, FDRequest)]
        if not requests:
            return list(terms)
        return [self.evaluate(x, requests)] + [t for t in terms if not isinstance(t, FDRequest)]


def report_calls(result, objective_term, holders):
    """``hess_fd_ngev`` / ``hess_fd_njev``: gradient / Jacobian calls spent on Hessian
    differences (``ngev`` / ``njev`` keep the reference's meaning); present when some Hessian
    term is a ``SparseFD``."""
    cons = [h.fd_hessian for h in holders if getattr(h, "fd_hessian", None) is not None]
    if objective_term is None and not cons:
        return
    result.hess_fd_ngev = int(objective_term.calls) if objective_term is not None else 0
    result.hess_fd_njev = int(sum(t.calls for t in cons))
