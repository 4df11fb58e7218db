"""``ipsolver._numdiff`` of the reference: ``approx_derivative`` in all three of its modes,
``group_columns`` and ``check_derivative``.

* ``as_linear_operator=True`` (reference _numdiff.py:342-441; ``hess='2-point'|'3-point'|'cs'``):
  ``fd.FiniteDifferenceOperator``, host callbacks.
* sparse and dense matrices (reference :371-400, :444-561; ``jac='2-point'|'3-point'|'cs'``): the
  grouped differences of ``fd_jacobian.SparseFDPlan`` on the device.  With a CUDA tensor ``x0``
  and a ``fun`` over CUDA tensors the result is a ``DeviceCSR`` (``DeviceDense`` for
  ``sparsity=None``) and nothing crosses PCIe.  With a numpy ``x0`` and a numpy ``fun`` the same
  kernels run: every perturbed point goes down to the host for the call and the values come
  back up (a documented round trip, as in operator mode), and the result is a scipy
  ``csr_matrix`` with the structure's pattern, or an ndarray for ``sparsity=None``.  The dense
  difference is the sparse one on the full pattern with every column a group of its own (its
  values in CSR order are the row-major matrix).

Differences from the reference, both on purpose: a grouping in which two columns of one group
share a row is refused instead of summed (``fd_jacobian``), and ``check_derivative`` returns 0.0
for a sparse Jacobian that matches exactly (the reference takes the maximum of an empty array).
"""
import numpy as np
import scipy.sparse as sps

from . import _hip
from .fd import FiniteDifferenceOperator, FD_METHODS

__all__ = ['approx_derivative', 'group_columns', 'check_derivative']


def group_columns(A, order=0):
    """Groups of columns of ``A`` (array or sparse, m x n) such that no two columns of a group
    have a nonzero in the same row (Curtis, Powell & Reid 1974), found greedily along a
    permutation of the columns: ``order`` is that permutation, or an int / None seeding a random
    one (default 0: random but repeatable).  Returns ``groups`` (n,), values 0 .. n_groups - 1.
    Same contract as the reference's ``group_columns`` (_numdiff.py:117-175)."""
    from scipy.optimize._group_columns import group_dense, group_sparse
    sparse = sps.issparse(A)
    if sparse:
        A = sps.csc_matrix(A)
    else:
        A = np.atleast_2d(A)
        if A.ndim != 2:
            raise ValueError("`A` must be 2-dimensional.")
        A = (A != 0).astype(np.int32)
    m, n = A.shape
    if order is None or np.isscalar(order):
        perm = np.random.RandomState(order).permutation(n)
    else:
        perm = np.asarray(order)
        if perm.shape != (n,):
            raise ValueError("`order` has incorrect shape.")
    permuted = A[:, perm]
    found = (group_sparse(m, n, permuted.indices, permuted.indptr) if sparse
             else group_dense(m, n, permuted))
    groups = np.empty_like(found)
    groups[perm] = found
    return groups


class DeviceNotAvailable(_hip.IpxError, NotImplementedError):
    """The matrix modes were asked for without a HIP device: they are implemented on the device
    only (there is no host implementation to fall back to)."""


def _is_cuda_tensor(x):
    try:
        import torch
    except ImportError:
        return False
    return torch.is_tensor(x) and x.is_cuda


def _plan_for(sparsity, n, m):
    """(plan, dense) of the ``sparsity`` argument: None (dense), a structure, (structure,
    groups), or a ready ``SparseFDPlan`` (what the constraint classes pass: symbolic work once)."""
    from .fd_jacobian import SparseFDPlan, dense_plan
    if sparsity is None:
        return dense_plan(n, m), True
    if isinstance(sparsity, SparseFDPlan):
        if sparsity.shape != (m, n):
            raise ValueError("the sparsity structure has shape %r, the Jacobian %r"
                             % (sparsity.shape, (m, n)))
        return sparsity, sparsity.dense
    if not sps.issparse(sparsity) and len(sparsity) == 2:
        structure, groups = sparsity
    else:
        structure, groups = sparsity, group_columns(sparsity)
    return SparseFDPlan(structure, np.atleast_1d(groups), n, m), False


def _approx_device(fun, x0, method, rel_step, f0, bounds, sparsity):
    """Matrix modes with a CUDA tensor ``x0`` and a device ``fun``."""
    import torch
    from .fd_jacobian import densify
    if x0.dim() > 1:
        raise ValueError("`x0` must have at most 1 dimension.")
    x0 = x0.detach().to(torch.float64).reshape(-1).contiguous()
    n = x0.numel()
    lb, ub = bounds
    shape = lambda b: tuple(b.shape) if torch.is_tensor(b) else np.shape(b)
    for b in (lb, ub):
        if shape(b) not in ((), (n,)):
            raise ValueError("Inconsistent shapes between bounds and `x0`.")

    def value(f):
        f = f.t if hasattr(f, "t") and not torch.is_tensor(f) else f
        return f.reshape(1) if torch.is_tensor(f) and f.dim() == 0 else f
    calls = 0
    if f0 is None:
        f0 = value(fun(x0))
        calls = 1
        if f0.dim() > 1:
            raise RuntimeError("`fun` return value has more than 1 dimension.")
    else:
        f0 = value(f0 if torch.is_tensor(f0) or hasattr(f0, "t")
                   else torch.as_tensor(np.atleast_1d(f0), device=x0.device))
        if f0.dim() > 1:
            raise ValueError("`f0` passed has more than 1 dimension.")
    plan, dense = _plan_for(sparsity, n, f0.numel())
    finite = [torch.is_tensor(b) or np.ndim(b) != 0 or not np.isinf(b) for b in (lb, ub)]
    if any(finite):             # (the one blocking read of this mode; none without bounds)
        lo, hi = plan._bound(lb, x0), plan._bound(ub, x0)
        bad = torch.zeros((), dtype=torch.bool, device=x0.device)
        if lo is not None:
            bad = bad | (x0 < lo).any()
        if hi is not None:
            bad = bad | (x0 > hi).any()
        if bool(bad):
            raise ValueError("`x0` violates bound constraints.")
    J = plan.evaluate(fun, x0, method, f0=f0, bounds=(lb, ub), rel_step=rel_step)
    plan.nfev += calls
    return densify(plan, J) if dense else J


def _approx_host(fun, x0, method, rel_step, f0, bounds, sparsity):
    """Matrix modes with numpy ``x0`` / ``fun``: the same kernels around host callbacks."""
    x0 = np.atleast_1d(x0)
    if x0.ndim > 1:
        raise ValueError("`x0` must have at most 1 dimension.")
    lb, ub = [np.asarray(b, dtype=float) for b in bounds]
    lb = np.resize(lb, x0.shape) if lb.ndim == 0 else lb
    ub = np.resize(ub, x0.shape) if ub.ndim == 0 else ub
    if lb.shape != x0.shape or ub.shape != x0.shape:
        raise ValueError("Inconsistent shapes between bounds and `x0`.")

    def fun_wrapped(x):
        f = np.atleast_1d(fun(x))
        if f.ndim > 1:
            raise RuntimeError("`fun` return value has more than 1 dimension.")
        return f
    calls = 0
    if f0 is None:
        f0 = fun_wrapped(x0)
        calls = 1
    else:
        f0 = np.atleast_1d(f0)
        if f0.ndim > 1:
            raise ValueError("`f0` passed has more than 1 dimension.")
    if np.any((x0 < lb) | (x0 > ub)):
        raise ValueError("`x0` violates bound constraints.")
    n, m = x0.size, f0.size
    plan, dense = _plan_for(sparsity, n, m)
    import torch
    if not torch.cuda.is_available():
        raise DeviceNotAvailable(
            "approx_derivative: dense / sparse finite-difference Jacobians are implemented on "
            "the device only and no HIP device is visible (the ipsolver product path is "
            "GPU-only: there is no CPU fallback); as_linear_operator=True runs on the host")
    from .device import ctx
    from .fd_jacobian import host_callback
    dev = ctx().device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    unbounded = np.all(np.isinf(lb)) and np.all(np.isinf(ub))
    J = plan.evaluate(host_callback(fun_wrapped, dev), up(x0), method, f0=up(f0),
                      bounds=None if unbounded else (up(lb), up(ub)), rel_step=rel_step)
    plan.nfev += calls
    if not dense:
        return plan.to_scipy(J)
    from .fd_jacobian import densify
    J = densify(plan, J).to_host()
    return J.ravel() if m == 1 else J


def approx_derivative(fun, x0, method='3-point', rel_step=None, f0=None,
                      bounds=(-np.inf, np.inf), sparsity=None, as_linear_operator=False,
                      args=(), kwargs={}):
    """Finite-difference approximation of the derivatives of a vector-valued function: the
    reference's ``approx_derivative`` (_numdiff.py:178-400; see the module docstring for the
    modes and what each returns)."""
    if method not in FD_METHODS:
        raise ValueError("Unknown method '%s'. " % method)
    f = (lambda x: fun(x, *args, **kwargs)) if (args or kwargs) else fun
    if not as_linear_operator:
        if _is_cuda_tensor(x0):
            return _approx_device(f, x0, method, rel_step, f0, bounds, sparsity)
        return _approx_host(f, x0, method, rel_step, f0, bounds, sparsity)
    x0 = np.atleast_1d(x0)
    if x0.ndim > 1:
        raise ValueError("`x0` must have at most 1 dimension.")
    lb, ub = (np.resize(np.asarray(b, dtype=float), x0.shape) for b in bounds)
    if not (np.all(np.isinf(lb)) and np.all(np.isinf(ub))):
        raise ValueError("Bounds not supported when `as_linear_operator` is True.")
    if f0 is not None and np.atleast_1d(f0).ndim > 1:
        raise ValueError("`f0` passed has more than 1 dimension.")
    op = FiniteDifferenceOperator(f, x0, method, rel_step, f0)
    if op.f0.ndim > 1:
        raise RuntimeError("`fun` return value has more than 1 dimension.")
    return op


def check_derivative(fun, jac, x0, bounds=(-np.inf, np.inf), args=(), kwargs={}):
    """Largest error of ``jac(x0)`` against a '3-point' finite-difference approximation of
    ``fun``: relative where the approximation exceeds 1 in magnitude, absolute elsewhere
    (reference _numdiff.py:564-639).  A sparse ``jac(x0)`` (scipy sparse, or a ``DeviceCSR``
    with a CUDA ``x0``) is differenced on its own sparsity structure."""
    J = jac(x0, *args, **kwargs)
    device_csr = hasattr(J, "to_scipy")
    if device_csr:
        J = J.to_scipy()
    elif hasattr(J, "to_host"):
        J = J.to_host()
    elif _is_cuda_tensor(J):
        J = J.cpu().numpy()
    if sps.issparse(J):
        J_diff = approx_derivative(fun, x0, bounds=bounds, sparsity=J, args=args, kwargs=kwargs)
        if hasattr(J_diff, "to_scipy"):
            J_diff = J_diff.to_scipy()
        err = sps.csr_matrix(J) - J_diff
        i, j, err_data = sps.find(err)
        if err_data.size == 0:
            return 0.0
        scale = np.maximum(1, np.abs(np.asarray(J_diff[i, j]).ravel()))
        return float(np.max(np.abs(err_data) / scale))
    J_diff = approx_derivative(fun, x0, bounds=bounds, args=args, kwargs=kwargs)
    if hasattr(J_diff, "to_host"):
        J_diff = J_diff.to_host()
        if J_diff.shape[0] == 1 and np.ndim(J) == 1:
            J_diff = J_diff.ravel()
    err = np.abs(J - J_diff)
    return float(np.max(err / np.maximum(1, np.abs(J_diff))))
