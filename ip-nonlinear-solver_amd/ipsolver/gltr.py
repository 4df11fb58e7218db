"""Projected GLTR: the trust-region subproblem solved over the whole Krylov space.

``projected_cg`` (Steihaug-Toint) stops at the first negative curvature or the first crossing of
the sphere and returns the point where the current CG direction meets it.  The Generalized
Lanczos Trust Region method (Gould, Lucidi, Roma & Toint 1999) keeps the Lanczos tridiagonal
``T_k`` that CG builds implicitly, goes on past the boundary and returns

    x = x0 + Q_k h,   h = argmin 1/2 h'T_k h + gamma_0 h_0   s.t. ||h|| <= R,

the minimiser of the model over the Krylov space inside the sphere.  It stands on ``H.dot`` and
``Z.dot`` like the general driver of ``qp.projected_cg`` (every Hessian kind, every projector);
the vector step with its reductions, the tridiagonal trust-region solve with its decision and
the recombination are csrc/gltr.hip.  Steps are enqueued in batches behind a stop word on the
device; one read of the 16-double header per batch.  Sphere only: no box.
"""
from math import sqrt

import numpy as np

from . import _hip
from . import device as dv
from .device import DVec, _p, stream_ptr

__all__ = ['projected_gltr', 'MAX_VECTORS']

MAX_VECTORS = 256           # IPX_GLTR_MAX_VECTORS
_HDR = 16
_TINY = 1e-25               # CLOSE_TO_ZERO (qp.py)
_BATCH_MIN, _BATCH_MAX = 2, 8

ST_STOP, ST_K, ST_GAMMA0, ST_R, ST_TOL, ST_LAMBDA, ST_HNORM, ST_Q, ST_GNEXT, ST_CASE = range(10)
ST_PATH, ST_ROUNDS = 11, 12

STATS = {"calls": 0, "vectors": 0, "boundary": 0, "state_reads": 0}

_WORK = {}


class _Work:
    """Q (max_vectors + 1 columns), the state block and the partial sums of one problem size."""

    def __init__(self, n, kmax):
        import torch
        lib = _hip.load()
        dev = dv.ctx().device
        self.Q = torch.zeros(n * (kmax + 1), dtype=torch.float64, device=dev)
        self.state = torch.zeros(int(lib.ipx_gltr_state_doubles(kmax)), dtype=torch.float64,
                                 device=dev)
        self.part = torch.zeros(int(lib.ipx_gltr_part_doubles(n)), dtype=torch.float64, device=dev)
        self.cols = [DVec(self.Q[j * n:(j + 1) * n]) for j in range(kmax + 1)]


def _work(n, kmax):
    key = (n, kmax, dv.ctx().device.index)
    w = _WORK.get(key)
    if w is None:
        if len(_WORK) >= 4:                 # (a few problem sizes at a time: Q is the big one)
            _WORK.pop(next(iter(_WORK)))
        w = _WORK[key] = _Work(n, kmax)
    return w


def check_max_vectors(max_vectors):
    if isinstance(max_vectors, bool) or int(max_vectors) != max_vectors \
            or not 1 <= int(max_vectors) <= MAX_VECTORS:
        raise ValueError("max_vectors must be an integer in 1..%d, got %r"
                         % (MAX_VECTORS, max_vectors))
    return int(max_vectors)


def projected_gltr(H, c, Z, Y, b, trust_radius, tol=None, max_iter=None, max_vectors=64,
                   return_all=False):
    """Minimise 1/2 x'Hx + c'x subject to Ax + b = 0, ||x|| <= trust_radius over the Krylov
    space of the projected Hessian.  Arguments as ``qp.projected_cg`` (``b=None`` stands for
    b = 0); returns ``(x, info)`` with ``niter`` (Lanczos vectors = Hessian products),
    ``stop_cond`` (4 tolerance or invariant subspace, 1 cap, 2 ``x0`` on the boundary),
    ``hits_boundary`` and the extension keys ``multiplier`` (lambda) and ``predicted``
    (q(x) - q(x0))."""
    from . import qp
    kmax = check_max_vectors(max_vectors)
    if getattr(getattr(Z, "projector", None), "sh", None) is not None or hasattr(c, "sh"):
        raise NotImplementedError("projected_gltr: the row-sharded backend has no GLTR; the "
                                  "method is available on one GPU only")
    r2 = float(trust_radius) * float(trust_radius)
    if np.isinf(r2):
        # no sphere: GLTR is CG there, and negative curvature must raise as it does today
        x, info = qp.projected_cg(H, c, Z, Y, b, trust_radius, tol=tol, max_iter=max_iter,
                                  return_all=return_all)
        info = dict(info, multiplier=0.0, predicted=None)
        return x, info
    b_zero = b is None
    if not b_zero and not hasattr(b, "sumsq_amax"):
        bh = np.asarray(b, dtype=float)
        if bh.ndim == 1 and not bh.any():
            b_zero = True
    c = qp._vec(c)
    n, m = len(c), Y.shape[1]
    if b_zero:
        x0, norm_x0 = None, 0.0
        g = Z.dot(Z.dot(c))
    else:
        x0 = Y.dot(-qp._vec(b))
        g = Z.dot(Z.dot(H.dot(x0) + c))
        norm_x0 = dv.norm(x0)

    def done(x, k, stop, boundary, lam=0.0, pred=0.0, allvecs=None):
        info = {'niter': k, 'stop_cond': stop, 'hits_boundary': boundary,
                'multiplier': lam, 'predicted': pred}
        if return_all:
            info['allvecs'] = allvecs if allvecs is not None else [x, x]
        return x, info

    tr_distance = trust_radius - norm_x0
    if tr_distance < 0:
        raise ValueError("Trust region problem does not have a solution.")
    if tr_distance < _TINY:
        return done(x0 if x0 is not None else c.zeros_like(), 0, 2, True)
    R = sqrt(r2 - norm_x0 * norm_x0)
    cap = n - m if max_iter is None else min(int(max_iter), n - m)
    cap = max(0, min(cap, kmax))

    W = _work(n, kmax)
    st = stream_ptr()
    Qp, sp, pp = _p(W.Q), _p(W.state), _p(W.part)
    _hip.call("ipx_gltr_start", n, kmax, cap, _p(g.t), Qp, sp, pp, R,
              -1.0 if tol is None else float(tol), st)
    x0p = None if x0 is None else _p(x0.t)

    def combine():
        out = dv._empty(n)
        _hip.call("ipx_gltr_combine", n, kmax, Qp, sp, x0p, _p(out), stream_ptr())
        return DVec(out)

    allvecs = [x0 if x0 is not None else c.zeros_like()] if return_all else None
    enq = 0
    hdr = None
    batch = 1 if return_all else _BATCH_MIN
    while True:
        end = min(cap, enq + batch)
        for j in range(enq, end):
            w = Z.dot(H.dot(W.cols[j]))
            _hip.call("ipx_gltr_step", n, kmax, _p(w.t), Qp, sp, pp, stream_ptr())
        enq = end
        hdr = dv.read_doubles(W.state, _HDR)
        STATS["state_reads"] += 1
        if return_all and int(hdr[ST_K]) == enq and enq > 0:
            allvecs.append(combine())
        if hdr[ST_STOP] != 0 or enq >= cap:
            break
        batch = 1 if return_all else min(_BATCH_MAX, 2 * batch)
    k = int(hdr[ST_K])
    stop = int(hdr[ST_STOP]) or 1
    x = combine() if k > 0 else (x0 if x0 is not None else c.zeros_like())
    lam = float(hdr[ST_LAMBDA])
    boundary = bool(k > 0 and (lam > 0 or hdr[ST_CASE] == 2))
    STATS["calls"] += 1
    STATS["vectors"] += k
    STATS["boundary"] += 1 if boundary else 0
    return done(x, k, stop, boundary, lam, float(hdr[ST_Q]) if k > 0 else 0.0, allvecs)
