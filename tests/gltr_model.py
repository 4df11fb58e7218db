"""numpy / scipy references for the projected GLTR tests (no GPU, no library code).

(i)   ``gltr``: the Lanczos recurrence of the issue with an eigendecomposition-based tridiagonal
      trust-region solve;
(ii)  ``exact_constrained``: the exact minimiser over null(A) inside the sphere (null-space basis,
      dense ``eigh``, a bracketed root for the multiplier);
(iii) ``steihaug``: projected CG as ``qp.projected_cg``'s general driver runs it (sphere only);
(iv)  ``tridiag_reference``: ``eigh`` of the tridiagonal with 200 bisection steps on lambda, and
      the eigenvector step to the boundary when ||h|| < R (1 - 1e-9) at the pole.
"""
import numpy as np
import scipy.linalg as sl

TINY = 1e-25


def tridiag_dense(diag, off):
    k = len(diag)
    T = np.diag(np.asarray(diag, dtype=float))
    for i in range(k - 1):
        T[i, i + 1] = T[i + 1, i] = off[i]
    return T


def _tr_by_eigh(B, g, R):
    """argmin 1/2 h'Bh + g'h over ||h|| <= R for a dense symmetric B: (h, lambda, case) with case
    0 interior, 1 boundary, 2 hard (a step along the lowest eigenvector was added)."""
    g = np.asarray(g, dtype=float)
    ev, V = np.linalg.eigh(B)
    a = V.T @ g

    def h_of(lam):
        return -V @ (a / (ev + lam))

    if ev[0] > 0:
        h = h_of(0.0)
        if np.linalg.norm(h) <= R:
            return h, 0.0, 0
    gn = np.linalg.norm(g)
    pole = max(0.0, -ev[0])
    lo = pole
    hi = pole + gn / R + 1e-300
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        with np.errstate(divide="ignore", over="ignore"):
            nrm = np.linalg.norm(a / (ev + mid))
        if nrm > R:
            lo = mid
        else:
            hi = mid
    lam = hi
    h = h_of(lam)
    nh = np.linalg.norm(h)
    if nh < R * (1 - 1e-9):
        # no root right of the pole in floating point: the eigenvector step to the boundary
        u = V[:, 0]
        hu = h @ u
        c = h @ h - R * R
        disc = max(hu * hu - c, 0.0)
        taus = [-hu + np.sqrt(disc), -hu - np.sqrt(disc)]
        cands = [h + t * u for t in taus]
        q = [0.5 * x @ B @ x + g @ x for x in cands]
        return cands[int(np.argmin(q))], lam, 2
    return h, lam, 1


def tridiag_reference(diag, off, g0, R):
    """(iv): (h, lambda, case, q) for T = tridiag(diag; off), g = g0 e_1."""
    k = len(diag)
    T = tridiag_dense(diag, off)
    g = np.zeros(k)
    g[0] = g0
    h, lam, case = _tr_by_eigh(T, g, R)
    return h, lam, case, 0.5 * h @ T @ h + g0 * h[0]


def _start(H, c, A, b):
    """x0 = Y(-b), g0 = Z(Z(H x0 + c)) with dense normal-equation projectors."""
    n = len(c)
    AAt = A @ A.T

    def Z(v):
        return v - A.T @ np.linalg.solve(AAt, A @ v)

    x0 = np.zeros(n) if b is None else -A.T @ np.linalg.solve(AAt, b)
    g = Z(Z(H @ x0 + c))
    return x0, g, Z


def default_tol(gamma0):
    return max(min(0.01 * gamma0, 0.1 * gamma0 ** 2), TINY)


def gltr(H, c, A, b, radius, tol=None, max_iter=None, max_vectors=64):
    """(i): returns (x, info) with info as ``projected_gltr``'s."""
    n, m = len(c), A.shape[0]
    x0, g, Z = _start(H, c, A, b)
    gamma0 = np.linalg.norm(g)
    nx0 = np.linalg.norm(x0)
    if radius < nx0:
        raise ValueError("Trust region problem does not have a solution.")
    if radius - nx0 < TINY:
        return x0, dict(niter=0, stop_cond=2, hits_boundary=True, multiplier=0.0, predicted=0.0)
    if tol is None:
        tol = default_tol(gamma0)
    if gamma0 ** 2 < tol:
        return x0, dict(niter=0, stop_cond=4, hits_boundary=False, multiplier=0.0, predicted=0.0)
    R = np.sqrt(radius ** 2 - nx0 ** 2)
    cap = min(n - m if max_iter is None else min(max_iter, n - m), max_vectors)
    Q = [g / gamma0]
    diag, off = [], []
    gk = 0.0
    stop = 1
    h = np.zeros(0)
    lam, case = 0.0, 0
    for k in range(cap):
        w = Z(H @ Q[k])
        delta = Q[k] @ w
        w = w - delta * Q[k]
        if k > 0:
            w = w - gk * Q[k - 1]
        gnext = np.linalg.norm(w)
        diag.append(delta)
        T = tridiag_dense(diag, off)
        g1 = np.zeros(k + 1)
        g1[0] = gamma0
        h, lam, case = _tr_by_eigh(T, g1, R)
        if gnext <= 1e-14 * gamma0 or (gnext * h[k]) ** 2 < tol:
            stop = 4
            break
        off.append(gnext)
        gk = gnext
        Q.append(w / gnext)
    k = len(h)
    x = x0 + sum(h[j] * Q[j] for j in range(k))
    T = tridiag_dense(diag, off[:k - 1])
    pred = 0.5 * h @ T @ h + gamma0 * h[0]
    return x, dict(niter=k, stop_cond=stop, hits_boundary=bool(lam > 0 or case == 2),
                   multiplier=float(lam), predicted=float(pred))


def exact_constrained(H, c, A, b, radius):
    """(ii): the minimiser of 1/2 x'Hx + c'x over Ax + b = 0, ||x|| <= radius."""
    n = len(c)
    AAt = A @ A.T
    x0 = np.zeros(n) if b is None else -A.T @ np.linalg.solve(AAt, b)
    N = sl.null_space(A)
    R = np.sqrt(radius ** 2 - x0 @ x0)
    B = N.T @ H @ N
    B = 0.5 * (B + B.T)
    gr = N.T @ (H @ x0 + c)
    y, lam, case = _tr_by_eigh(B, gr, R)
    return x0 + N @ y, lam, case


def steihaug(H, c, A, b, radius, tol=None, max_iter=None):
    """(iii): the sphere-only branch of ``qp.projected_cg``'s general driver."""
    n, m = len(c), A.shape[0]
    x, _, Z = _start(H, c, A, b)
    r = Z(H @ x + c)
    g = Z(r)
    p = -g
    Hp = H @ p
    rtg = np.linalg.norm(g) ** 2
    if tol is None:
        tol = max(min(0.01 * np.sqrt(rtg), 0.1 * rtg), TINY)
    cap = n - m if max_iter is None else min(max_iter, n - m)

    def to_sphere(x, d, entire_line):
        a, bq, cq = d @ d, 2 * (x @ d), x @ x - radius ** 2
        s = np.sqrt(bq * bq - 4 * a * cq)
        aux = bq + np.copysign(s, bq)
        ta, tb = sorted([-aux / (2 * a), -2 * cq / aux])
        return tb if entire_line else min(1.0, tb)

    k = 0
    stop = 1
    hits = False
    for _ in range(cap):
        if rtg < tol:
            stop = 4
            break
        k += 1
        pHp = Hp @ p
        if pHp <= 0:
            x = x + to_sphere(x, p, True) * p
            stop, hits = 3, True
            break
        alpha = rtg / pHp
        xn = x + alpha * p
        if np.linalg.norm(xn) >= radius:
            x = x + to_sphere(x, alpha * p, False) * alpha * p
            stop, hits = 2, True
            break
        r = r + alpha * Hp
        gn = Z(r)
        rtgn = np.linalg.norm(gn) ** 2
        p = -gn + (rtgn / rtg) * p
        x, r, rtg = xn, gn, rtgn
        Hp = H @ p
    return x, dict(niter=k, stop_cond=stop, hits_boundary=hits)


def model_value(H, c, x):
    return 0.5 * x @ (H @ x) + c @ x
