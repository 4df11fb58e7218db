"""The arithmetic of the radius guard (csrc/ipx_common.h ipx_rguard, exported as
ipx_rguard_start / ipx_rguard_step_x / ipx_rguard_step_q: the code the lead lanes of the loop's
kernels run) on the host: a numpy projected CG is driven for 300 iterations through the exported
steps, and after every iteration X >= ||x|| and Q >= ||p|| against norms summed in longdouble.

The Hessian's eigenvalues spread over 1e10 and the null space has 300 dimensions, so the CG does
not converge within the run and loses orthogonality on the way: the bounds use the triangle
inequality alone and do not care.  ||g||^2 reaches the helper as a float64 sum in an order of its
own (reversed, in fours), as the kernels' order differs from numpy's.
"""
import numpy as np

N, M, ITERATIONS = 400, 100, 300


def _problem():
    rng = np.random.default_rng(11)
    A = rng.standard_normal((M, N))
    Qm, _ = np.linalg.qr(rng.standard_normal((N, N)))
    H = (Qm * np.logspace(0.0, 10.0, N)) @ Qm.T
    H = 0.5 * (H + H.T)
    c = rng.standard_normal(N)
    G = np.linalg.inv(A @ A.T)

    def Z(v):
        return v - A.T @ (G @ (A @ v))
    return H, c, Z


def _sumsq(v):
    """A float64 sum of squares in an order that is not numpy's pairwise one."""
    return float(np.sum((v * v)[::-1].reshape(-1, 4).sum(axis=1)))


def _norm_ld(v):
    w = v.astype(np.longdouble)
    return np.sqrt(np.sum(w * w))


def test_bounds_hold_over_300_iterations():
    from ipsolver import _hip
    lib = _hip.load()
    assert lib.ipx_rguard_start(1.0) == 1.0 + 2.0 ** -20
    assert lib.ipx_rguard_step_x(1.0, 2.0, -3.0) == (1.0 + 3.0 * 2.0) * (1.0 + 2.0 ** -20)
    assert lib.ipx_rguard_step_q(2.0, 0.5, 9.0) == (0.5 * 2.0 + 3.0) * (1.0 + 2.0 ** -20)
    H, c, Z = _problem()
    x = np.zeros(N)
    r = Z(c)
    g = Z(r)
    p = -g
    rt_g = _sumsq(g)
    X, Q = lib.ipx_rguard_start(0.0), lib.ipx_rguard_start(rt_g)
    assert X == 0.0 and Q >= _norm_ld(p)
    worst = 1.0
    for it in range(ITERATIONS):
        Hp = H @ p
        alpha = rt_g / float(p @ Hp)                 # qp_subproblem.py:579
        T = lib.ipx_rguard_step_x(X, Q, alpha)
        x = x + alpha * p                            # :580, 630
        r = r + alpha * Hp                           # :622
        g = Z(r)
        gg = _sumsq(g)
        beta = gg / rt_g                             # :627
        p = beta * p - g                             # :628
        X, Q = T, lib.ipx_rguard_step_q(Q, beta, gg)
        r, rt_g = g, gg
        nx, npn = _norm_ld(x), _norm_ld(p)
        assert np.isfinite(X) and np.isfinite(Q)
        assert X >= nx and Q >= npn, (it, X, float(nx), Q, float(npn))
        worst = max(worst, float(X / nx))
    # (a figure, not a bound: how loose the guard is on this trajectory)
    print("radius guard on the host: max X/||x|| over %d iterations %.4g" % (ITERATIONS, worst))
