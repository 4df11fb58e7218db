"""The end-to-end problem of the dense-QR tests, shared by the fixture's generator
(tests/golden/make_golden_dense_qr.py) and tests/test_gpu_dense_qr_e2e.py: BASELINE config 2's
recipe at n = 300, m = 60 with a Jacobian of prescribed condition number."""
import numpy as np
import scipy.linalg

N, M = 300, 60
CONDS = (1e6, 1e9)


def problem(cond, n=N, m=M):
    """A = U diag(logspace(0, -log10 cond, m)) V', H = G G' + I, c, b = A x_f from
    ``default_rng(0)`` (draws in this order: U, V, G, c, x_f)."""
    rng = np.random.default_rng(0)
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    V, _ = np.linalg.qr(rng.standard_normal((n, m)))
    A = (U * np.logspace(0, -np.log10(cond), m)) @ V.T
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    H = G.dot(G.T) + np.eye(n)
    c = rng.standard_normal(n)
    xf = rng.standard_normal(n)
    return A, H, c, A.dot(xf)


def kkt_point(A, H, c, b):
    """The minimiser of 1/2 x'Hx + c'x on A x = b by a null-space solve with a complete QR of
    A': x = Q1 R^-T b + Q2 w, (Q2'H Q2) w = -Q2'(c + H Q1 R^-T b)."""
    m = A.shape[0]
    Q, R = scipy.linalg.qr(A.T, mode="full")
    Q1, Q2 = Q[:, :m], Q[:, m:]
    xr = Q1.dot(scipy.linalg.solve_triangular(R[:m], b, trans="T"))
    w = scipy.linalg.solve(Q2.T.dot(H.dot(Q2)), -Q2.T.dot(c + H.dot(xr)), assume_a="pos")
    return xr + Q2.dot(w)


def objective(H, c):
    return (lambda x: 0.5 * x.dot(H.dot(x)) + c.dot(x), lambda x: H.dot(x) + c, lambda x: H)
