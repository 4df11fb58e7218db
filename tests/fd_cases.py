"""Inputs of the finite-difference Jacobian tests, shared by the generator of their goldens
(tests/golden/make_golden_fd_jac.py, which runs the reference on them) and by the tests
(test_fd_jacobian_host.py, test_gpu_fd_jacobian.py).  Own code; numpy / scipy only.

Every test function is a polynomial built from ``+ - *`` and CSR products only, so that numpy /
scipy on the host and the elementwise kernels / row-order SpMV of the device compute the same
bits."""
import numpy as np
import scipy.sparse as sps

METHODS = ('2-point', '3-point', 'cs')
TAG = {'2-point': '2p', '3-point': '3p', 'cs': 'cs'}
KAPPA = 0.1


def step_x0():
    """0, -0, tiny, ordinary and large magnitudes of both signs, each repeated once per bound
    combination of ``step_bounds``."""
    base = np.array([0.0, -0.0, 1e-300, -1e-300, 1e-8, -1e-8, 0.5, -0.5, 1.0, -1.0, 3.7, -3.7,
                     1e8, -1e8, 1e15, -1e15])
    return np.repeat(base, len(_DISTANCES))


# (distance to the lower bound, distance to the upper bound): on a bound, next to it (closer than
# the steps of 1.5e-8 / 6e-6), closer than two steps, far from it, none
_DISTANCES = [(0.0, np.inf), (np.inf, 0.0), (0.0, 1.0), (1.0, 0.0), (1e-12, 1.0), (1.0, 1e-12),
              (1e-9, 1e-9), (1e-9, 3e-9), (4e-6, 1e-3), (1e-3, 4e-6), (1e-5, 1e-5), (0.0, 0.0),
              (2.0, 3.0), (np.inf, 1e-7), (1e-7, np.inf), (5e-6, 7e-6)]


def step_bounds(x0):
    """Bound sets by name: none, lower only, upper only, both (tight enough to flip or shrink a
    step and to switch '3-point' to one-sided).  ``x0`` lies inside all of them."""
    k = len(x0) // len(_DISTANCES)
    dl = np.tile(np.array([d[0] for d in _DISTANCES]), k)
    du = np.tile(np.array([d[1] for d in _DISTANCES]), k)
    inf = np.full(len(x0), np.inf)
    return {"none": (-inf, inf), "lower": (x0 - dl, inf), "upper": (-inf, x0 + du),
            "both": (x0 - dl, x0 + du)}


def step_rel(x0):
    return np.random.default_rng(5).uniform(1e-9, 1e-3, len(x0))


def case_bounds(x0):
    """Bounds for the Jacobian cases: a third of the variables close to a lower bound, a third
    close to an upper one (closer than the '3-point' step), the rest free."""
    n = len(x0)
    lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    lb[0::3] = x0[0::3] - 1e-7
    ub[0::3] = x0[0::3] + 2.0
    ub[1::3] = x0[1::3] + 1e-9
    return lb, ub


def poly_fun(A, W, b):
    """``c(x) = A x + kappa/2 W (x*x) - b`` over scipy CSR matrices (real or complex x)."""
    def fun(x):
        return A.dot(x) + 0.5 * KAPPA * W.dot(x * x) - b
    return fun


def _structure(A, seed, order):
    A = sps.csr_matrix(A)
    A.sort_indices()
    m, n = A.shape
    rng = np.random.default_rng(seed)
    S = sps.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    W = sps.csr_matrix((A.data * A.data, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    x0 = rng.uniform(-1, 1, n)
    b = rng.standard_normal(m)
    return {"S": S, "A": A, "W": W, "b": b, "x0": x0, "fun": poly_fun(A, W, b), "order": order}


def structures(synthetic):
    """tri: tridiagonal 12 x 12; banded: ``CenteredBandedNLP(2000, 200).A0``; rand: a seeded random
    30 x 40 pattern with an empty row, an empty column and -- stored in the structure -- entries
    on which the function does not depend (their derivative is an explicit zero)."""
    out = {}
    rng = np.random.default_rng(11)
    n = 12
    tri = sps.diags([rng.standard_normal(n - 1), rng.standard_normal(n),
                     rng.standard_normal(n - 1)], [-1, 0, 1], format="csr")
    out["tri"] = _structure(tri, 1, np.arange(n)[::-1].copy())
    prob = synthetic.CenteredBandedNLP(2000, 200, eps=1e-3)
    out["banded"] = _structure(prob.A0, 2, np.roll(np.arange(2000), 7))
    m, n = 30, 40
    R = sps.random(m, n, density=0.12, random_state=np.random.RandomState(3), format="lil",
                   data_rvs=np.random.RandomState(4).standard_normal)
    R[5, :] = 0
    R[:, 7] = 0
    R = sps.csr_matrix(R)
    R.eliminate_zeros()
    R.sort_indices()
    st = _structure(R, 3, np.random.RandomState(9).permutation(n))
    # every fourth stored value is 0: a structural entry the function does not depend on
    A = st["A"].copy()
    A.data[::4] = 0.0
    st["A"], st["W"] = A, sps.csr_matrix((A.data * A.data, A.indices, A.indptr), shape=A.shape)
    st["fun"] = poly_fun(st["A"], st["W"], st["b"])
    out["rand"] = st
    return out


def dense_poly(n, m, seed):
    """``f_i = a_i x[p_i] x[q_i] + c_i x[r_i] - d_i``: gathers and ``+ - *`` only.  Returns the
    tables; ``dense_fun`` evaluates them with numpy, the GPU test with torch."""
    rng = np.random.default_rng(seed)
    return {"p": rng.integers(0, n, m), "q": rng.integers(0, n, m), "r": rng.integers(0, n, m),
            "a": rng.standard_normal(m), "c": rng.standard_normal(m), "d": rng.standard_normal(m)}


def dense_fun(t):
    def fun(x):
        return t["a"] * x[t["p"]] * x[t["q"]] + t["c"] * x[t["r"]] - t["d"]
    return fun


def dense_cases():
    out = {}
    for name, (m, n, method, bounded) in {"dense0": (3, 4, '2-point', False),
                                          "dense1": (1, 5, '3-point', True),
                                          "dense2": (4, 1, 'cs', False)}.items():
        t = dense_poly(n, m, 20 + m)
        x0 = np.random.default_rng(30 + n).uniform(-1, 1, n)
        bounds = case_bounds(x0) if bounded else (-np.inf, np.inf)
        out[name] = {"tables": t, "fun": dense_fun(t), "x0": x0, "method": method,
                     "bounds": bounds, "m": m, "n": n}
    return out
