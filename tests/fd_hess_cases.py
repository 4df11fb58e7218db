"""Inputs of the sparse finite-difference Hessian tests, shared by the generator of their goldens
(tests/golden/make_golden_fd_hess.py, which runs the reference on them) and by the tests
(test_fd_hessian_host.py, test_gpu_fd_hessian.py).  Own code; numpy / scipy only.

A case is a function ``g: R^n -> R^n`` whose Jacobian lies inside a structurally symmetric
pattern ``S | S'`` but is NOT symmetric itself (so the symmetrisation shows), built from
``+ - *`` and CSR products only (tests/fd_cases.py).  Per problem there are two: ``grad`` -- the
polynomial ``A x + kappa/2 W (x*x) - b`` -- and ``jtv`` -- ``x -> J(x)' v`` of the constraint
``c = A x + kappa/2 W (x*x) - b`` with ``v`` frozen, whose derivative is diagonal: every other
stored entry is an explicit zero.

Problems: ``banded`` (``CenteredBandedNLP(2000, 200)``: its own ``grad`` on the tridiagonal
pattern, its own ``J(x)' v`` on the diagonal), ``tri7`` (one partial tile, fewer entries than
lanes; the structure is handed over as its LOWER triangle + diagonal, so it must be symmetrised),
``arrow`` (n = 2100: row 0 and column 0 full, 2100 > IPX_SPMV_TILE_NNZ = 2048 entries in one row,
G = n groups) and ``hole`` (a random pattern whose row and column 5 are empty)."""
import numpy as np
import scipy.sparse as sps

from fd_cases import KAPPA, METHODS, TAG  # noqa: F401

ARROW_N = 2100


def _sym(S):
    S = sps.csr_matrix(S)
    P = sps.csr_matrix(((S + S.T) != 0).astype(np.int8))
    P.sort_indices()
    return P


def _poly_case(A, seed, structure=None):
    A = sps.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    W = sps.csr_matrix((A.data * A.data, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    At, Wt = sps.csr_matrix(A.T), sps.csr_matrix(W.T)
    At.sort_indices()
    Wt.sort_indices()
    x0, b, v = rng.uniform(-1, 1, n), rng.standard_normal(n), rng.standard_normal(n)
    atv, wtv = At.dot(v), Wt.dot(v)

    def grad(x):
        return A.dot(x) + 0.5 * KAPPA * W.dot(x * x) - b

    def jtv(x):
        return atv + KAPPA * (x * wtv)
    S = sps.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return {"n": n, "structure": S if structure is None else structure, "P": _sym(S), "x0": x0,
            "A": A, "W": W, "b": b, "v": v, "atv": atv, "wtv": wtv,
            "funs": {"grad": grad, "jtv": jtv}}


def cases(synthetic):
    out = {}
    prob = synthetic.CenteredBandedNLP(2000, 200, eps=1e-3)
    v = np.random.default_rng(21).standard_normal(prob.m)
    Sf = sps.csr_matrix((np.ones(prob.Q.nnz), prob.Q.indices, prob.Q.indptr), shape=prob.Q.shape)
    out["banded"] = {"n": prob.n, "x0": prob.x0, "v": v, "prob": prob,
                     "structures": {"grad": Sf, "jtv": sps.identity(prob.n, format="csr")},
                     "funs": {"grad": prob.grad,
                              "jtv": lambda x: prob.constr_jac(x).T.dot(v)}}
    rng = np.random.default_rng(12)
    n = 7
    tri = sps.diags([rng.standard_normal(n - 1), rng.standard_normal(n),
                     rng.standard_normal(n - 1)], [-1, 0, 1], format="csr")
    out["tri7"] = _poly_case(tri, 4, structure=sps.csr_matrix(sps.tril(abs(tri) > 0)))
    n = ARROW_N
    arrow = sps.lil_matrix((n, n))
    arrow[0, :] = rng.standard_normal(n)
    arrow[:, 0] = rng.standard_normal(n).reshape(n, 1)
    arrow.setdiag(rng.standard_normal(n))
    out["arrow"] = _poly_case(arrow.tocsr(), 5)
    n = 40
    R = sps.random(n, n, density=0.1, random_state=np.random.RandomState(6), format="lil",
                   data_rvs=np.random.RandomState(7).standard_normal)
    R.setdiag(np.random.RandomState(8).standard_normal(n))
    R[5, :] = 0
    R[:, 5] = 0
    R = sps.csr_matrix(R)
    R.eliminate_zeros()
    out["hole"] = _poly_case(R, 6)
    for name in ("tri7", "arrow", "hole"):
        c = out[name]
        c["structures"] = {"grad": c["structure"], "jtv": c["structure"]}
    return out


def sym_pattern(case, which):
    """``S | S'`` of a case's structure: sorted CSR 0/1."""
    return _sym(case["structures"][which])


def planes(plan, fun, x0, method):
    """(f0, F1, F2, dx, h, one_sided) of ``fun`` at the plan's perturbed points, by the library's
    host entries for the steps and the points (pinned to the reference's bits by
    test_fd_jacobian_host.py) and numpy for the function."""
    from ipsolver.fd_jacobian import steps_host, perturb_host
    h, flags = steps_host(x0, method)
    G, n = plan.n_groups, plan.n
    dx = np.zeros(n)
    F1 = np.empty((G, n))
    F2 = np.empty((G, n)) if method == '3-point' else None
    for g in range(G):
        x1, x2 = perturb_host(x0, h, flags, plan.groups, g, method, dx)
        if method == 'cs':
            F1[g] = fun(x0 + 1j * x1).imag
        else:
            F1[g] = fun(x1)
        if x2 is not None:
            F2[g] = fun(x2)
    f0 = None if method == 'cs' else fun(x0)
    return f0, F1, F2, dx, h, flags
