#!/usr/bin/env python3
"""The yardstick of the sparse rank-deficient end-to-end test, by RUNNING THE REFERENCE
(tests/golden/make_golden.py's set-up, as tests/golden/make_golden_rank_deficient.py; build
container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sparse_rank_deficient.py

Writes sparse_rank_deficient_e2e.json (numbers only).  On ``sparse_deficient_cases.e2e_small()``
(the flow QP on the pure incidence matrix of the 12 x 12 grid, scaled by 2^-10, rank m - 1, a
consistent right-hand side) the reference is run twice: with the sparse matrix as it is (its
default for sparse Jacobians, the augmented system by SuperLU) and with the same matrix dense (its
pivoted QR, which notices the rank and takes the SVD exit).  Per run: ``status``, ``niter``,
``fun``, ``optimality``, ``constr_violation``, the distance ``max|x - x*| / max|x*|`` to the KKT
point of the independent rows, and how far one unit in the last place of every component of the
gradient (three seeded sign patterns) moves ``fun`` and ``x`` (relative).
"""
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg  # noqa: E402  (imports the reference as ``ipsolver``)
import sparse_deficient_cases as cases  # noqa: E402  (tests/ is on the path through make_golden)

HERE = os.path.dirname(os.path.abspath(__file__))


def solve(A, c, b, grad=None):
    import scipy.sparse as sps
    H = sps.identity(A.shape[1], format="csr")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mg.ref.minimize_constrained(lambda x: 0.5 * x.dot(x) + c.dot(x),
                                           np.zeros(A.shape[1]), grad or (lambda x: x + c),
                                           lambda x: H, mg.ref.LinearConstraint(A, ("equals", b)),
                                           method="equality_constrained_sqp")


def main():
    A, c, b, ind = cases.e2e_small()
    xs = cases.kkt_point(A[ind], c, b[ind])
    out = {}
    for name, Ain in (("sparse", A), ("dense", A.toarray())):
        res = solve(Ain, c, b)
        x = np.asarray(res.x)
        fun_ulp = x_ulp = 0.0
        for seed in (31, 32, 33):
            signs = np.random.default_rng(seed).choice([-1.0, 1.0], size=c.size)
            rp = solve(Ain, c, b, lambda xx: (xx + c) * (1.0 + np.ldexp(1.0, -52) * signs))
            fun_ulp = max(fun_ulp, abs(rp.fun - res.fun) / abs(res.fun))
            x_ulp = max(x_ulp, float(np.max(np.abs(np.asarray(rp.x) - x)) / np.max(np.abs(x))))
        rec = {"status": int(res.status), "niter": int(res.niter), "fun": float(res.fun),
               "optimality": float(res.optimality),
               "constr_violation": float(res.constr_violation),
               "distance": float(np.max(np.abs(x - xs)) / np.max(np.abs(xs))),
               "fun_one_ulp": float(fun_ulp), "x_one_ulp": float(x_ulp)}
        print("%s: %s" % (name, rec))
        out[name] = rec
    with open(os.path.join(HERE, "sparse_rank_deficient_e2e.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
