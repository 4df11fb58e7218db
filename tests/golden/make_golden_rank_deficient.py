#!/usr/bin/env python3
"""The yardstick of the rank-deficient end-to-end test, by RUNNING THE REFERENCE
(tests/golden/make_golden.py's set-up, as tests/golden/make_golden_dense_qr.py; build container
only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rank_deficient.py

Writes rank_deficient_e2e.json (numbers only).  Per cond of
``rank_deficient_cases.E2E_CONDS``, on ``rank_deficient_cases.e2e_problem(cond)`` (the dense-QR
problem scaled by 2^-10, six consistent combination rows added, rows permuted): the reference's
``status``, ``niter``, ``fun``, ``optimality``, ``constr_violation``, its distance
``max|x - x*| / max|x*|`` to the KKT point of the independent rows
(``dense_qr_cases.kkt_point``), and how far one unit in the last place of every component of the
gradient (three seeded sign patterns) moves its ``fun`` and its ``x`` (relative).

The UNSCALED variant of the same problem is not part of the fixture: the reference does not
converge on it (its absolute tol = 1e-15 keeps spurious singular values of 3-6e-16; DESIGN.md
section 4o).
"""
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg  # noqa: E402  (imports the reference as ``ipsolver``)
import dense_qr_cases  # noqa: E402  (tests/ is on the path through make_golden)
import rank_deficient_cases as cases  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def solve(A, H, c, b, grad=None):
    fun, grad0, hess = dense_qr_cases.objective(H, c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mg.ref.minimize_constrained(fun, np.zeros(A.shape[1]), grad or grad0, hess,
                                           mg.ref.LinearConstraint(A, ("equals", b)),
                                           method="equality_constrained_sqp")


def main():
    out = {}
    for cond in cases.E2E_CONDS:
        A, H, c, b, ind = cases.e2e_problem(cond)
        xs = dense_qr_cases.kkt_point(A[ind], H, c, b[ind])
        res = solve(A, H, c, b)
        x = np.asarray(res.x)
        fun_ulp = x_ulp = 0.0
        for seed in (31, 32, 33):
            signs = np.random.default_rng(seed).choice([-1.0, 1.0], size=c.size)
            rp = solve(A, H, c, b,
                       lambda xx: (H.dot(xx) + c) * (1.0 + np.ldexp(1.0, -52) * signs))
            fun_ulp = max(fun_ulp, abs(rp.fun - res.fun) / abs(res.fun))
            x_ulp = max(x_ulp, float(np.max(np.abs(np.asarray(rp.x) - x)) / np.max(np.abs(x))))
        rec = {"status": int(res.status), "niter": int(res.niter), "fun": float(res.fun),
               "optimality": float(res.optimality),
               "constr_violation": float(res.constr_violation),
               "distance": float(np.max(np.abs(x - xs)) / np.max(np.abs(xs))),
               "fun_one_ulp": float(fun_ulp), "x_one_ulp": float(x_ulp)}
        print("cond %.0e: %s" % (cond, rec))
        out["cond_%.0e" % cond] = rec
    with open(os.path.join(HERE, "rank_deficient_e2e.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
