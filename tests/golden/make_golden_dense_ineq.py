#!/usr/bin/env python3
"""Golden traces of dense constraint Jacobians with inequality rows, by RUNNING THE REFERENCE
(tests/golden/make_golden.py's set-up and helpers; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dense_ineq.py

Writes e2e_dense_ineq.json (numbers only): ``synthetic.CenteredDenseNLP(300, 60)`` under one
constraint of mixed kind (``synthetic.mixed_interval_kind``: 20 equality rows out of order,
20 rows ``(-inf, 0.05]``, 20 rows ``[-0.05, 0.05]``) solved with ``tr_interior_point``, as a
NonlinearConstraint (a new dense Jacobian every step) and as a dense LinearConstraint of the
same matrix (a constant Jacobian): the scalar trace, x, v, s and the counters, with the one-ulp
sensitivity record ``tests/test_host_logic.compare`` reads.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg  # noqa: E402  (imports the reference as ``ipsolver``)

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    syn, ref = mg.synthetic, mg.ref
    last = {}
    trace_of = mg._trace_of

    def keeping(*args):
        res, rows = trace_of(*args)
        last.setdefault("res", res)        # the unperturbed run comes first
        return res, rows
    mg._trace_of = keeping

    def record(key, *args, **kw):
        last.clear()
        rec = mg.run_e2e(key, *args, **kw)
        res = last["res"]
        # the whole multiplier and slack vectors (run_e2e keeps vectors up to 64 entries)
        rec["v"] = mg.jf(np.asarray(res.v, dtype=float).ravel())
        rec["s"] = mg.jf(np.asarray(res.s, dtype=float).ravel())
        return rec
    out = {}
    n, m = 300, 60
    prob = syn.CenteredDenseNLP(n, m, eps=1e-3)
    kind = syn.mixed_interval_kind(m)
    key = "dense_ineq_n%d" % n
    out[key] = record(key, prob.fun, prob.x0, prob.grad, prob.hess,
                      prob.constraints(ref, kind), method="tr_interior_point")
    key = "dense_lin_ineq_n%d" % n
    out[key] = record(key, prob.fun, prob.x0, prob.grad, prob.hess,
                      ref.LinearConstraint(prob.A, kind), method="tr_interior_point")
    with open(os.path.join(HERE, "e2e_dense_ineq.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
