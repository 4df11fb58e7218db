#!/usr/bin/env python3
"""Golden numbers of finite-difference Jacobians, by RUNNING THE REFERENCE's ``_numdiff``
(tests/golden/make_golden.py's set-up and helpers; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fd_jac.py

Writes (numbers only):

fd_jac.npz
  steps_*        ``_compute_absolute_step`` + ``_adjust_scheme_to_bounds`` on ``fd_cases.step_x0``
                 under every bound set of ``fd_cases.step_bounds``, all three methods: h and
                 use_one_sided
  <s>_*          per structure s of ``fd_cases.structures`` (tri, banded, rand): ``group_columns``
                 for order=0 and for an explicit order; per method and with / without bounds the
                 reference's h, flags, f0, every group's function values (F1, F2: G x m, recorded
                 from the calls ``_sparse_difference`` made), dx (its formulas on the recorded
                 points), the perturbed points themselves (small structures only) and its
                 Jacobian (CSR with sorted indices)
  dense*_J       three dense differences (``fd_cases.dense_cases``)

e2e_fd_jac.json
  ``synthetic.CenteredBandedNLP(2000, 200, eps=1e-3)`` with the constraint Jacobian by
  ``approx_derivative(constr_fun, x, method, sparsity=(S, groups))``, both methods x '2-point' /
  '3-point': ``run_e2e`` records; their ``one_ulp`` record is made by ``one_ulp_sensitivity``'s
  procedure with the CONSTRAINT VALUES USED IN THE DIFFERENCES moved by one unit in the last
  place (seeded signs, drawn anew for every evaluation) -- the input this feature is sensitive
  to.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (imports the reference as ``ipsolver``; the dtype shim)
from ipsolver import _numdiff as rnd  # noqa: E402  (the REFERENCE's)
import fd_cases  # noqa: E402

assert rnd.__file__.startswith("/root/reference"), rnd.__file__

METHODS = fd_cases.METHODS


def steps(out):
    x0 = fd_cases.step_x0()
    for name, (lb, ub) in fd_cases.step_bounds(x0).items():
        for method in METHODS:
            h = rnd._compute_absolute_step(None, x0, method)
            if method == 'cs':
                flags = np.zeros(x0.size, dtype=bool)
            else:
                h, flags = rnd._adjust_scheme_to_bounds(
                    x0, h, 1, '1-sided' if method == '2-point' else '2-sided', lb, ub)
            tag = "steps_%s_%s" % (name, fd_cases.TAG[method])
            out[tag + "_h"], out[tag + "_os"] = h, np.asarray(flags, dtype=bool)
    # a relative step given per variable
    rel = fd_cases.step_rel(x0)
    out["steps_rel_h"] = rnd._compute_absolute_step(rel, x0, '2-point')


def sparse_case(out, name, st, keep_points):
    S, fun, x0 = st["S"], st["fun"], st["x0"]
    m, n = S.shape
    out[name + "_groups0"] = rnd.group_columns(S, 0)
    out[name + "_groups_order"] = rnd.group_columns(S, st["order"])
    groups = out[name + "_groups0"]
    G = int(groups.max()) + 1
    for bounded in (False, True):
        lb, ub = fd_cases.case_bounds(x0) if bounded else (np.full(n, -np.inf), np.full(n, np.inf))
        for method in METHODS:
            tag = "%s_%s_%s" % (name, fd_cases.TAG[method], "b" if bounded else "u")
            calls = []

            def recording(x):
                f = fun(x)
                calls.append((np.array(x), np.array(f)))
                return f
            f0 = fun(x0)
            J = rnd.approx_derivative(recording, x0, method, f0=f0, bounds=(lb, ub),
                                      sparsity=(S, groups))
            J = sps.csr_matrix(J)
            J.sort_indices()
            h = rnd._compute_absolute_step(None, x0, method)
            flags = np.zeros(n, dtype=bool)
            if method != 'cs':
                h, flags = rnd._adjust_scheme_to_bounds(
                    x0, h, 1, '1-sided' if method == '2-point' else '2-sided', lb, ub)
            per = 2 if method == '3-point' else 1
            assert len(calls) == per * G
            F1 = np.empty((G, m))
            F2 = np.empty((G, m)) if per == 2 else None
            X1 = np.empty((G, n))
            X2 = np.empty((G, n)) if per == 2 else None
            dx = np.zeros(n)
            for g in range(G):
                e = groups == g
                if method == '2-point':
                    X1[g], F1[g] = calls[g]
                    dx[e] = (X1[g] - x0)[e]
                elif method == 'cs':
                    X1[g], F1[g] = calls[g][0].imag, calls[g][1].imag
                    assert np.array_equal(calls[g][0].real, x0)
                    dx[e] = (h * e)[e]
                else:
                    X1[g], F1[g] = calls[2 * g]
                    X2[g], F2[g] = calls[2 * g + 1]
                    one = flags & e
                    two = ~flags & e
                    dx[one] = X2[g][one] - x0[one]
                    dx[two] = X2[g][two] - X1[g][two]
            out[tag + "_h"], out[tag + "_os"], out[tag + "_f0"] = h, flags, f0
            out[tag + "_F1"], out[tag + "_dx"] = F1, dx
            if F2 is not None:
                out[tag + "_F2"] = F2
            if keep_points:
                out[tag + "_X1"] = X1
                if X2 is not None:
                    out[tag + "_X2"] = X2
            out[tag + "_J_data"] = J.data
            out[tag + "_J_indices"] = J.indices.astype(np.int32)
            out[tag + "_J_indptr"] = J.indptr.astype(np.int32)


def dense(out):
    for name, case in fd_cases.dense_cases().items():
        J = rnd.approx_derivative(case["fun"], case["x0"], case["method"], bounds=case["bounds"])
        out[name + "_J"] = np.asarray(J)


def one_ulp_constraint(rows, x, build, x0, kw, m, seeds=(31, 32, 33)):
    """``make_golden.one_ulp_sensitivity`` with the perturbation moved from the objective
    gradient to the constraint values the differences are formed from."""
    ref_rows = np.array([[np.nan if v is None else v for v in r] for r in rows], dtype=float)
    stable = len(ref_rows)
    sens = np.zeros((len(ref_rows), 8))
    x_sens, same_end = 0.0, True
    for seed in seeds:
        rng = np.random.default_rng(seed)
        # a new sign pattern for every evaluation: one pattern shared by f(x + h) and f(x) would
        # scale their difference, not move it
        res_p, rows_p = mg._trace_of(
            *build(lambda: 1.0 + np.ldexp(1.0, -52) * rng.choice([-1.0, 1.0], size=m)), kw)
        pr = np.array(rows_p, dtype=float)
        k = min(len(pr), len(ref_rows))
        ints = (0, 1, 7)
        agree = np.all(pr[:k][:, ints] == ref_rows[:k][:, ints], axis=1)
        first_bad = int(np.argmin(agree)) if not agree.all() else k
        stable = min(stable, first_bad)
        if len(pr) != len(ref_rows) or first_bad < k:
            same_end = False
        with np.errstate(invalid="ignore"):
            d = np.abs(pr[:k] - ref_rows[:k])
        d[~np.isfinite(d)] = 0.0
        sens[:k] = np.maximum(sens[:k], d)
        xp = np.asarray(res_p.x)
        x_sens = max(x_sens, float(np.max(np.abs(xp - x)) / max(np.max(np.abs(x)), 1e-300)))
    return {"stable_rows": int(stable), "rows": mg.jf(sens[:stable]),
            "x": x_sens if same_end else None, "seeds": list(seeds)}


def e2e(groups):
    ref, syn = mg.ref, mg.synthetic
    prob = syn.CenteredBandedNLP(2000, 200, eps=1e-3)
    S = sps.csr_matrix((np.ones(prob.A0.nnz), prob.A0.indices, prob.A0.indptr),
                       shape=prob.A0.shape)
    out = {}
    if "--no-sens" not in sys.argv:
        sys.argv.append("--no-sens")          # (run_e2e's own record perturbs the gradient)
    for method in ("equality_constrained_sqp", "tr_interior_point"):
        for fd in ("2-point", "3-point"):
            def build(scale, fd=fd):
                def cfun(x):
                    return prob.constr_fun(x) * (scale() if callable(scale) else scale)

                def jac(x):
                    return rnd.approx_derivative(cfun, x, fd, sparsity=(S, groups))
                con = ref.NonlinearConstraint(prob.constr_fun, ("equals", 0), jac,
                                              prob.constr_hess)
                return prob.fun, prob.x0, prob.grad, prob.hess, con
            key = "banded_eq_n2000_%s_jac%s" % (method, fd_cases.TAG[fd])
            kw = {"method": method}
            rec = mg.run_e2e(key, *build(1.0), **kw)
            res, rows = mg._trace_of(*build(1.0), kw)
            rec["one_ulp"] = one_ulp_constraint(rows, np.asarray(res.x), build, prob.x0, kw,
                                                prob.m)
            rec["n_groups"] = int(groups.max()) + 1
            print("  %-44s stable rows %d of %d, x moves %s"
                  % (key, rec["one_ulp"]["stable_rows"], len(rows), rec["one_ulp"]["x"]))
            out[key] = rec
    with open(os.path.join(HERE, "e2e_fd_jac.json"), "w") as f:
        json.dump(out, f)


def main():
    out = {}
    steps(out)
    for name, st in fd_cases.structures(mg.synthetic).items():
        sparse_case(out, name, st, keep_points=st["S"].shape[1] <= 64)
    dense(out)
    np.savez_compressed(os.path.join(HERE, "fd_jac.npz"), **out)
    print("fd_jac.npz: %d arrays, %d bytes" % (len(out),
                                               os.path.getsize(os.path.join(HERE, "fd_jac.npz"))))
    e2e(out["banded_groups0"])


if __name__ == "__main__":
    main()
