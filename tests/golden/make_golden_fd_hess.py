#!/usr/bin/env python3
"""Golden numbers of sparse finite-difference Hessians, by RUNNING THE REFERENCE's ``_numdiff``
(tests/golden/make_golden.py's set-up and helpers; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fd_hess.py

Writes (numbers only):

fd_hess.npz
  per problem p of ``fd_hess_cases.cases`` (banded, tri7, arrow, hole), function w (grad, jtv)
  and method: ``<p>_<w>_groups`` (``group_columns(S | S')``), the pattern ``S | S'`` (indptr,
  indices) and ``<p>_<w>_<method>_J`` -- the reference's ``approx_derivative(g, x, method,
  sparsity=(S | S', groups))`` on that pattern, explicit zeros kept -- and ``..._sym``,
  ``0.5 (J + J')`` on the same pattern.

e2e_fd_hess.json
  ``synthetic.CenteredBandedNLP(2000, 200, eps=1e-3)``, both methods x '2-point' / '3-point',
  with CALLABLE Hessians that return those symmetrised differences (``hess(x)`` of ``grad``,
  ``constr_hess(x, v)`` of ``x -> J(x)' v``): ``run_e2e`` records with its one-ulp record.
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
import fd_hess_cases as hc  # noqa: E402

assert rnd.__file__.startswith("/root/reference"), rnd.__file__


def on_pattern(J, P):
    """The values of ``J`` at the stored entries of ``P`` (CSR order), zeros where J has none."""
    tag = sps.csr_matrix((np.arange(1, P.nnz + 1, dtype=np.float64), P.indices, P.indptr),
                         shape=P.shape)
    J = sps.coo_matrix(J)
    pos = np.asarray(tag[J.row, J.col]).ravel().astype(np.int64) - 1
    assert np.all(pos >= 0), "the reference wrote outside the pattern"
    val = np.zeros(P.nnz)
    val[pos] = J.data            # (the reference's matrix holds each entry once)
    return val


def symmetrised(fun, x, method, P, groups):
    J = rnd.approx_derivative(fun, x, method, sparsity=(P, groups))
    val = on_pattern(J, P)
    M = sps.csr_matrix((val, P.indices, P.indptr), shape=P.shape)
    Mt = sps.csr_matrix(M.T)
    Mt.sort_indices()            # (P is symmetric: M' has P's pattern, explicit zeros kept)
    assert np.array_equal(Mt.indices, P.indices) and np.array_equal(Mt.indptr, P.indptr)
    return val, 0.5 * (val + Mt.data)


def kernels(out):
    for name, case in hc.cases(mg.synthetic).items():
        for which, fun in case["funs"].items():
            P = hc.sym_pattern(case, which)
            groups = rnd.group_columns(P, 0)
            key = "%s_%s" % (name, which)
            out[key + "_groups"] = groups.astype(np.int32)
            out[key + "_indptr"] = P.indptr.astype(np.int32)
            out[key + "_indices"] = P.indices.astype(np.int32)
            for method in hc.METHODS:
                J, sym = symmetrised(fun, case["x0"], method, P, groups)
                out["%s_%s_J" % (key, hc.TAG[method])] = J
                out["%s_%s_sym" % (key, hc.TAG[method])] = sym
            print("  %-14s n %5d nnz %6d G %d" % (key, case["n"], P.nnz, groups.max() + 1))


def e2e(out_npz):
    ref, syn = mg.ref, mg.synthetic
    prob = syn.CenteredBandedNLP(2000, 200, eps=1e-3)
    case = hc.cases(syn)["banded"]
    Pf, Pc = hc.sym_pattern(case, "grad"), hc.sym_pattern(case, "jtv")
    gf, gc = out_npz["banded_grad_groups"], out_npz["banded_jtv_groups"]
    out = {}
    for method in ("equality_constrained_sqp", "tr_interior_point"):
        for fd in ("2-point", "3-point"):
            def hess(x, fd=fd):
                _, sym = symmetrised(prob.grad, x, fd, Pf, gf)
                return sps.csr_matrix((sym, Pf.indices, Pf.indptr), shape=Pf.shape)

            def constr_hess(x, v, fd=fd):
                _, sym = symmetrised(lambda y: prob.constr_jac(y).T.dot(v), x, fd, Pc, gc)
                return sps.csr_matrix((sym, Pc.indices, Pc.indptr), shape=Pc.shape)
            con = ref.NonlinearConstraint(prob.constr_fun, ("equals", 0), prob.constr_jac,
                                          constr_hess)
            key = "banded_eq_n2000_%s_hess%s" % (method, hc.TAG[fd])
            rec = mg.run_e2e(key, prob.fun, prob.x0, prob.grad, hess, con, method=method)
            rec["n_groups_f"], rec["n_groups_c"] = int(gf.max()) + 1, int(gc.max()) + 1
            out[key] = rec
    with open(os.path.join(HERE, "e2e_fd_hess.json"), "w") as f:
        json.dump(out, f)


def main():
    out = {}
    kernels(out)
    np.savez_compressed(os.path.join(HERE, "fd_hess.npz"), **out)
    print("fd_hess.npz: %d arrays, %d bytes"
          % (len(out), os.path.getsize(os.path.join(HERE, "fd_hess.npz"))))
    e2e(out)


if __name__ == "__main__":
    main()
