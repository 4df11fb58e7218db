"""Projected GLTR without a GPU: the tridiagonal trust-region solve's host twin against an
eigendecomposition, the numpy model of the method against the exact constrained minimiser, and
the validation of the ``subproblem`` option."""
import ctypes

import numpy as np
import pytest

import gltr_cases
import gltr_model


def tridiag_host(diag, off, g0, R):
    from ipsolver import _hip
    lib = _hip.load()
    k = len(diag)
    diag = np.ascontiguousarray(diag, dtype=float)
    off = np.ascontiguousarray(off if k > 1 else np.zeros(1), dtype=float)
    out = np.zeros(8 + k)
    rc = lib.ipx_gltr_tridiag_host(k, diag.ctypes.data_as(ctypes.c_void_p),
                                   off.ctypes.data_as(ctypes.c_void_p), g0, R,
                                   out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return dict(lam=out[0], hnorm=out[1], q=out[2], case=int(out[3]), path=int(out[4]),
                rounds=int(out[5]), h=out[8:].copy())


def test_tridiagonal_solve_against_eigh():
    """Issue bounds: q_T(h) <= q_ref + 1e-10 |q_ref|, ||h|| <= R (1 + 1e-10), | ||h|| - R | <=
    1e-10 R whenever lambda > 0; at least 100 of the 600 random problems take the near-hard or
    the collapsed-bracket exit."""
    cases = gltr_cases.tridiagonals()
    hard = 0
    worst_gap = worst_norm = 0.0
    for idx, (diag, off, g0, R) in enumerate(cases):
        got = tridiag_host(diag, off, g0, R)
        _, _, _, q_ref = gltr_model.tridiag_reference(diag, off, g0, R)
        h = got["h"]
        T = gltr_model.tridiag_dense(diag, off)
        q = 0.5 * h @ T @ h + g0 * h[0]
        nh = np.linalg.norm(h)
        assert q <= q_ref + 1e-10 * abs(q_ref), (idx, got["path"], q, q_ref)
        assert nh <= R * (1 + 1e-10), (idx, got["path"], nh, R)
        if got["lam"] > 0:
            assert abs(nh - R) <= 1e-10 * R, (idx, got["path"], nh, R)
            worst_norm = max(worst_norm, abs(nh - R) / R)
        else:
            assert got["case"] == 0 and got["path"] == 0
        # what the routine reports is what it returns
        assert abs(got["q"] - q) <= 1e-12 * max(abs(q), 1e-300) + 1e-300
        assert abs(got["hnorm"] - nh) <= 1e-12 * nh
        assert got["case"] == {0: 0, 1: 1, 2: 2, 3: 2}[got["path"]]
        worst_gap = max(worst_gap, (q - q_ref) / abs(q_ref))
        if idx < 600 and got["path"] in (2, 3):
            hard += 1
    print("worst model gap %.3g, worst norm error %.3g, near-hard or collapsed %d of 600"
          % (worst_gap, worst_norm, hard))
    assert hard >= 100, hard


def test_tridiagonal_solve_rejects_bad_arguments():
    from ipsolver import _hip
    lib = _hip.load()
    d = np.ones(4)
    o = np.ones(3)
    out = np.zeros(12)
    P = ctypes.c_void_p
    args = (d.ctypes.data_as(P), o.ctypes.data_as(P))
    assert lib.ipx_gltr_tridiag_host(0, *args, 1.0, 1.0, out.ctypes.data_as(P)) < 0
    assert lib.ipx_gltr_tridiag_host(257, *args, 1.0, 1.0, out.ctypes.data_as(P)) < 0
    assert lib.ipx_gltr_tridiag_host(4, *args, 0.0, 1.0, out.ctypes.data_as(P)) < 0
    assert lib.ipx_gltr_tridiag_host(4, *args, 1.0, 0.0, out.ctypes.data_as(P)) < 0
    assert lib.ipx_gltr_state_doubles(64) == 16 + 3 * 64
    assert lib.ipx_gltr_part_doubles(70001) == 2 * lib.ipx_gltr_grid(70001)


@pytest.mark.parametrize("case", sorted(gltr_cases.CASES))
def test_numpy_model_against_exact_minimiser(case):
    """The recurrence of the issue (no reorthogonalisation) at tol = 1e-24 gamma_0^2 reaches the
    exact constrained minimiser: ||x - x*|| <= 1e-10 ||x*||, model gap <= 1e-12 relative."""
    for seed in gltr_cases.SEEDS:
        H, c, A, b, radius = gltr_cases.problem(case, seed)
        _, g, _ = gltr_model._start(H, c, A, b)
        tol = 1e-24 * (g @ g)
        x, info = gltr_model.gltr(H, c, A, b, radius, tol=tol, max_vectors=256)
        xs, _, _ = gltr_model.exact_constrained(H, c, A, b, radius)
        qs, q = gltr_model.model_value(H, c, xs), gltr_model.model_value(H, c, x)
        assert np.linalg.norm(x - xs) <= 1e-10 * np.linalg.norm(xs), (case, seed, info)
        assert abs(q - qs) <= 1e-12 * abs(qs), (case, seed, q, qs)
        assert info["stop_cond"] == 4
        assert info["hits_boundary"] == (case in gltr_cases.ON_BOUNDARY)


def test_numpy_model_beats_steihaug_where_the_issue_says():
    for case in gltr_cases.GAINS:
        for seed in gltr_cases.SEEDS:
            H, c, A, b, radius = gltr_cases.problem(case, seed)
            x, _ = gltr_model.gltr(H, c, A, b, radius)
            xc, _ = gltr_model.steihaug(H, c, A, b, radius)
            q, qc = gltr_model.model_value(H, c, x), gltr_model.model_value(H, c, xc)
            assert q <= qc - 0.01 * abs(qc), (case, seed, q, qc)


# ---- option validation: raised before any device work (this file runs without a GPU) ---------
def _maratos_call(**kw):
    import ipsolver
    import problems
    p = problems.Maratos()
    options = kw.pop("options")
    return ipsolver.minimize_constrained(p.fun, p.x0, p.grad, p.hess, p.constraints(ipsolver),
                                         options=options, **kw)


def test_unknown_subproblem_is_a_value_error():
    with pytest.raises(ValueError, match="subproblem"):
        _maratos_call(options={"subproblem": "lanczos"})


@pytest.mark.parametrize("bad", [0, 257, -1, 2.5, True])
def test_gltr_max_vectors_range(bad):
    with pytest.raises(ValueError, match="max_vectors"):
        _maratos_call(options={"subproblem": "gltr", "gltr_max_vectors": bad})
    from ipsolver import qp
    with pytest.raises(ValueError, match="max_vectors"):
        qp.projected_gltr(None, None, None, None, None, 1.0, max_vectors=bad)


def test_gltr_with_the_barrier_method_is_a_value_error():
    import ipsolver
    import problems
    with pytest.raises(ValueError, match="tr_interior_point"):
        _maratos_call(options={"subproblem": "gltr"}, method="tr_interior_point")
    p = problems.HyperbolicIneq()        # method=None resolves to the barrier method here
    with pytest.raises(ValueError, match="tr_interior_point"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, p.hess, p.constraints(ipsolver),
                                      options={"subproblem": "gltr"})


def test_gltr_on_the_sharded_backend_is_not_implemented():
    with pytest.raises(NotImplementedError, match="row-sharded"):
        _maratos_call(options={"subproblem": "gltr", "shard": True})


def test_sqp_rejects_an_unknown_subproblem():
    from ipsolver import sqp
    with pytest.raises(ValueError, match="subproblem"):
        sqp.equality_constrained_sqp(None, None, None, np.zeros(2), 0.0, None, np.zeros(1), None,
                                     None, None, None, subproblem="nope")
