"""The aggregate-block ("compact") and two-level preconditioners of ``IterativeNormalSolver``
(ipsolver/iterative.py, csrc/pcg.hip) on the flow matrices of two_level_cases.py, against the
numpy model (two_level_model.py): the coarse matrix, one application of the preconditioner, the
iteration counts, the accuracy of the solve, a refactorization, and the option
``iterative_precond`` through ``minimize_constrained`` and the box-Schur elimination.

Iteration counts of the model (plain PCG to 1e-12, right-hand side ``rhs(m)``): two-level 63 / 70
/ 71 at N = 24 / 48 / 64, flat in m; "compact" 129 at N = 48; N = 64 with 36 coarse rows (groups
of 4 blocks) 98.  A device count moves by one or two with the summation order: the margin of
10 % + 2 below.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import two_level_cases as tc
import two_level_model as tm

pytestmark = pytest.mark.gpu

HOT_PATH_RTOL = 1e-10


@functools.lru_cache(maxsize=None)
def matrix(name, N):
    return tc.thinned_grid(N) if name == "thinned" else tc.grid(N)


@functools.lru_cache(maxsize=None)
def device_matrix(name, N):
    import ipsolver.device as dv
    return dv.DeviceCSR.from_scipy(matrix(name, N))


def solver_for(name, N, precond, coarse_max=None, rtol=None):
    """A solver on a pattern of its own copy when ``coarse_max`` is given (the class attribute is
    read at construction)."""
    from ipsolver.iterative import IterativeNormalSolver
    cls = IterativeNormalSolver if coarse_max is None else \
        type("Grouped", (IterativeNormalSolver,), {"COARSE_MAX": coarse_max})
    solver = cls(device_matrix(name, N), precond=precond)
    if rtol is not None:
        solver.RTOL = rtol
    return solver


@functools.lru_cache(maxsize=None)
def model(name, N, coarse_max=4096):
    A = matrix(name, N)
    ag = tm.Aggregation(A, coarse_max)
    return A, ag, tm.preconditioner(A, ag), tm.preconditioner(A, ag, two_level=False)


@functools.lru_cache(maxsize=None)
def model_count(N, precond, coarse_max=4096):
    A, _, two, compact = model("grid", N, coarse_max)
    return tm.pcg(A, tc.rhs(N * N), two if precond == "two-level" else compact, 1e-12)[1]


@functools.lru_cache(maxsize=None)
def device_count(N, precond, coarse_max=None):
    import ipsolver.device as dv
    solver = solver_for("grid", N, precond, coarse_max, rtol=1e-12)
    solver.solve(dv.DVec.from_host(tc.rhs(N * N)))
    print("N = %d %s coarse_max %s: %d iterations, stats %r"
          % (N, precond, coarse_max, solver.stats["iterations"], solver.stats))
    return solver.stats["iterations"]


def within_margin(got, want):
    return abs(got - want) <= 0.1 * want + 2


def test_coarse_matrix():
    """C = P'A from ipx_csr_aggregate_rows: sums of at most 32 terms."""
    solver = solver_for("grid", 24, "two-level")
    A, ag, _, _ = model("grid", 24)
    want = sps.csr_matrix(ag.P.T.dot(A))
    got = solver.C.to_scipy()
    assert got.shape == want.shape == (ag.ncoarse, A.shape[1])
    assert solver.stats["blocks"] == ag.nblk and solver.stats["coarse_rows"] == ag.ncoarse
    assert solver.stats["group"] == 1
    err = abs(got - want).max() / abs(want).max()
    print("coarse matrix: relative error %.2e" % err)
    assert err <= HOT_PATH_RTOL
    # the stored pattern is the union of the member rows' columns: nothing outside it is lost
    assert abs(want).sum() - abs(got).sum() <= HOT_PATH_RTOL * abs(want).sum()


@pytest.mark.parametrize("N,coarse_max,group", [(24, None, 1), (48, 20, 4)])
def test_preconditioner_application(N, coarse_max, group):
    import ipsolver.device as dv
    solver = solver_for("grid", N, "two-level", coarse_max)
    assert solver.stats["group"] == group
    _, ag, apply_M, _ = model("grid", N, coarse_max or 4096)
    assert solver.stats["coarse_rows"] == ag.ncoarse
    rng = np.random.default_rng(5)
    for k in range(10):
        r = rng.standard_normal(N * N)
        z, rz = solver.precond_apply(dv.DVec.from_host(r))
        want = apply_M(r)
        errz = np.max(np.abs(z.to_host() - want)) / np.max(np.abs(want))
        errrz = abs(rz - r.dot(want)) / abs(r.dot(want))
        print("apply %d: z %.2e  r'z %.2e (r'z = %.6e)" % (k, errz, errrz, rz))
        assert errz <= HOT_PATH_RTOL and errrz <= HOT_PATH_RTOL
        assert rz > 0                    # a symmetric positive definite preconditioner


def test_iteration_counts_against_block():
    """Two-level at N = 48 takes at most half of what "block" takes on the same matrix (the model:
    70 against 248)."""
    assert device_count(48, "two-level") <= 0.5 * device_count(48, "block")


def test_iteration_counts_are_flat_in_m():
    """(the model: 71 at N = 64 against 63 at N = 24, while "block" grows 2.85 x)"""
    assert device_count(64, "two-level") <= 1.3 * device_count(24, "two-level")


@pytest.mark.parametrize("N,precond", [(24, "two-level"), (48, "two-level"), (64, "two-level"),
                                       (48, "compact")])
def test_iteration_counts_against_the_model(N, precond):
    assert within_margin(device_count(N, precond), model_count(N, precond))


def test_iteration_counts_with_grouped_blocks():
    """N = 64 with COARSE_MAX = 40: 135 blocks in groups of at most 4, 36 coarse rows."""
    _, ag, _, _ = model("grid", 64, 40)
    assert (ag.nblk, ag.group, ag.ncoarse) == (135, 4, 36)
    got = device_count(64, "two-level", 40)
    assert within_margin(got, model_count(64, "two-level", 40))
    assert got < device_count(64, "compact")


@pytest.mark.parametrize("name,N", [("grid", 24), ("grid", 48), ("thinned", 64)])
@pytest.mark.parametrize("precond", ["two-level", "compact"])
def test_solve_accuracy(name, N, precond):
    """The true residual under the rule test_gpu_normal_solve.py uses for the CG, at the class's
    own RTOL."""
    import ipsolver.device as dv
    A = matrix(name, N)
    solver = solver_for(name, N, precond)
    w = tc.rhs(A.shape[0])
    v = solver.solve(dv.DVec.from_host(w)).to_host()
    res = np.linalg.norm(w - A.dot(A.T.dot(v))) / np.linalg.norm(w)
    print("%s N = %d %s: true residual %.2e, stats %r" % (name, N, precond, res, solver.stats))
    assert res <= solver.WARN_RELRES
    assert not solver.ill_conditioned


def test_refactorization_does_no_graph_work(monkeypatch):
    """The same pattern with new values: the aggregation, the padded order and the pattern of C
    are the pattern's."""
    import ipsolver.device as dv
    from ipsolver import iterative
    calls = []
    real = iterative._aggregate_greedy

    def spy(indptr, indices, cap):
        calls.append(cap)
        return real(indptr, indices, cap)
    monkeypatch.setattr(iterative, "_aggregate_greedy", spy)
    A = matrix("grid", 48)
    Ad = dv.DeviceCSR.from_scipy(A)                      # (a pattern nothing is cached on)
    cls = type("Grouped", (iterative.IterativeNormalSolver,), {"COARSE_MAX": 20})
    first = cls(Ad, precond="two-level")
    assert calls == [32, 4]
    A2 = A.copy()
    A2.data *= 1.0 + 0.25 * np.random.default_rng(3).random(A.nnz)
    Ad2 = dv.DeviceCSR(Ad.pattern, dv.DVec.from_host(A2.data).t)
    second = cls(Ad2, precond="two-level")
    assert calls == [32, 4]
    assert second.aggregation is first.aggregation and second.border is first.border
    assert second.C.pattern is first.C.pattern
    w = tc.rhs(A.shape[0])
    v = second.solve(dv.DVec.from_host(w)).to_host()
    res = np.linalg.norm(w - A2.dot(A2.T.dot(v))) / np.linalg.norm(w)
    assert res <= second.WARN_RELRES
    want = sps.csr_matrix(tm.Aggregation(A, 20).P.T.dot(A2))
    assert abs(second.C.to_scipy() - want).max() <= HOT_PATH_RTOL * abs(want).max()


def test_option_through_minimize_constrained(monkeypatch):
    """An equality-constrained QP over the N = 48 flow network, min 1/2 ||x||^2 + c'x subject to
    the balance rows, with the dense Cholesky out of reach as for m > 16384."""
    import ipsolver
    import ipsolver.projector as projector
    from ipsolver import solver_options
    from ipsolver.dense import DenseNormalSolver
    A = matrix("grid", 48)
    m, n = A.shape
    rng = np.random.default_rng(11)
    c, b = rng.standard_normal(n), A.dot(rng.standard_normal(n))
    # KKT: x = -c - A'lam, A x = b
    lam = np.linalg.solve(A.dot(A.T).toarray(), -(b + A.dot(c)))
    x_kkt = -c - A.T.dot(lam)
    monkeypatch.setattr(DenseNormalSolver, "MAX_ROWS_FROM_SPARSE", m - 1)
    used = []
    real = projector.normal_solver_for

    def spy(*args, **kw):
        used.append(real(*args, **kw))
        return used[-1]
    monkeypatch.setattr(projector, "normal_solver_for", spy)
    H = sps.identity(n, format="csr")
    gtol = 1e-8

    def run(**options):
        del used[:]
        res = ipsolver.minimize_constrained(
            lambda x: 0.5 * x.dot(x) + c.dot(x), np.zeros(n), lambda x: x + c, lambda x: H,
            ipsolver.LinearConstraint(A, ("equals", b)), gtol=gtol, options=options)
        return res, list(used)

    res, solvers = run(iterative_precond="two-level")
    assert res.normal_solver == "IterativeNormalSolver"
    assert solvers and all(s.precond == "two-level" for s in solvers)
    assert solver_options.current().iterative_precond == "block"      # gone after the call
    assert res.constr_violation <= gtol and res.optimality <= gtol
    rel = lambda a, want: np.linalg.norm(a - want) / np.linalg.norm(want)
    print("two-level: x against the KKT solve %.2e, %d iterations" % (rel(res.x, x_kkt), res.niter))
    assert rel(res.x, x_kkt) <= 1e-6
    res0, solvers0 = run()
    assert res0.normal_solver == "IterativeNormalSolver"
    assert solvers0 and all(s.precond == "block" for s in solvers0)
    assert res0.constr_violation <= gtol and res0.optimality <= gtol
    assert rel(res.x, res0.x) <= 1e-6


def test_box_schur_inner_solver_honours_the_option(monkeypatch):
    """A barrier Jacobian over the flow network's incidence rows: the box-Schur elimination leaves
    the general rows' Schur complement to an iterative inner solver, two-level under the option."""
    import selection_cases as sc
    import ipsolver.device as dv
    import ipsolver.projector as projector
    from ipsolver.dense import DenseNormalSolver
    N = 24
    G = matrix("grid", N)[:, :2 * N * (N - 1)]
    A = sc.barrier_jacobian(G, np.random.default_rng(2))
    monkeypatch.setattr(DenseNormalSolver, "MAX_ROWS_FROM_SPARSE", 0)
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    outs = {}
    for precond in ("block", "two-level"):
        Ad = dv.DeviceCSR.from_scipy(A)
        with projector.iterative_precond(precond):
            Z, LS, Y = projector.projections(Ad)
        solver = Z.projector.solver
        assert projector.solver_name(solver) == "BoxSchurNormalSolver/IterativeNormalSolver"
        assert solver.inner.precond == precond
        outs[precond] = [op.dot(dv.DVec.from_host(v)).to_host()
                         for op, v in ((Z, x), (LS, x), (Y, y))]
    for got, want in zip(outs["two-level"], outs["block"]):
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("box-Schur projection: %.2e" % err)
        assert err <= 1e-9
