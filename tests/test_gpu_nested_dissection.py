"""The nested-dissection direct (A A')^-1 (csrc/nested.hip, ipsolver/nested.py): assembly exact,
every solve judged by an exact residual (tests/normal_ref.py) on both front paths, a forest, a
general pattern, bit identity, a refactorization, the pivot signals, and the public calls under
``sparse_direct="nested-dissection"``.

Inputs.  ``A = diag(2^e) [8 G, I]``, G with entries +-1 and e = -3 throughout (``[G, 2^-3 I]``) or
-3 + {-8 ... 8} per row: S is exact and below 26 bits, so ``normal_ref.backward_error`` evaluates
the residual exactly.

Bound (u = 2^-53).  The yardstick is a host factorization of the same S for the same w: LAPACK's
Cholesky of the dense S up to m = 2304, SuperLU (``scipy.sparse.linalg.splu``) beyond, judged by
the same eta.  The device may exceed max(host eta, u) by the factor C_ND, which allows for the
other elimination and summation orders.  The largest eta / max(host eta, u) these tests printed
on an MI355X is MEASURED_RATIO below; C_ND is that with a margin of 5 (C_DIRECT, C_BLOCK: margins
of 4 - 6).
"""
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps
import scipy.sparse.linalg

import nested_model as nm
import normal_ref as nr
import two_level_cases as tc

pytestmark = pytest.mark.gpu

U = nr.U
MEASURED_RATIO = 1.58         # the N = 12 grid: 1.58 u against LAPACK's 0.98 u; every other case
C_ND = 8.0                    # of this file stays below 1.2.  C_ND is that with a margin of 5.
HOT_PATH_RTOL = 1e-10
DENSE_YARDSTICK_ROWS = 2304
OPTION = {"sparse_direct": "nested-dissection"}


def integer_rows(A):
    """[8 G, I] of a matrix [G, 2^-3 I] (integers), so that ``pow2_rows(., -3)`` is A exactly."""
    Ai = sps.csr_matrix(A * 8.0)
    assert np.array_equal(Ai.data, np.round(Ai.data))
    return Ai


# name -> (matrix [G, 2^-3 I], LEAF, SMALL_FRONT or None, graded rows)
CASES = {
    "grid6": (lambda: tc.grid(6, 0.125), 64, None, False),         # one front, no boundary
    "grid12": (lambda: tc.grid(12, 0.125), 32, None, False),
    "grid48": (lambda: tc.grid(48, 0.125), 32, None, False),
    "grid48-graded": (lambda: tc.grid(48, 0.125), 32, None, True),
    "grid48-tiled": (lambda: tc.grid(48, 0.125), 32, 32, False),
    "grid48-tiled-graded": (lambda: tc.grid(48, 0.125), 32, 32, True),
    "grid100": (lambda: tc.grid(100, 0.125), 64, None, False),
    "thinned": (lambda: tc.thinned_grid(eps=0.125), 32, None, False),
    "random": (nm.random_sparse, 32, None, False),
    "random-graded": (nm.random_sparse, 32, None, True),
}


def solver_class(leaf, small=None):
    from ipsolver.nested import NestedDissectionNormalSolver
    attrs = {"LEAF": leaf}
    if small is not None:
        attrs["SMALL_FRONT"] = small
    return type("Cut", (NestedDissectionNormalSolver,), attrs)


@functools.lru_cache(maxsize=None)
def system(name):
    """(A_int, e, S exact, w, host eta) of a case, computed once."""
    build, _, _, graded = CASES[name]
    Ai = integer_rows(build())
    m = Ai.shape[0]
    rng = np.random.default_rng(len(name))
    e = np.full(m, -3, np.int64)
    if graded:
        e += rng.integers(-8, 9, m)
    S = nr.gram_pow2(Ai, e)
    w = rng.standard_normal(m)
    if m <= DENSE_YARDSTICK_ROWS:
        x = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S.toarray(), lower=True), w)
    else:
        x = scipy.sparse.linalg.splu(sps.csc_matrix(S)).solve(w)
    return Ai, e, S, w, nr.backward_error(S, x, w)


def build_solver(name):
    import ipsolver.device as dv
    Ai, e, _, _, _ = system(name)
    _, leaf, small, _ = CASES[name]
    return solver_class(leaf, small)(dv.DeviceCSR.from_scipy(nr.pow2_rows(Ai, e)))


def check_eta(name, x, S, w, host):
    eta = nr.backward_error(S, x, w)
    ratio = eta / max(host, U)
    print("eta/u %-20s device %.3g  host %.3g  ratio %.3g" % (name, eta / U, host / U, ratio))
    assert ratio <= C_ND, (name, eta / U, host / U)


# ------------------------------------------------------------------------------ 1. assembly
@pytest.mark.parametrize("small", [None, 32])
def test_assembled_leaf_fronts_are_the_entries_of_s(small):
    """Level 0 (no children) assembled and not factored, on the integer rows [8 G, I]: the own
    columns of every front are the entries of S bit for bit, the update block is zero, a tiled
    front carries its unit diagonal between the own and the boundary rows."""
    import ipsolver.device as dv
    Ai = integer_rows(tc.grid(48, 0.125))
    S = nr.gram_pow2(Ai).toarray()
    solver = solver_class(32, small)(dv.DeviceCSR.from_scipy(Ai))
    sym, plan = solver.symbolic, solver.plan
    solver.assemble_level(0)
    leaves = np.flatnonzero(sym.level == 0)
    tiled = 0
    for j in leaves:
        s, b, ld, pad = (int(plan.sn[j, k]) for k in (1, 2, 5, 6))
        F = solver.front(j)
        own = sym.perm[sym.sn_ptr[j]:sym.sn_ptr[j + 1]]
        rows = np.concatenate((own, sym.perm[sym.bnd[sym.bnd_ptr[j]:sym.bnd_ptr[j + 1]]]))
        at = np.concatenate((np.arange(s), s + pad + np.arange(b)))       # storage rows
        want = np.zeros((ld, ld))
        want[np.ix_(at, at[:s])] = S[np.ix_(rows, own)]
        want[s:s + pad, s:s + pad] = np.eye(pad)
        assert np.array_equal(np.tril(F), np.tril(want)), j
        tiled += pad > 0 or ld != s + b
    assert (tiled > 0) == (small is not None) and len(leaves) > 50
    if small is not None:
        # (a tiled front whose own rows are no multiple of 64)
        assert any(plan.sn[j, 1] % 64 for j in leaves if plan.sn[j, 1] + plan.sn[j, 2] > small)


# ------------------------------------------------------------------------------ 2. solves
@pytest.mark.parametrize("name", sorted(CASES))
def test_solve_by_exact_residual(name):
    import ipsolver.device as dv
    _, _, S, w, host = system(name)
    solver = build_solver(name)
    assert solver.flag_bits == 0 and not solver.ill_conditioned
    st = solver.stats
    print("%s: %r" % (name, st))
    if name == "grid6":
        assert (st["fronts"], st["levels"], st["largest_front"]) == (1, 1, 36)
    if name.startswith("grid48"):
        assert (st["largest_front"], st["levels"]) == (72, 7)
        assert (st["large_fronts"] > 0) == ("tiled" in name)
    if name == "grid100":
        assert st["largest_front"] == 150 and 0 < st["large_fronts"] <= 8
    if name == "thinned":
        assert int((solver.symbolic.parent < 0).sum()) > 1            # a forest
    if name.startswith("random"):
        assert st["largest_front"] > 128 and st["large_fronts"] > 0
    x = solver.solve(dv.DVec.from_host(w)).to_host()
    assert st["solves"] == 1 and st["launches_per_solve"] == 2 * st["levels"]
    check_eta(name, x, S, w, host)


def test_both_paths_agree_within_the_bound():
    """No bit identity is claimed between the LDS path and the tiled path (other summation orders
    in the trailing update): both are within the bound above, and close to each other."""
    import ipsolver.device as dv
    _, _, S, w, _ = system("grid48")
    xs = [build_solver(n).solve(dv.DVec.from_host(w)).to_host() for n in ("grid48", "grid48-tiled")]
    diff = np.max(np.abs(xs[0] - xs[1])) / np.max(np.abs(xs[0]))
    print("LDS path against tiled path: %.3g" % diff)
    assert diff <= HOT_PATH_RTOL


# ------------------------------------------------------------------------------ 3. bit identity
@pytest.mark.parametrize("name", ["grid48", "grid48-tiled", "random"])
def test_factorization_and_solve_are_deterministic(name):
    import ipsolver.device as dv
    import torch
    _, _, _, w, _ = system(name)
    one, two = build_solver(name), build_solver(name)
    assert one.symbolic is not two.symbolic            # (two patterns, two analyses, same tables)
    assert torch.equal(one.ws, two.ws)
    wd = dv.DVec.from_host(w)
    x1, x2, x3 = one.solve(wd).to_host(), one.solve(wd).to_host(), two.solve(wd).to_host()
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3)


# ------------------------------------------------------------------------------ 4. refactorization
def test_refactorization_does_no_graph_work(monkeypatch):
    import ipsolver.device as dv
    from ipsolver import nested
    calls = []
    real = nested._analyze

    def spy(pattern, leaf):
        calls.append(leaf)
        return real(pattern, leaf)
    monkeypatch.setattr(nested, "_analyze", spy)
    Ai, e, _, w, _ = system("grid48")
    cls = solver_class(32)
    Ad = dv.DeviceCSR.from_scipy(nr.pow2_rows(Ai, e))     # (a pattern nothing is cached on)
    first = cls(Ad)
    assert calls == [32]
    e2 = e + np.random.default_rng(8).integers(-8, 9, len(e))
    A2 = nr.pow2_rows(Ai, e2)
    second = cls(dv.DeviceCSR(Ad.pattern, dv.DVec.from_host(A2.data).t))
    assert calls == [32]
    assert second.symbolic is first.symbolic and second.plan is first.plan
    S2 = nr.gram_pow2(Ai, e2)
    x = second.solve(dv.DVec.from_host(w)).to_host()
    host = nr.backward_error(
        S2, scipy.linalg.cho_solve(scipy.linalg.cho_factor(S2.toarray(), lower=True), w), w)
    check_eta("refactorization", x, S2, w, host)


# ------------------------------------------------------------------------------ 5. pivot signals
def _with_two_more_rows(private):
    """The N = 12 flow rows [8 G, I] and, on two columns of their own, the rows (2, 0) and
    (2, private): a connected piece of its own, one supernode with S = [[4, 4], [4, 4 + p^2]]."""
    Ai = integer_rows(tc.grid(12, 0.125))
    pair = sps.csr_matrix(np.array([[2.0, 0.0], [2.0, private]]))
    A = sps.bmat([[Ai, None], [None, pair]], format="csr")
    A.eliminate_zeros()
    A.sort_indices()
    return A


def test_duplicated_row_is_refused():
    """Rows (2, 0) and (2, 0): the first pivot is 4, its root 2 and the quotient 4 / 2 are exact,
    so the second pivot is 4 - 2 * 2 = 0 exactly: not positive, LinAlgError.  The same through
    ``projections``: the SVD exit with the reference's warning."""
    import ipsolver.device as dv
    import ipsolver.projector as projector
    A = _with_two_more_rows(0.0)
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        solver_class(64)(dv.DeviceCSR.from_scipy(A))
    with projector.sparse_direct("nested-dissection"):
        with pytest.warns(UserWarning, match="Singular Jacobian"):
            Z, _, _ = projector.projections(dv.DeviceCSR.from_scipy(A))
    assert isinstance(Z.projector, projector.SVDProjector)


def test_nearly_duplicated_row_is_ill_conditioned():
    """Rows (2, 0) and (2, 2^-24): the second pivot is 2^-48 exactly, 2^-50 of its diagonal entry
    4 + 2^-48 and so below 2^-43 of it: positive, ``ill_conditioned``, no exception.  (A shift of
    2^-30 as in the first sketch of this test cannot be held: 4 + 2^-60 is not an fp64 number, S
    itself would be singular and the case the one above.  2^-24 is within a factor 4 of the
    largest shift whose pivot still loses 43 bits while S stays exact.)"""
    import ipsolver.device as dv
    solver = solver_class(64)(dv.DeviceCSR.from_scipy(_with_two_more_rows(2.0 ** -24)))
    assert solver.flag_bits == 1 and solver.ill_conditioned
    w = np.zeros(solver.m)
    w[:144] = np.random.default_rng(2).standard_normal(144)
    x = solver.solve(dv.DVec.from_host(w)).to_host()
    assert np.all(np.isfinite(x)) and np.array_equal(x[144:], [0.0, 0.0])


# ------------------------------------------------------------------------------ 6. public calls
def test_projections_under_the_option():
    """Z, LS, Y at N = 48 against a dense host computation."""
    import ipsolver.device as dv
    import ipsolver.projector as projector
    A = tc.grid(48, 0.125)
    Ad = dv.DeviceCSR.from_scipy(A)
    with projector.sparse_direct("nested-dissection"):
        Z, LS, Y = projector.projections(Ad)
    assert projector.last_normal_solver() == "NestedDissectionNormalSolver"
    assert projector.solver_name(Z.projector.solver) == "NestedDissectionNormalSolver"
    Z0, _, _ = projector.projections(dv.DeviceCSR.from_scipy(A))
    assert projector.last_normal_solver() == "DenseNormalSolver"        # as without the option
    assert projector.sparse_direct_choice() == "off"
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    Sinv = np.linalg.inv(A.dot(A.T).toarray())
    want = (x - A.T.dot(Sinv.dot(A.dot(x))), Sinv.dot(A.dot(x)), A.T.dot(Sinv.dot(y)))
    for name, op, v, ref in zip("Z LS Y".split(), (Z, LS, Y), (x, x, y), want):
        got = op.dot(dv.DVec.from_host(v)).to_host()
        err = np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(ref)))
        print("projections under the option: %s %.2e" % (name, err))
        assert err <= HOT_PATH_RTOL


def _flow_qp(N, seed):
    A = tc.grid(N, 0.125)
    n = A.shape[1]
    rng = np.random.default_rng(seed)
    return A, rng.standard_normal(n), A.dot(rng.standard_normal(n))


def test_equality_constrained_problem_through_minimize_constrained():
    """min 1/2 ||x||^2 + c'x subject to the flow balance rows of the N = 48 network, against the
    dense KKT solve."""
    import ipsolver
    from ipsolver import solver_options
    A, c, b = _flow_qp(48, 11)
    n = A.shape[1]
    lam = np.linalg.solve(A.dot(A.T).toarray(), -(b + A.dot(c)))
    x_kkt = -c - A.T.dot(lam)
    H = sps.identity(n, format="csr")
    gtol = 1e-8

    def run(**options):
        return ipsolver.minimize_constrained(
            lambda x: 0.5 * x.dot(x) + c.dot(x), np.zeros(n), lambda x: x + c, lambda x: H,
            ipsolver.LinearConstraint(A, ("equals", b)), gtol=gtol, options=options)

    res = run(**OPTION)
    assert res.normal_solver == "NestedDissectionNormalSolver"
    assert solver_options.current().sparse_direct == "off"             # gone after the call
    assert res.constr_violation <= gtol and res.optimality <= gtol
    rel = lambda a, want: np.linalg.norm(a - want) / np.linalg.norm(want)
    print("nested dissection: x against the KKT solve %.2e, %d iterations"
          % (rel(res.x, x_kkt), res.niter))
    assert rel(res.x, x_kkt) <= 1e-6
    res0 = run()
    assert res0.normal_solver == "DenseNormalSolver"                   # what it reports today
    assert rel(res0.x, x_kkt) <= 1e-6


def test_barrier_problem_with_a_box(monkeypatch):
    """The same rows with a box on every variable, the dense Cholesky out of reach as for
    m > 16384: the box-Schur elimination keeps the bound rows, its inner solver is the
    nested-dissection solver under the option and the preconditioned CG without it; the same
    solution to the tolerance the two-level test holds its runs to."""
    import ipsolver
    from ipsolver.dense import DenseNormalSolver
    A, c, b = _flow_qp(24, 12)
    n = A.shape[1]
    H = sps.identity(n, format="csr")
    monkeypatch.setattr(DenseNormalSolver, "MAX_ROWS_FROM_SPARSE", 0)
    gtol = 1e-8

    def run(**options):
        return ipsolver.minimize_constrained(
            lambda x: 0.5 * x.dot(x) + c.dot(x), np.zeros(n), lambda x: x + c, lambda x: H,
            [ipsolver.LinearConstraint(A, ("equals", b)),
             ipsolver.BoxConstraint(("interval", -4.0, 4.0))], gtol=gtol, options=options)

    res = run(**OPTION)
    assert res.normal_solver == "BoxSchurNormalSolver/NestedDissectionNormalSolver"
    res0 = run()
    assert res0.normal_solver == "BoxSchurNormalSolver/IterativeNormalSolver"
    for r in (res, res0):
        assert r.status in (1, 2) and r.constr_violation <= gtol
    rel = np.linalg.norm(res.x - res0.x) / np.linalg.norm(res0.x)
    print("barrier problem with a box: with the option against without %.2e (%d / %d iterations)"
          % (rel, res.niter, res0.niter))
    assert rel <= 1e-6
