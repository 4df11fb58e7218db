"""The option ``sparse_rank_deficient`` (solver_options.py): its values, its place in the cache
key, ``pop_from`` / ``scoped``, the row-sharded backends' refusal -- and the conditions the GPU
tests' inputs (tests/sparse_deficient_cases.py) must meet, asserted with the numpy model of the
pivot-skipping Cholesky (tests/sparse_deficient_model.py) and the oracle's rank rule, not with the
code under test.  No GPU."""
import numpy as np
import pytest

import ipsolver
from ipsolver import projector, solver_options as so

import sparse_deficient_cases as cases
import sparse_deficient_model as model

EPS = np.finfo(float).eps


def test_values():
    assert so.SPARSE_RANK_DEFICIENT == ("host-svd", "skip-pivots")
    assert so.RANK_DEFICIENT == ("host-svd", "pivoted-qr")
    assert so.NAMES[-2:] == ("sparse_rank_deficient", "rank_deficient")
    for value in so.SPARSE_RANK_DEFICIENT:
        assert so.check("sparse_rank_deficient", value) == value
        assert projector.check_sparse_rank_deficient(value) == value
    for bad in ("svd", "pivoted-qr", None, 1, "", "skip"):
        with pytest.raises(ValueError, match="sparse_rank_deficient must be one of"):
            so.check("sparse_rank_deficient", bad)
    assert projector.SPARSE_RANK_DEFICIENT is so.SPARSE_RANK_DEFICIENT
    assert projector.sparse_rank_deficient_choice() == "host-svd"


# every key that existed before the option, as the parent commit forms it
KEYS_BEFORE = [
    ({}, ("iterative", 0, 0)),
    ({"wide_band": "block-tridiagonal-wide", "border_columns": 3, "link_rows": 2},
     ("block-tridiagonal-wide", 3, 2)),
    ({"iterative_precond": "two-level"}, ("iterative", 0, 0, "two-level")),
    ({"sparse_direct": "nested-dissection"}, ("iterative", 0, 0, "nested-dissection")),
    ({"dense_factorization": "householder-qr"}, ("iterative", 0, 0, "householder-qr")),
    ({"rank_deficient": "pivoted-qr"}, ("iterative", 0, 0, "pivoted-qr")),
    ({"iterative_precond": "compact", "sparse_direct": "nested-dissection", "link_rows": 1,
      "dense_factorization": "householder-qr", "rank_deficient": "pivoted-qr"},
     ("iterative", 0, 1, "compact", "nested-dissection", "householder-qr", "pivoted-qr")),
]


@pytest.mark.parametrize("changes,key", KEYS_BEFORE)
def test_key_unchanged_under_the_default(changes, key):
    assert so.current().sparse_rank_deficient == "host-svd"
    with so.scoped(**changes):
        assert so.current().key() == key
        with so.scoped(sparse_rank_deficient="host-svd"):
            assert so.current().key() == key
        with so.scoped(sparse_rank_deficient="skip-pivots"):
            assert so.current().key() == key + ("skip-pivots",)
        assert so.current().key() == key


def test_pop_from_and_scoped():
    assert "sparse_rank_deficient" not in so.pop_from({"xtol": 1e-9})
    options = {"sparse_rank_deficient": "skip-pivots", "xtol": 1e-9}
    held = so.pop_from(options)
    assert options == {"xtol": 1e-9} and held["sparse_rank_deficient"] == "skip-pivots"
    assert "rank_deficient" not in held and "sparse_direct" not in held
    with pytest.raises(ValueError, match="sparse_rank_deficient must be one of"):
        so.pop_from({"sparse_rank_deficient": "device"})
    with projector.sparse_rank_deficient("skip-pivots"):
        assert projector.sparse_rank_deficient_choice() == "skip-pivots"
        assert "sparse_rank_deficient" not in so.pop_from({})
        with so.scoped(**so.pop_from({})):
            assert so.current().sparse_rank_deficient == "skip-pivots"
        # the options beside the tuple survive a change of another one
        with so.scoped(link_rows=1, rank_deficient="pivoted-qr"):
            cur = so.current()
            assert (cur.sparse_rank_deficient, cur.rank_deficient, cur.link_rows) == \
                ("skip-pivots", "pivoted-qr", 1)
    assert projector.sparse_rank_deficient_choice() == "host-svd"
    with pytest.raises(RuntimeError, match="inside"):
        with so.scoped(sparse_rank_deficient="skip-pivots"):
            raise RuntimeError("inside")
    assert so.current().sparse_rank_deficient == "host-svd"
    assert so.current().key() == ("iterative", 0, 0)


def test_row_sharded_backend_refuses_the_option():
    import problems
    p = problems.Maratos()
    with pytest.raises(NotImplementedError, match="sparse_rank_deficient='skip-pivots': the "
                                                  "row-sharded backend builds its"):
        ipsolver.minimize_constrained(
            p.fun, p.x0, p.grad, p.hess, p.constraints(ipsolver),
            options={"shard": True, "sparse_rank_deficient": "skip-pivots"})
    assert so.current().sparse_rank_deficient == "host-svd"


# ---------------------------------------------------------------- the inputs of the GPU tests
def test_the_search_found_every_position():
    """The skipped pivot at every wanted place of the elimination order, by the model."""
    lds, tiled = cases.lds_position_cases(), cases.tiled_position_cases()
    assert sorted(lds) == ["last-own-row", "leaf-front", "separator-front", "two-in-one-front"]
    assert sorted(tiled) == ["tile-15", "tile-16", "tile-63", "tile-64", "tile-last"]

    def where(name):
        _, _, small, sym, mod = cases.built(name)
        out = model.positions(sym, mod)
        for j, _, s, _ in out:
            large = small is not None and s + int(sym.boundary[j]) > small
            assert large == name.startswith("tile"), (name, j)
        return out
    (_, p, s, level), = where("lds-last-own-row")
    assert p == s - 1 and s > 1
    (_, p, s, level), = where("lds-leaf-front")
    assert level == 0 and 0 < p < s - 1
    (_, p, s, level), = where("lds-separator-front")
    assert level > 0 and 0 < p < s - 1
    (j1, p1, _, _), (j2, p2, _, _) = where("lds-two-in-one-front")
    assert j1 == j2 and p1 != p2
    for want in cases.TILED_POSITIONS[1:]:
        (_, p, s, level), = where("tile-%s" % want)
        assert level == 0 and 65 <= s <= 128 and p == (s - 1 if want == "last" else want)
    # the first own row of a front: zero rows, on either path (sparse_deficient_cases.py says why
    # nothing else lands there)
    for name in ("two-zero-rows", "tile-0"):
        assert [(p, s) for _, p, s, _ in where(name)] == [(0, 1), (0, 1)]


@pytest.mark.parametrize("name", sorted(cases.all_cases()))
def test_case_conditions(name):
    """Kept pivots >= 2^-30 of their diagonal entry, dropped ones <= 2^-46 (the margin to 2^-43
    covers the device's other summation order); the oracle works with the rank m - q; the model's
    operators are the oracle's."""
    A, _, _, sym, mod = cases.built(name)
    m, n = A.shape
    q = len(mod.dropped)
    print("%s: m %d q %d, kept >= 2^%.1f, dropped <= 2^%.1f"
          % (name, m, q, np.log2(mod.kept_ratio),
             np.log2(mod.dropped_ratio) if mod.dropped_ratio > 0 else -np.inf))
    assert 1 <= q <= 32
    assert mod.kept_ratio >= 2.0 ** -30
    assert mod.dropped_ratio <= 2.0 ** -46
    assert cases.oracle_rank(A) == m - q == mod.rank
    assert np.linalg.matrix_rank(A[mod.kept].toarray()) == m - q
    Zo, LSo, Yo = cases.oracle_svd_operators(A)
    Z, LS, Y = mod.operators()
    rng = np.random.default_rng(m + n)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    kappa = max(cases.conditions(A, mod.kept))
    for op, ref, v in ((Z, Zo, x), (LS, LSo, x), (Y, Yo, b)):
        want = ref.dot(v)
        assert np.max(np.abs(op(v) - want)) <= 50 * kappa * EPS * np.max(np.abs(want))


def test_fallback_case_has_more_dropped_rows_than_the_cap():
    A = cases.thinned_g()
    mod = model.SkippingCholesky(A, model.analysis(A, 32).perm)
    assert len(mod.dropped) == 49 > 32
    assert cases.oracle_rank(A) == A.shape[0] - 49
