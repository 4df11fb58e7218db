"""The option ``rank_deficient`` (solver_options.py): its values, its place in the cache key,
``pop_from`` / ``scoped``, the row-sharded backends' refusal -- and the conditions the GPU tests'
inputs (tests/rank_deficient_cases.py) must meet, asserted with scipy's pivoted QR and the
oracle's rank rule.  No GPU."""
import numpy as np
import pytest
import scipy.linalg

import ipsolver
from ipsolver import projector, solver_options as so

import rank_deficient_cases as cases


def test_values():
    assert so.RANK_DEFICIENT == ("host-svd", "pivoted-qr")
    assert so.NAMES[-1] == "rank_deficient"
    assert so.DENSE_FACTORIZATIONS == ("normal-equations", "householder-qr")
    for value in so.RANK_DEFICIENT:
        assert so.check("rank_deficient", value) == value
        assert projector.check_rank_deficient(value) == value
    for bad in ("svd", "qr", None, 1, "", "householder-qr"):
        with pytest.raises(ValueError, match="rank_deficient must be one of"):
            so.check("rank_deficient", bad)
    assert projector.RANK_DEFICIENT is so.RANK_DEFICIENT
    assert projector.rank_deficient_choice() == "host-svd"


# every key that existed before the option, as the parent commit forms it
KEYS_BEFORE = [
    ({}, ("iterative", 0, 0)),
    ({"wide_band": "block-tridiagonal-wide", "border_columns": 3, "link_rows": 2},
     ("block-tridiagonal-wide", 3, 2)),
    ({"iterative_precond": "two-level"}, ("iterative", 0, 0, "two-level")),
    ({"sparse_direct": "nested-dissection"}, ("iterative", 0, 0, "nested-dissection")),
    ({"dense_factorization": "householder-qr"}, ("iterative", 0, 0, "householder-qr")),
    ({"iterative_precond": "compact", "sparse_direct": "nested-dissection", "link_rows": 1,
      "dense_factorization": "householder-qr"},
     ("iterative", 0, 1, "compact", "nested-dissection", "householder-qr")),
]


@pytest.mark.parametrize("changes,key", KEYS_BEFORE)
def test_key_unchanged_under_the_default(changes, key):
    assert so.current().rank_deficient == "host-svd"
    with so.scoped(**changes):
        assert so.current().key() == key
        with so.scoped(rank_deficient="host-svd"):
            assert so.current().key() == key
        with so.scoped(rank_deficient="pivoted-qr"):
            assert so.current().key() == key + ("pivoted-qr",)
        assert so.current().key() == key


def test_pop_from_and_scoped():
    assert "rank_deficient" not in so.pop_from({"xtol": 1e-9})
    untouched = {"xtol": 1e-9}
    so.pop_from(untouched)
    assert untouched == {"xtol": 1e-9}
    options = {"rank_deficient": "pivoted-qr", "xtol": 1e-9}
    held = so.pop_from(options)
    assert options == {"xtol": 1e-9} and held["rank_deficient"] == "pivoted-qr"
    assert "dense_factorization" not in held
    with pytest.raises(ValueError, match="rank_deficient must be one of"):
        so.pop_from({"rank_deficient": "device"})
    with projector.rank_deficient("pivoted-qr"):
        assert projector.rank_deficient_choice() == "pivoted-qr"
        # an option that is not given keeps the value in force
        assert "rank_deficient" not in so.pop_from({})
        with so.scoped(**so.pop_from({})):
            assert so.current().rank_deficient == "pivoted-qr"
        # the options beside the tuple survive a change of another one
        with so.scoped(link_rows=1, dense_factorization="householder-qr"):
            cur = so.current()
            assert (cur.rank_deficient, cur.dense_factorization, cur.link_rows) == \
                ("pivoted-qr", "householder-qr", 1)
    assert projector.rank_deficient_choice() == "host-svd"
    with pytest.raises(RuntimeError, match="inside"):
        with so.scoped(rank_deficient="pivoted-qr"):
            raise RuntimeError("inside")
    assert so.current().rank_deficient == "host-svd"
    assert so.current().key() == ("iterative", 0, 0)
    with pytest.raises(ValueError):
        with so.scoped(rank_deficient="svd"):
            pass
    assert so.current().rank_deficient == "host-svd"


def test_row_sharded_backend_refuses_the_option():
    import problems
    p = problems.Maratos()
    with pytest.raises(NotImplementedError, match="rank_deficient='pivoted-qr': the "
                                                  "row-sharded backend builds its own"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, p.hess, p.constraints(ipsolver),
                                      options={"shard": True, "rank_deficient": "pivoted-qr"})
    assert so.current().rank_deficient == "host-svd"


@pytest.mark.parametrize("name,args", cases.all_cases())
def test_case_conditions(name, args):
    """Conditions on the INPUTS of tests/test_gpu_rank_deficient.py, not on the code under test:
    the oracle works with the intended rank, and the pivots of LAPACK's column-pivoted QR that the
    device's relative rule must keep (drop) are >= 2^-30 (<= 2^-46) of the first one -- both far
    from its threshold 2^-43."""
    A, rank = cases.build(*args)
    m = A.shape[0]
    assert cases.oracle_rank(A) == rank
    d = np.abs(np.diag(scipy.linalg.qr(A.T, pivoting=True, mode="r")[0]))
    if rank == 0:
        assert not d.any()
        return
    kept = d[:rank].min() / d[0]
    dropped = d[rank:].max() / d[0] if rank < m else 0.0
    print("%s: rank %d, kept >= 2^%.1f, dropped <= 2^%.1f"
          % (name, rank, np.log2(kept), np.log2(dropped) if dropped > 0 else -np.inf))
    assert kept >= 2.0 ** -30
    assert dropped <= 2.0 ** -46


@pytest.mark.parametrize("cond", cases.E2E_CONDS)
def test_e2e_problem_conditions(cond):
    A, H, c, b, independent = cases.e2e_problem(cond)
    m = len(independent)
    assert A.shape == (m + cases.E2E_EXTRA, H.shape[0])
    assert cases.oracle_rank(A) == m
    assert np.linalg.matrix_rank(A[independent]) == m
    # the added rows are consistent: b lies in the range of A up to rounding
    x = np.linalg.lstsq(A[independent], b[independent], rcond=None)[0]
    assert np.max(np.abs(A @ x - b)) <= 1e-12 * np.max(np.abs(b))
