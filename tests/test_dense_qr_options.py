"""The option ``dense_factorization`` (solver_options.py): its values, its place in the cache
key, ``pop_from`` / ``scoped``, and the row-sharded backends' refusal.  No GPU."""
import numpy as np
import pytest

import ipsolver
from ipsolver import projector, solver_options as so


def test_values():
    assert so.DENSE_FACTORIZATIONS == ("normal-equations", "householder-qr")
    assert "dense_factorization" in so.NAMES
    for value in so.DENSE_FACTORIZATIONS:
        assert so.check("dense_factorization", value) == value
        assert projector.check_dense_factorization(value) == value
    for bad in ("qr", "cholesky", None, 1, ""):
        with pytest.raises(ValueError, match="dense_factorization must be one of"):
            so.check("dense_factorization", bad)


# every key that existed before the option, as the parent commit forms it
KEYS_BEFORE = [
    ({}, ("iterative", 0, 0)),
    ({"wide_band": "block-tridiagonal"}, ("block-tridiagonal", 0, 0)),
    ({"wide_band": "block-tridiagonal-wide", "border_columns": 3, "link_rows": 2},
     ("block-tridiagonal-wide", 3, 2)),
    ({"iterative_precond": "two-level"}, ("iterative", 0, 0, "two-level")),
    ({"sparse_direct": "nested-dissection"}, ("iterative", 0, 0, "nested-dissection")),
    ({"iterative_precond": "compact", "sparse_direct": "nested-dissection", "link_rows": 1},
     ("iterative", 0, 1, "compact", "nested-dissection")),
]


@pytest.mark.parametrize("changes,key", KEYS_BEFORE)
def test_key_unchanged_under_the_default(changes, key):
    assert so.current().dense_factorization == "normal-equations"
    with so.scoped(**changes):
        assert so.current().key() == key
        with so.scoped(dense_factorization="normal-equations"):
            assert so.current().key() == key
        with so.scoped(dense_factorization="householder-qr"):
            assert so.current().key() == key + ("householder-qr",)
            assert so.current().key() != key
        assert so.current().key() == key


def test_pop_from_and_scoped():
    assert "dense_factorization" not in so.pop_from({"xtol": 1e-9})
    untouched = {"xtol": 1e-9}
    so.pop_from(untouched)
    assert untouched == {"xtol": 1e-9}
    options = {"dense_factorization": "householder-qr", "xtol": 1e-9}
    held = so.pop_from(options)
    assert options == {"xtol": 1e-9} and held["dense_factorization"] == "householder-qr"
    with pytest.raises(ValueError, match="dense_factorization must be one of"):
        so.pop_from({"dense_factorization": "lapack"})
    with projector.dense_factorization("householder-qr"):
        assert projector.dense_factorization_choice() == "householder-qr"
        # an option that is not given keeps the value in force
        assert "dense_factorization" not in so.pop_from({})
        with so.scoped(**so.pop_from({})):
            assert so.current().dense_factorization == "householder-qr"
    assert projector.dense_factorization_choice() == "normal-equations"
    with pytest.raises(RuntimeError, match="inside"):
        with so.scoped(dense_factorization="householder-qr"):
            raise RuntimeError("inside")
    assert so.current().dense_factorization == "normal-equations"
    assert so.current().key() == ("iterative", 0, 0)
    with pytest.raises(ValueError):
        with so.scoped(dense_factorization="svd"):
            pass
    assert so.current().dense_factorization == "normal-equations"


def test_replace_keeps_the_options_beside_the_tuple():
    with so.scoped(dense_factorization="householder-qr", iterative_precond="compact"):
        with so.scoped(link_rows=1):
            cur = so.current()
            assert (cur.dense_factorization, cur.iterative_precond, cur.link_rows) == \
                ("householder-qr", "compact", 1)


def test_row_sharded_backend_refuses_the_option():
    import problems
    p = problems.Maratos()
    with pytest.raises(NotImplementedError, match="dense_factorization='householder-qr': the "
                                                  "row-sharded backend builds its own"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, p.hess, p.constraints(ipsolver),
                                      options={"shard": True,
                                               "dense_factorization": "householder-qr"})
    assert so.current().dense_factorization == "normal-equations"
