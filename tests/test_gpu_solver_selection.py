"""The selection of the (A A')^-1 solver (ipsolver/selection.py) against the table recorded before
it was rewritten as a rule list (tests/golden/solver_selection.json, written by
scripts/record_solver_selection.py on an MI355X): for every case of tests/selection_cases.py under
every combination of the options, the same solver, the same row-permutation flags, and the same
number of launches and blocking reads for the factorization -- the device sees the same work.
(A case without ``launches`` / ``reads`` in the file: its counts differed between two recordings
of the same code and were dropped there.)
"""
import importlib.util
import json
import os

import pytest

import selection_cases as sc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "solver_selection.json")) as f:
    TABLE = json.load(f)


@pytest.fixture(scope="module")
def measure():
    spec = importlib.util.spec_from_file_location(
        "record_solver_selection", os.path.join(ROOT, "scripts", "record_solver_selection.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.measure


def test_the_table_covers_the_catalog():
    assert sorted(TABLE) == sorted(sc.CASES)
    ids = sorted(sc.option_id(o) for o in sc.OPTIONS)
    assert len(ids) == 12 and all(sorted(TABLE[name]["entries"]) == ids for name in TABLE)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_selection_is_the_recorded_one(measure, name):
    A, max_rows = sc.build(name)
    gold = TABLE[name]
    assert list(A.shape) == gold["shape"] and max_rows == gold["max_rows"]
    for options in sc.OPTIONS:
        want = gold["entries"][sc.option_id(options)]
        got = measure(A, max_rows, options)
        print("%-28s %-40s %s" % (name, sc.option_id(options), got))
        assert set(want) >= {"solver", "row_perm", "row_order"}
        assert {key: got[key] for key in want} == want, (name, options)


def test_link_solver_is_declined_as_ill_conditioned():
    """What the table cannot tell apart by the name: for ``linked-ill-conditioned`` the linked
    solver is BUILT (no refusal, every pivot of K positive) with one pivot below 2^-43 of its
    F_jj, and it is ``link_solver`` that declines it."""
    from ipsolver import device as dv, projector as proj
    A, rows = sc.link_row_nearly_in_the_band()
    Ad = dv.DeviceCSR.from_scipy(A)
    with proj.link_rows(4):
        split = proj._link_split_for(Ad.pattern)
        assert split is not None and list(split.d_rows) == list(rows)
        solver = proj.LinkedRowsNormalSolver(Ad, split)
        assert solver.flag_bits == 1 and solver.ill_conditioned
        assert 2.0 ** 43 < solver.cancellation < 2.0 ** 53
        assert proj.link_solver(Ad) is None
