"""Host side of the solver selection (ipsolver/selection.py, solver_options.py): the pattern facts
the rules read, against the table recorded on an MI355X before the selection was rewritten
(tests/golden/solver_selection.json).  No GPU: the facts are host work on host patterns.
"""
import json
import os

import numpy as np
import pytest

import selection_cases as sc
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "solver_selection.json")) as f:
    TABLE = json.load(f)


class _HostMatrix:
    """What the facts read of a device matrix."""

    def __init__(self, A):
        from ipsolver.banded import HostPattern
        self.shape = A.shape
        self.pattern = HostPattern(A.indptr, A.indices, A.shape)


def test_option_key_tells_every_combination_apart():
    from ipsolver import solver_options as so
    keys = []
    for policy, border, link in sc.OPTIONS:
        with so.scoped(wide_band=policy, border_columns=border, link_rows=link):
            keys.append(so.current().key())
            assert so.current() == (policy, border, link)
    assert len(set(keys)) == len(sc.OPTIONS) == 12
    assert so.current().key() == ("iterative", 0, 0)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_pattern_facts_agree_with_the_recorded_selection(name):
    from ipsolver import selection, solver_options as so
    A, _ = sc.build(name)
    gold = TABLE[name]["entries"]
    if isinstance(A, np.ndarray):
        assert not any(e["row_order"] or e["row_perm"] for e in gold.values())
        return
    Ah = _HostMatrix(A)
    for policy, border, link in sc.OPTIONS:
        want = gold[sc.option_id((policy, border, link))]
        with so.scoped(wide_band=policy, border_columns=border, link_rows=link):
            f = selection._Facts(Ah)
            order = selection._banded_row_order(Ah)
            found = {"Linked": f.link_split is not None, "Bordered": f.border_split is not None}
            inner = {"Linked": selection._link_split_for, "Bordered": selection._border_split_for}
            assert (order is not None) == want["row_order"], (name, policy, border, link)
            solver = want["solver"] or ""
            for kind, limit in (("Linked", link), ("Bordered", border)):
                if limit == 0 or want["row_order"]:
                    assert not found[kind]
                if solver.startswith(kind):
                    assert found[kind]
                in_general = f.box_any and inner[kind](f.general) is not None
                if solver.startswith("BoxSchurNormalSolver/" + kind):
                    assert in_general
                # this option alone changed the device's work (a solver built and refused, declined
                # or discarded included): only a found split does that
                off = gold[sc.option_id((policy, 0, 0))]
                if limit and (border == 0 or link == 0) and "launches" in want \
                        and want["launches"] != off["launches"]:
                    assert found[kind] or in_general, (name, policy, border, link)


def test_general_rows_are_analysed_once(monkeypatch):
    """The analysis the selection's facts make on the host pattern of the general rows is handed
    to the device selection's pattern when that is made, and the facts read that pattern from
    then on -- whichever of the two comes first, ``_Symbolic`` runs once.  (The device selection
    is stood in for by a host object: no GPU here.)"""
    from ipsolver import banded, boxschur, selection, solver_options as so

    class HostSelection:
        row_pointers = staticmethod(boxschur.RowSelection.row_pointers)

        def __init__(self, pattern, rows, sign):
            host = boxschur.general_rows_pattern(pattern)
            self.pattern = banded.HostPattern(host.indptr_h, host.indices_h, host.shape)

    made = []
    real = banded._Symbolic

    def counting(pattern):
        made.append(pattern)
        return real(pattern)
    monkeypatch.setattr(boxschur, "RowSelection", HostSelection)
    monkeypatch.setattr(banded, "_Symbolic", counting)
    # facts first, as in ``_rule_barrier_jacobian``
    Ah = _HostMatrix(sc.build("box-band")[0])
    with so.scoped(border_columns=4, link_rows=4):
        f = selection._Facts(Ah)
        host = f.general
        assert f.box_banded and selection._border_split_for(host) is None
        assert selection._link_split_for(host) is None and made == [host]
        sel = boxschur.general_rows(Ah.pattern)
        assert sel.pattern is not host and f.general is sel.pattern
        for name in (banded._SYMBOLIC_ATTR, "_ipx_aat_half_bw", "_ipx_border_split",
                     "_ipx_link_split"):
            assert sel.pattern.__dict__[name] is host.__dict__[name], name
        assert banded._symbolic_for(sel.pattern) is banded._symbolic_for(host) and len(made) == 1
    # the device selection first, as when ``BoxSchurNormalSolver`` is built directly
    del made[:]
    Ah = _HostMatrix(sc.build("box-band")[0])
    sel = boxschur.general_rows(Ah.pattern)
    sym = banded._symbolic_for(sel.pattern)
    f = selection._Facts(Ah)
    assert f.general is sel.pattern and f.general_k == sym.k and made == [sel.pattern]
