"""k_cg_step2_hp (csrc/cg.hip) on shifted-contiguous row tiles -- entry k of row i at span offset
``col16[s] + i + k``, the interior tiles of a banded Hessian -- which carry a flag bit in the
per-tile table (ipsolver.cg_fused.flagged_rowlen): the GUARD form then forms their column offsets
instead of reading them, the plain and XSUM forms mask the bit and read the table.

Every Hessian of tests/test_gpu_step2_hp_row_lanes.py and of tests/test_gpu_loop_kernel_edges.py
runs in the plain, GUARD and XSUM forms, with the offsets formed (the default) and with the table
read for every tile (debug form ``table-columns``), and each run is compared BIT FOR BIT with the
twin of those files -- the vector k_cg_step2 followed by k_csr_spmv -- on x, p, r, Hp, v, the
partial arrays and the state block after 1, 2 and 5 iterations.  The twin of a case and form is
run once and shared.

Which tiles carry the flag is worked out here from the scipy matrix, row by row, and compared
with the table the kernel was given: interior tiles of the tridiagonal and pentadiagonal
matrices and every tile of the diagonal one do, the first and last tile of a banded matrix (a
shorter edge row), the tile with the two longer rows and the 2 x 2 and 4 x 4 blocks (uniform, but
not shifted by one per row) do not.
"""
import numpy as np
import pytest

import test_gpu_loop_kernel_edges as edges
import test_gpu_step2_hp_row_lanes as lanes

pytestmark = pytest.mark.gpu

FORMS = ("inf", "guard", "xsum")
CASES = sorted(lanes.CASES) + ["edges:" + name for name in sorted(edges.HESSIANS)]
# cases whose tiles must (True) / must not (False) hold a flagged tile
FLAGGED = {"tridiagonal-2100": True, "tridiagonal-2732": True, "tridiagonal-2733": True,
           "pairs": False, "diagonal": True, "blocks-of-4": False, "pentadiagonal": True,
           "longer-row-between": True, "separate-diagonal": True, "signed-zeros": True,
           "edges:tridiagonal-2000": True, "edges:pentadiagonal": True,
           "edges:one-longer-row": True, "edges:short-last-tile": True, "edges:pairs": False}


def problem(case):
    return edges.hessian_problem(case[6:]) if case.startswith("edges:") else lanes.problem(case)


def shifted_by_rows(pat):
    """Per row tile: uniform, non-empty, and row i a run of consecutive columns that starts i
    columns to the right of row 0's -- from the row pointers and column indices alone."""
    nt = pat.ntiles
    rows = pat.tiles_h[:nt + 1].astype(np.int64)
    indptr, indices = pat.indptr_h.astype(np.int64), pat.indices_h.astype(np.int64)
    out = []
    for r0, r1 in zip(rows[:-1], rows[1:]):
        lens = np.diff(indptr[r0:r1 + 1])
        ok = r1 > r0 and lens[0] > 0 and bool(np.all(lens == lens[0]))
        if ok:
            first = indices[indptr[r0]]
            for i in range(r1 - r0):
                cols = indices[indptr[r0 + i]:indptr[r0 + i + 1]]
                ok = ok and np.array_equal(cols, first + i + np.arange(lens[0]))
        out.append(bool(ok))
    return out


def hp_loop(monkeypatch, q, form, table):
    """lanes.hp_loop's fused loop, with the column table read for every tile or not."""
    import ipsolver.cg_fused as cg_fused
    monkeypatch.setenv("IPX_DEBUG_FORMS", lanes.FORMS[form] + (",table-columns" if table else ""))
    L = cg_fused._Loop(q.H, q.P, None, None, resident=False, fused_projection=q.n % 2 == 0)
    a = L.args
    assert not a.resident and a.H_hmax > 0 and bool(a.xsums) and bool(a.A_span)
    assert bool(a.H_col16) and bool(a.H_rowlen)
    return L


_TWINS = {}


def twin(monkeypatch, case, form):
    if (case, form) not in _TWINS:
        q = problem(case)
        radius = np.inf if form == "inf" else 1e300
        with monkeypatch.context() as mp:      # (the twin's fuse_halo answers 0: not beyond here)
            _TWINS[case, form] = edges.snapshots(lanes.hp_loop(mp, q, False, form), q, radius)
    return _TWINS[case, form]


@pytest.mark.parametrize("table", [False, True], ids=["formed", "table"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_formed_offsets_against_step2_and_spmv(monkeypatch, case, form, table):
    import ipsolver.cg_fused as cg_fused
    q = problem(case)
    want = twin(monkeypatch, case, form)
    L = hp_loop(monkeypatch, q, form, table)
    pat = lanes.csr_of(q).pattern
    word = L.H_rowlen.cpu().numpy()
    rl = np.array(lanes.rowlen_of(q))
    flag = (word >= 0) & ((word & cg_fused.ROWLEN_SHIFTED) != 0)
    assert np.array_equal(np.where(word < 0, -1, word & (cg_fused.ROWLEN_SHIFTED - 1)), rl)
    if table:
        assert not flag.any()
    else:
        assert flag.tolist() == shifted_by_rows(pat), (flag.tolist(), rl.tolist())
        assert bool(flag.any()) == FLAGGED[case]
        if FLAGGED[case] and case != "diagonal":
            # flagged and unflagged tiles in one launch
            assert not flag.all()
    radius = np.inf if form == "inf" else 1e300
    got = edges.snapshots(L, q, radius, guard=form == "guard")
    edges.assert_same_bits(got, want)
