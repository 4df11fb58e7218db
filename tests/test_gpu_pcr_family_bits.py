"""The cyclic-reduction kernels of csrc/banded.hip against bits recorded from them.

k_pcr_check, k_solve_pcr and k_step1_solve_tail share their arithmetic (csrc/pcr_window.h), and
the parity tests of the suite (test_gpu_projection_placement.py, test_gpu_cg_fused_projection.py,
test_gpu_qp.py) compare the fused launch with the separate ones -- forms that a change to the
shared pieces moves TOGETHER.  This test anchors them: every array that the cases of
tests/pcr_family_cases.py return must be ``array_equal`` to tests/golden/pcr_family_bits.npz,
recorded on an MI355X from the commit before the pieces were shared (``tests/golden/
make_golden.py --pcr-family``).  Vectors of more than 512 entries are compared through a digest
that any changed bit changes (pcr_family_cases.digest).

A later change that reorders a sum of these kernels ON PURPOSE re-records the fixture, and says
so; one that does not mean to must leave it as it is.

Cases (instantiation reached):
  projection_m*       7, 8, 9, 18 and 25 windows, two iterations of the bare loop: the fused
                      launch (k_step1_solve_tail<6, 0 and 2, false, true>), the same reading the
                      column table (CONTIG = false), the separate launches (k_solve_pcr<6, 1>)
  projection_radius   XN = 0 in every iteration (``read-xn2``), XN = 1 (no radius)
  priming             the public call whose priming projections are k_step1_solve_tail<.., PRIME>
                      launches with sign +1 and -1, and the same through k_solve_pcr
  tail_qv2/4/8        k_solve_pcr<2 / 4 / 8, 1>: 780, 1560 and 2990 variables per window (n even:
                      the pair tail needs the ELL(2) form of A', which an odd n does not get)
  level_*             k_pcr_check's verdict (status, level, decoupled, geometry) on one matrix per
                      outcome: level 4, 6 and 7, separators coupled, still coupled at distance
                      128, a non-positive reduced diagonal; where the reduction is the solve,
                      k_solve_pcr<0, 1> (levels 4, 6) and <0, 2> (level 7: a window of 516 rows)
                      without and with residual partials
  rows                the nine-window box-Schur problem (bounds on one side): k_solve_pcr<0, 1,
                      true> forming its own right-hand side
  rows_post           the same general rows with bounds on both sides of every variable: the
                      per-item tail, k_solve_pcr<0, 1, true, 512, true>
Which kernel each of tail_qv* and rows* launches was read off a kernel trace of the recording.
"""
import numpy as np
import pytest

import pcr_family_cases as cases
from conftest import load_npz


@pytest.fixture(scope="module")
def golden():
    return load_npz("pcr_family_bits")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_bits_of_the_recorded_commit(golden, name):
    got = cases.CASES[name]()
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert want and sorted(got) == sorted(want)
    differ = [k for k in sorted(got)
              if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert not differ, (name, differ)


def test_level_seven_matrix_in_the_numpy_model():
    """The matrices of the ``level_*`` cases in a numpy model of k_pcr_check (runs without a GPU).
    ``L7``, the one that reaches k_solve_pcr<0, 2> (a window of 260 + 2 * 128 = 516 rows, two per
    lane): the coupling at distance 64 is above 2^-56 of the reduced diagonal by a factor 1.3 --
    the decision edge of test_gpu_normal_solve.test_cyclic_reduction_decision_edges, whose matrix
    this is; it cannot be far from the edge, a slower decay couples the chunk separators, 65 rows
    apart, and takes the solve off the reduction -- and the one at distance 128 is 17 orders
    below it.  The model divides where the kernel multiplies by a reciprocal good to an ulp
    (v_rcp_f64 and one Newton step): seven levels of such differences move a ratio by parts in
    1e15, not by the 30 % that separate 1.3 from the threshold; the recorded verdict is level 7."""
    ratios = cases.reduction_model(cases.LEVEL_CASES["L7"](3000))
    assert all(r > 1e8 for r in ratios[:5]) and 1.2 < ratios[5] < 1.5 and ratios[6] < 1e-15
    low = cases.reduction_model(cases.LEVEL_CASES["low"](3000))
    assert low[2] > 1.0 and low[3] < 1e-9                    # level 4
    six = cases.reduction_model(cases.LEVEL_CASES["L6"](3000))
    assert six[4] > 1.0 and six[5] < 1e-6                    # level 6
    assert cases.reduction_model(cases.LEVEL_CASES["coupled"](3000))[6] > 1.0
    assert min(cases.reduction_model(cases.LEVEL_CASES["indefinite"](3000))) < 0.0
