"""The dense QR projectors against bits recorded from them.

The tolerance tests (test_gpu_dense_qr.py, test_gpu_rank_deficient.py) compare the Householder QR
and the pivoted QR / complete orthogonal decomposition with LAPACK and the oracle, and with
themselves.  This test anchors them to a commit: every array that the cases of
tests/dense_qr_bits_cases.py return must be ``array_equal``, with the same dtype, to
tests/golden/dense_qr_bits.npz, recorded on an MI355X from the commit before the projectors got
their shared base and the two kernel files their shared header (``tests/golden/make_golden.py
--dense-qr-bits``).  Arrays of more than 512 entries are compared through a digest that any
changed bit changes (pcr_family_cases.digest).  The launch and blocking-read counts of every
construction and of the operator calls are among the arrays.

A later change that reorders a sum of these kernels, or adds a launch, ON PURPOSE re-records the
fixture, and says so; one that does not mean to must leave it as it is.

Cases (path reached):
  qr-normal-*, qr-graded-*   ``DenseQRProjector``: one row; one panel; panel + 1; two panels + 2
                             with a ragged n and two chunks; nine panels, the last from chunk 1
  cod-*                      ``DenseCODProjector``: rank 0 (early return), low rank, the usual
                             shapes, and (520, 2100), whose steps from j = 512 start at chunk 1
  public-*                   ``projector.projections`` under each option: the operators and
                             ``last_normal_solver()``
"""
import numpy as np
import pytest

import dense_qr_bits_cases as cases
from conftest import load_npz


@pytest.fixture(scope="module")
def golden():
    return load_npz("dense_qr_bits")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_bits_of_the_recorded_commit(golden, name):
    got = cases.CASES[name]()
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert want and sorted(got) == sorted(want)
    differ = [k for k in sorted(got)
              if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    assert not differ, (name, differ)
