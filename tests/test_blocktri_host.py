"""Host side of the block-tridiagonal solver: block size from the half bandwidth, the inputs of
tests/test_gpu_blocktri.py (exactly representable S, the half bandwidth and conditioning claimed
for them), the wide-band policy's plumbing.  No GPU."""
import numpy as np
import pytest

import blocktri_cases as bc
import normal_ref as nr


def test_block_size_from_half_bandwidth():
    from ipsolver import blocktri, projector
    for k, b in bc.BLOCK_OF_K.items():
        assert blocktri.block_size(k) == b
    assert blocktri.block_size(1) == 16 and projector.block_size(5) == 16
    with pytest.raises(NotImplementedError, match="65"):
        blocktri.block_size(65)


@pytest.mark.parametrize("k", bc.KS)
def test_inputs_of_the_gpu_test_are_what_they_claim(k):
    """Every matrix of the solve test: S within 26 significant bits (residual_exact's
    condition), half bandwidth min(k, m - 1), kappa of the scaled S within the family's."""
    worst = {False: 0.0, True: 0.0}
    for name, m, private, graded in bc.edge_cases(k):
        A, e, w = bc.build(k, name, m, private, graded)
        S = nr.gram_pow2(A, e)
        nr.assert_26_bits(S.data)
        assert bc.half_bandwidth(S) == min(k, m - 1), (name, m)
        assert len(w) == m and np.all(np.isfinite(w))
        if m > 1:
            worst[private] = max(worst[private], nr.scaled_cond(nr.gram_pow2(A)))
    print("k=%d: kappa plain %.3g private %.3g" % (k, worst[False], worst[True]))
    assert worst[False] <= bc.KAPPA_PLAIN and worst[True] <= bc.KAPPA_PRIVATE, worst


def test_other_inputs():
    rng = np.random.default_rng(0)
    A = bc.ocp_rows(12, 4, 40, rng)
    assert np.abs(A.data).max() <= 2 ** 6 and np.array_equal(A.data, np.round(A.data))
    assert bc.half_bandwidth(nr.gram_pow2(A)) == 23
    assert bc.half_bandwidth(nr.gram_pow2(bc.ocp_rows(6, 2, 30, rng))) == 11
    S = nr.gram_pow2(bc.moving_average(1500, 11, 512, 1))
    nr.assert_26_bits(S.data)
    assert bc.half_bandwidth(S) == 11
    A = bc.identical_rows(np.random.default_rng(4))
    S = nr.gram_pow2(A).toarray()
    assert S[16, 16] == 256 and np.array_equal(S[16], S[17]) and bc.half_bandwidth(S) <= 16
    for k, m in ((9, 47), (16, 48), (17, 65), (33, 129)):
        assert bc.half_bandwidth(nr.gram_pow2(bc.band_rows(rng, m, k, lim=bc.lim_for(k)))) == k


def test_wide_band_policy_plumbing():
    from ipsolver import projector
    assert projector.wide_band_policy() == "iterative"
    with pytest.raises(ValueError, match="wide_band"):
        with projector.wide_band("cholesky"):
            pass
    assert projector.wide_band_policy() == "iterative"
    with pytest.raises(RuntimeError):
        with projector.wide_band("block-tridiagonal"):
            assert projector.wide_band_policy() == "block-tridiagonal"
            with projector.wide_band("iterative"):
                assert projector.wide_band_policy() == "iterative"
            assert projector.wide_band_policy() == "block-tridiagonal"
            raise RuntimeError("inside")
    assert projector.wide_band_policy() == "iterative"


def test_unknown_wide_band_option_is_refused_before_anything_runs():
    import ipsolver
    calls = []
    with pytest.raises(ValueError, match="wide_band"):
        ipsolver.minimize_constrained(lambda x: calls.append(1) or 0.0, np.zeros(2),
                                      lambda x: np.zeros(2), options={"wide_band": "direct"})
    assert not calls
