"""Host side of the wide block-tridiagonal solver: block size from the half bandwidth, the inputs
of tests/test_gpu_blockwide.py (exactly representable S, the half bandwidth and conditioning
claimed for them), the new value of the wide-band policy.  No GPU."""
import numpy as np
import pytest

import blocktri_cases as bc
import blockwide_cases as bw
import normal_ref as nr


def test_block_size_from_half_bandwidth():
    from ipsolver import blockwide, projector
    for k, b in bw.BLOCK_OF_K.items():
        assert blockwide.block_size(k) == b
    assert blockwide.BLOCK_SIZES == (128, 256)
    assert projector.WideBlockTridiagonalNormalSolver is blockwide.WideBlockTridiagonalNormalSolver
    with pytest.raises(NotImplementedError, match="257"):
        blockwide.block_size(257)
    # the existing solver's limits are where they were
    from ipsolver import blocktri
    assert blocktri.BLOCK_SIZES[-1] == 64
    with pytest.raises(NotImplementedError, match="65"):
        blocktri.block_size(65)


@pytest.mark.parametrize("k", bw.KS)
def test_inputs_of_the_gpu_test_are_what_they_claim(k):
    """Every matrix of the solve test: S within 26 significant bits (residual_exact's
    condition), half bandwidth min(k, m - 1), kappa of the scaled S within the family's."""
    worst = {False: 0.0, True: 0.0}
    b = bw.BLOCK_OF_K[k]
    for name, m, private, graded in bw.edge_cases(k):
        A, e, w = bw.build(k, name, m, private, graded)
        S = nr.gram_pow2(A, e)
        nr.assert_26_bits(S.data)
        assert bc.half_bandwidth(S) == min(k, m - 1), (name, m)
        assert len(w) == m and np.all(np.isfinite(w))
        assert bw.levels(m, b) == {1: 1, 2: 2, 3: 3, 4: 3, 5: 4, 6: 4, 9: 5, 10: 5}[-(-m // b)]
        worst[private] = max(worst[private], nr.scaled_cond(nr.gram_pow2(A)))
    print("k=%d: kappa plain %.3g private %.3g" % (k, worst[False], worst[True]))
    assert worst[False] <= bw.KAPPA_PLAIN and worst[True] <= bw.KAPPA_PRIVATE, worst


def test_other_inputs():
    rng = np.random.default_rng(0)
    assert bc.half_bandwidth(nr.gram_pow2(bc.ocp_rows(40, 8, 12, rng))) == 79
    assert bc.half_bandwidth(nr.gram_pow2(bc.ocp_rows(70, 10, 6, rng))) == 139
    assert bc.half_bandwidth(nr.gram_pow2(bc.band_rows(rng, 600, 300, lim=2 ** 4))) == 300
    A = bc.identical_rows(np.random.default_rng(4), m=300, k=65, at=128)
    S = nr.gram_pow2(A).toarray()
    assert S[128, 128] == 256 and np.array_equal(S[128], S[129])
    assert 64 < bc.half_bandwidth(S) <= 128
    for k, m in ((65, 257), (129, 513)):
        assert bc.half_bandwidth(nr.gram_pow2(bc.band_rows(rng, m, k, lim=bw.LIM))) == k


def test_the_new_policy_value_is_accepted_nests_and_restores():
    from ipsolver import projector
    assert projector.WIDE_BAND_POLICIES == ("iterative", "block-tridiagonal",
                                            "block-tridiagonal-wide")
    assert projector.wide_band_policy() == "iterative"
    assert projector.check_wide_band("block-tridiagonal-wide") == "block-tridiagonal-wide"
    with pytest.raises(RuntimeError):
        with projector.wide_band("block-tridiagonal-wide"):
            assert projector.wide_band_policy() == "block-tridiagonal-wide"
            with projector.wide_band("block-tridiagonal"):
                assert projector.wide_band_policy() == "block-tridiagonal"
                with projector.wide_band("iterative"):
                    assert projector.wide_band_policy() == "iterative"
            assert projector.wide_band_policy() == "block-tridiagonal-wide"
            raise RuntimeError("inside")
    assert projector.wide_band_policy() == "iterative"


def test_an_unknown_value_is_still_refused():
    import ipsolver
    from ipsolver import projector
    with pytest.raises(ValueError, match="wide_band"):
        with projector.wide_band("block-tridiagonal-wider"):
            pass
    assert projector.wide_band_policy() == "iterative"
    calls = []
    with pytest.raises(ValueError, match="wide_band"):
        ipsolver.minimize_constrained(lambda x: calls.append(1) or 0.0, np.zeros(2),
                                      lambda x: np.zeros(2), options={"wide_band": "wide"})
    assert not calls
