"""Quasi-Newton Hessians (ipsolver.LBFGS / ipsolver.LSR1) without a GPU: the numpy twin of the
compact forms against the dense recursions, the library's host copy of the middle-matrix step
against the twin, and the public parameters' validation."""
import numpy as np
import pytest

import ipsolver
from ipsolver import _hip

from quasi_newton_twin import CompactTwin, HostMemory, dense_recursion


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _spd(n, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Q @ np.diag(rng.uniform(0.5, 20.0, n)) @ Q.T


def _indefinite(n, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Q @ np.diag(rng.uniform(-5.0, 10.0, n)) @ Q.T


def _lbfgs_sequence(n, rng):
    """pairs y = A s with a skipped pair (s'y < 0) and s = 0 among them"""
    A = _spd(n, rng)
    seq = []
    for k in range(11):
        s = rng.standard_normal(n)
        seq.append((s, A @ s))
        if k == 3:
            seq.append((s, -s))                     # negative curvature: skipped
        if k == 6:
            seq.append((np.zeros(n), np.zeros(n)))  # the same point: no update
    return seq


@pytest.mark.parametrize("memory,init", [(3, None), (5, None), (4, 2.5), (32, None)])
def test_lbfgs_twin_is_the_dense_recursion_and_the_library_matches_it(memory, init):
    rng = np.random.default_rng(memory)
    n = 24
    twin = CompactTwin(0, memory, init)
    host = HostMemory(_hip.load(), 0, memory, n, init)
    for s, y in _lbfgs_sequence(n, rng):
        twin.update(s, y)
        host.update(s, y)
        assert (host.counts) == (twin.updates, twin.skipped)
        B = twin.B(n)
        if twin.S:
            assert _rel(B, dense_recursion(0, twin.S, twin.Y, twin.sigma)) < 1e-12
        assert host.sigma == pytest.approx(twin.sigma, rel=1e-14)
        assert _rel(host.B(), B) < 1e-12
    assert twin.skipped == 1 and twin.updates == 11
    assert min(memory, 11) == len(twin.S) == int(host.state[1])


@pytest.mark.parametrize("memory,init", [(3, None), (6, None), (4, 0.7)])
def test_lsr1_twin_is_the_dense_recursion_and_the_library_matches_it(memory, init):
    rng = np.random.default_rng(10 + memory)
    n = 20
    A = _indefinite(n, rng)
    twin = CompactTwin(1, memory, init)
    host = HostMemory(_hip.load(), 1, memory, n, init)
    skipped = 0
    for k in range(12):
        s = rng.standard_normal(n)
        if k in (4, 9):
            # y - Bs orthogonal to s: the SR1 denominator vanishes -- skipped
            t = rng.standard_normal(n)
            t -= (t @ s) / (s @ s) * s
            y = twin.B(n) @ s + t
            skipped += 1
        else:
            y = A @ s
        if k == 7:
            twin.update(np.zeros(n), np.zeros(n))
            host.update(np.zeros(n), np.zeros(n))
        twin.update(s, y)
        host.update(s, y)
        assert host.counts == (twin.updates, twin.skipped)
        B = twin.B(n)
        if twin.S and len(twin.S) == twin.updates:    # (no pair dropped yet)
            assert _rel(B, dense_recursion(1, twin.S, twin.Y, twin.sigma)) < 1e-10
        assert _rel(host.B(), B) < 1e-12
        assert _rel(host.dot(s), B @ s) < 1e-12
    assert twin.skipped == skipped
    assert twin.updates == 12 - skipped


def test_lsr1_compact_form_equals_the_recursion_before_the_memory_drops_pairs():
    rng = np.random.default_rng(3)
    n, memory = 15, 8
    A = _indefinite(n, rng)
    twin = CompactTwin(1, memory)
    for _ in range(memory):
        s = rng.standard_normal(n)
        twin.update(s, A @ s)
    assert twin.updates == memory
    assert _rel(twin.B(n), dense_recursion(1, twin.S, twin.Y, twin.sigma)) < 1e-12


def test_lsr1_sigma_is_fixed_at_the_first_stored_pair():
    rng = np.random.default_rng(5)
    n = 10
    host = HostMemory(_hip.load(), 1, 4, n)
    s = rng.standard_normal(n)
    host.update(s, 3.0 * s + 0.1 * rng.standard_normal(n))
    sigma = host.sigma
    assert host.counts == (1, 0) and sigma != 1.0
    for _ in range(5):
        s = rng.standard_normal(n)
        host.update(s, 7.0 * s + rng.standard_normal(n))
    assert host.sigma == sigma


def test_the_gram_is_the_gram_of_the_ring():
    rng = np.random.default_rng(8)
    n, memory = 12, 3
    host = HostMemory(_hip.load(), 0, memory, n)
    A = _spd(n, rng)
    for _ in range(7):                              # two wrap-arounds
        s = rng.standard_normal(n)
        host.update(s, A @ s)
    assert _rel(host.gram(), host.W @ host.W.T) < 1e-13


@pytest.mark.parametrize("cls", [ipsolver.LBFGS, ipsolver.LSR1])
def test_parameters_are_validated(cls):
    for bad in (0, 33, -1, 2.5, "10", True):
        with pytest.raises(ValueError):
            cls(memory=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "full"):
        with pytest.raises(ValueError):
            cls(init_scale=bad)
    cls(memory=1)
    cls(memory=32, init_scale=3.0)
    obj = cls()
    assert not callable(obj)
    assert obj.memory == 10 and obj.init_scale == 'auto'
    assert cls.__name__ in ipsolver.__all__


def test_threshold_parameters():
    assert ipsolver.LBFGS(min_curvature=0.0).min_curvature == 0.0
    assert ipsolver.LSR1(min_denominator=1e-6).min_denominator == 1e-6
    with pytest.raises(ValueError):
        ipsolver.LBFGS(min_curvature=-1.0)
    with pytest.raises(ValueError):
        ipsolver.LSR1(min_denominator=float("nan"))


def _problem():
    return (lambda x: float(x @ x), np.ones(3), lambda x: 2 * x)


@pytest.mark.parametrize("strategy", [ipsolver.LBFGS(), ipsolver.LSR1()])
def test_constant_hessian_is_refused(strategy):
    fun, x0, grad = _problem()
    with pytest.raises(ValueError, match="constant_hessian"):
        ipsolver.minimize_constrained(fun, x0, grad, strategy,
                                      options={'constant_hessian': True})


@pytest.mark.parametrize("strategy", [ipsolver.LBFGS(), ipsolver.LSR1()])
def test_sharded_backend_is_refused(strategy):
    fun, x0, grad = _problem()
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ipsolver.minimize_constrained(fun, x0, grad, strategy, options={'shard': True})

    class FakeShardVec:          # what minimize recognises a distributed start vector by
        sh = None
        owns = None
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ipsolver.minimize_constrained(fun, FakeShardVec(), grad, strategy)
