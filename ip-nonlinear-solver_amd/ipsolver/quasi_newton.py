"""Limited-memory quasi-Newton approximations of Hessians the user has no callback for:
``hess=LBFGS()`` or ``hess=LSR1()`` in ``minimize_constrained`` (the objective) and in
``NonlinearConstraint(fun, kind, jac, hess=...)`` (a constraint).

The objects hold parameters only.  Every solve starts from an empty memory (``_Memory``), so two
solves with the same object give the same bits.  They are deliberately not callable: the
solver's ``callable(hess)`` branches never take them for a Hessian callback.

Both rules keep the compact form ``B = sigma I + W C W'`` with ``W = [S Y]`` on the device
(csrc/lowrank.hip): S and Y are two rings of ``memory`` columns in one buffer, sigma and the
signs are folded into C, and a product is ``B p = sigma p + W (C (W'p))`` -- two HBM-bound
passes over W, no host involvement.  An update is three launches and reads nothing back.

A strategy on the objective alone approximates the objective's Hessian; constraint Hessians
then come from their callbacks, from finite differences or are absent, exactly as without a
strategy.  As soon as a nonlinear constraint carries a strategy, ONE memory per solve
approximates the SUM of all Lagrangian-Hessian terms declared with a strategy (Nocedal & Wright
section 18.3; ``LagrangianQN``): its pair is ``s = x+ - x``, ``y = grad_x L_Q(x+, v+) -
grad_x L_Q(x, v+)`` with ``L_Q`` the part of the Lagrangian whose terms carry a strategy -- the
objective's ``g+ - g`` when it participates, ``(J(x+) - J(x))' v+`` per participating constraint
(``ipx_csr_tdiff_dot``: one launch each, the gradients fused into the first).  All
participating terms must carry equal strategies.  The CG loops see one low-rank term, as for
the objective alone.  The Lagrangian's Hessian is usually indefinite, so ``LSR1`` is the rule
to prefer with constraints; ``LBFGS`` skips every pair with ``s'y <= min_curvature ||s|| ||y||``
as it does for the objective.
"""
import numbers

import numpy as np

MAX_MEMORY = 32            # IPX_LR_MAX_MEMORY: r = 2 memory <= 64 columns
KIND_LBFGS, KIND_LSR1 = 0, 1


def _check(memory, init_scale, threshold, what):
    if isinstance(memory, bool) or not isinstance(memory, numbers.Integral) \
            or not 1 <= memory <= MAX_MEMORY:
        raise ValueError("memory must be an integer between 1 and %d, got %r"
                         % (MAX_MEMORY, memory))
    if not (isinstance(init_scale, str) and init_scale == 'auto'):
        if isinstance(init_scale, (bool, str)) or not isinstance(init_scale, numbers.Real) \
                or not np.isfinite(init_scale) or init_scale <= 0:
            raise ValueError("init_scale must be 'auto' or a positive finite number, got %r"
                             % (init_scale,))
    if isinstance(threshold, (bool, str)) or not isinstance(threshold, numbers.Real) \
            or not np.isfinite(threshold) or threshold < 0:
        raise ValueError("%s must be a non-negative finite number, got %r" % (what, threshold))


class _Strategy:
    kind = None

    @property
    def init_value(self):
        """sigma the kernels take: > 0 given, 0 = 'auto'"""
        return 0.0 if isinstance(self.init_scale, str) else float(self.init_scale)

    def __repr__(self):
        return "%s(memory=%d, init_scale=%r, %s=%r)" % (
            type(self).__name__, self.memory, self.init_scale, self._threshold_name,
            self.threshold)

    def _key(self):
        return (type(self), self.memory, self.init_scale, self.threshold)

    def __eq__(self, other):
        """Equal strategies: the same class, ``memory``, ``init_scale`` and threshold (what the
        terms of one Lagrangian memory must agree on)."""
        if not isinstance(other, _Strategy):
            return NotImplemented
        return self._key() == other._key()

    def __ne__(self, other):
        eq = self.__eq__(other)
        return eq if eq is NotImplemented else not eq

    def __hash__(self):
        return hash(self._key())


class LBFGS(_Strategy):
    """Limited-memory BFGS approximation of the objective's Hessian.

    Compact form of Byrd, Nocedal & Schnabel (1994) over the stored pairs (oldest first)::

        B = sigma I - [sigma S  Y] [[sigma S'S, L], [L', -D]]^-1 [sigma S'; Y']

    with ``L`` the strictly lower triangle of ``S'Y`` and ``D`` its diagonal.

    Update rule.  Each time the solver asks for the Lagrangian Hessian at a new accepted ``x``,
    ``s = x - x_prev`` and ``y = grad f(x) - grad f(x_prev)``, ``x_prev`` the point of the last
    update and both gradients the ones the solver already evaluated (no extra gradient calls).
    ``s = 0`` (the same point again, as across barrier levels) is not an update and is not
    counted.  The pair is stored when ``s'y > min_curvature ||s|| ||y||``, otherwise skipped
    and counted in ``hess_skipped``; when the memory is full the oldest pair is dropped.
    ``sigma = y'y / s'y`` of the newest stored pair for ``init_scale='auto'`` (1 before the
    first), else ``init_scale``.  The middle matrix is inverted by Gauss-Jordan with partial
    pivoting; a pivot at or below ``1e-14 max|entry|`` skips the pair too (a guard: with every
    ``s'y > 0`` the matrix is invertible).

    Limitation: a pair is only stored along steps of positive curvature.  On an objective with
    negative curvature along the steps the solver takes (the Coulomb energy of ``Elec`` in the
    test problems) every pair after the first few is skipped, ``B`` stops changing and the solve
    can run out of iterations; ``LSR1`` stores such pairs.

    On a constraint (``NonlinearConstraint(..., hess=LBFGS())``) the memory approximates the
    Hessian of the Lagrangian's participating terms (module header), ``y`` is the difference of
    their gradients with the new multipliers, and the same skip rule applies: pairs with
    ``s'y <= min_curvature ||s|| ||y||`` are skipped.  The Lagrangian's Hessian is usually
    indefinite, so prefer ``LSR1`` with constraints.

    Parameters
    ----------
    memory : int, 1 <= memory <= 32
        Pairs kept.
    init_scale : 'auto' or float > 0
    min_curvature : float >= 0
    """
    kind = KIND_LBFGS
    _threshold_name = "min_curvature"

    def __init__(self, memory=10, init_scale='auto', min_curvature=1e-8):
        _check(memory, init_scale, min_curvature, "min_curvature")
        self.memory = int(memory)
        self.init_scale = init_scale
        self.min_curvature = float(min_curvature)

    @property
    def threshold(self):
        return self.min_curvature


class LSR1(_Strategy):
    """Limited-memory symmetric rank-one approximation of the objective's Hessian.

    Compact form over the stored pairs (oldest first)::

        B = sigma I + (Y - sigma S) (D + L + L' - sigma S'S)^-1 (Y - sigma S)'

    with ``L`` the strictly lower triangle of ``S'Y`` and ``D`` its diagonal.

    Update rule.  ``s``, ``y``, ``x_prev`` and the ``s = 0`` case as for ``LBFGS``.  ``sigma``
    is fixed at the first stored pair -- ``y'y / s'y`` when that is positive, else 1 -- or is
    ``init_scale``; before a pair is stored, each candidate is tested against ``sigma I`` with
    the sigma it would fix.  The pair is stored when ``|s'(y - Bs)| >= min_denominator ||s||
    ||y - Bs||`` (and ``s'(y - Bs) != 0``), ``B`` the current approximation, and the new middle
    matrix inverts by Gauss-Jordan with partial pivoting with every pivot above
    ``1e-14 max|entry|``; otherwise it is skipped and counted.  When the memory is full the
    oldest pair is dropped.  ``s'Bs`` and ``||y - Bs||`` follow from the Gram of ``[S Y]`` and
    ``C`` (no extra pass over the vectors).

    On a constraint (``NonlinearConstraint(..., hess=LSR1())``) the memory approximates the
    Hessian of the Lagrangian's participating terms (module header).  That Hessian is usually
    indefinite, which this rule represents: it is the one to prefer with constraints.

    Parameters
    ----------
    memory : int, 1 <= memory <= 32
    init_scale : 'auto' or float > 0
    min_denominator : float >= 0
    """
    kind = KIND_LSR1
    _threshold_name = "min_denominator"

    def __init__(self, memory=10, init_scale='auto', min_denominator=1e-8):
        _check(memory, init_scale, min_denominator, "min_denominator")
        self.memory = int(memory)
        self.init_scale = init_scale
        self.min_denominator = float(min_denominator)

    @property
    def threshold(self):
        return self.min_denominator


def is_strategy(hess):
    return isinstance(hess, _Strategy)


class LowRankTerm:
    """The memory's term ``B`` of the Lagrangian Hessian: an x-space device operator
    (``backend_hip.hessian_operator`` pads it in z-space).  A view of the memory: valid until
    the memory's next update, which is the next Hessian the solver asks for."""
    device_operator = True
    lowrank_term = True

    def __init__(self, memory):
        self.mem = memory
        self.shape = (memory.n, memory.n)

    def dot(self, p, out=None, accumulate=False):
        from . import _hip
        from .device import DVec, _empty, _p, stream_ptr
        m = self.mem
        if out is None:
            out = DVec(_empty(m.n))
            accumulate = False
        _hip.call("ipx_lowrank_apply", m.n, m.strategy.memory, _p(m.W), _p(m.state), _p(p.t),
                  _p(out.t), 1 if accumulate else 0, _p(m.part), stream_ptr())
        return out

    matvec = dot


class _Memory:
    """One solve's memory of a strategy on the device: W (n x 2 memory), the state block, the
    partial-sum scratch; the last update's point and gradient."""

    def __init__(self, strategy, n):
        import torch
        from . import _hip
        from .device import ctx
        lib = _hip.load()
        self.strategy, self.n = strategy, int(n)
        dev = ctx().device
        M = strategy.memory
        self.W = torch.zeros(2 * M * self.n, dtype=torch.float64, device=dev)
        st = np.zeros(lib.ipx_lowrank_state_doubles(M))
        st[0] = strategy.init_value if strategy.init_value > 0 else 1.0
        self.state = torch.from_numpy(st).to(dev)
        self.part = torch.empty(lib.ipx_lowrank_part_doubles(self.n, M), dtype=torch.float64,
                                device=dev)
        self.x_prev = self.g_prev = None
        self.term = LowRankTerm(self)

    def observe(self, x, g):
        """The solver asks for the Hessian at ``x`` (DVec) whose gradient is ``g`` (DVec):
        update with (x - x_prev, g - g_prev) unless it is the first point."""
        from . import _hip
        from .device import stream_ptr, _p
        if self.x_prev is not None:
            s, y = x - self.x_prev, g - self.g_prev
            st = self.strategy
            _hip.call("ipx_lowrank_update", st.kind, self.n, st.memory, st.init_value,
                      st.threshold, _p(self.W), _p(s.t), _p(y.t), _p(self.state), _p(self.part),
                      stream_ptr())
        # copies: the caller's vectors may be buffers it writes again
        self.x_prev, self.g_prev = x.copy(), g.copy()
        return self.term

    def counts(self):
        """(updates, skipped) -- one blocking read, at the end of a solve"""
        from .device import read_doubles
        v = read_doubles(self.state, 2, offset=3)
        return int(v[0]), int(v[1])


def host_hessian(strategy, grad, n):
    """``hess`` for host-callback mode: x (numpy) -> the objective's term.  ``grad`` is the
    memoised gradient (minimize._Memoize), so the gradient at an accepted point is the one the
    solver evaluated there."""
    from .device import DVec
    memory = _Memory(strategy, n)
    last = {"x": None}

    def hess(x):
        if last["x"] is not None and np.array_equal(x, last["x"]):
            return memory.term                  # the same point again: not an update
        last["x"] = np.array(x, dtype=float, copy=True)
        return memory.observe(DVec.from_host(x), DVec.from_host(grad(x)))
    return hess, memory


class DeviceGradientMemo:
    """Device-callback mode: the user's gradient callback with copies of its last few points and
    its results kept.  The solver evaluates the gradient at every accepted point before it asks for
    the Hessian there, so a lookup finds it; the point is compared by value (one blocking read
    per Hessian: the solver reuses device buffers, which a tensor's storage address or version
    does not see).  A lookup that misses calls the callback."""

    KEEP = 4

    def __init__(self, grad):
        self.grad = grad
        self._seen = []                 # (point, gradient), newest first
        self.misses = 0                 # lookups that had to call the callback

    def __call__(self, xt):
        g = self.grad(xt)
        # copies of both: the solver reuses its buffers, a callback may reuse its output
        import torch
        gt = g if torch.is_tensor(g) else g.t
        self._seen = [(xt.detach().clone(), gt.detach().clone())] + self._seen[:self.KEEP - 1]
        return g

    def lookup(self, xt):
        import torch
        for x, g in self._seen:
            if xt.shape == x.shape and bool(torch.equal(xt, x)):
                return g
        self.misses += 1
        return self(xt)


def device_hessian(strategy, memo, n):
    """``hess`` for device-callback mode: CUDA tensor -> the objective's term.  The same point
    again gives s = 0, which the update kernel ignores."""
    from . import device_mode as dm
    memory = _Memory(strategy, n)

    def hess(xt):
        g = memo.lookup(xt)
        return memory.observe(dm.as_dvec(xt), dm.as_dvec(g))
    return hess, memory


# ---- one memory for every Lagrangian term declared with a strategy -----------------------------
class QNRequest:
    """What the Hessian callback of a participating term returns: the memoised gradient at the
    point (the objective: ``g``) or the constraint's Jacobian there and its multipliers (``J``,
    ``v``: what a callable ``hess(x, v)`` would have got).  The Lagrangian's requests are
    resolved together into the memory's one term (``LagrangianQN.resolve``)."""

    def __init__(self, n, g=None, J=None, v=None):
        self.g, self.J, self.v = g, J, v
        self.shape = (int(n), int(n))

    def dot(self, p):
        from . import _hip
        raise _hip.IpxError("a quasi-Newton Hessian term is part of the Lagrangian's one memory "
                            "(LagrangianQN); it has no product of its own")


def participating(hess, constraints):
    """The strategies of a call, the objective's first -- or [] when no constraint carries one
    (then a strategy objective keeps its own memory).  Unequal strategies are a ValueError."""
    cons = [c._hess for c in constraints if is_strategy(getattr(c, "_hess", None))]
    if not cons:
        return []
    found = ([hess] if is_strategy(hess) else []) + cons
    for other in found[1:]:
        if other != found[0]:
            raise ValueError(
                "quasi-Newton Hessians of one problem share ONE memory (the Lagrangian's), so "
                "they must be equal strategies -- the same class, memory, init_scale and "
                "threshold: got %r and %r; pass equal ones, or give one of the terms a Hessian "
                "callback or finite differences" % (found[0], other))
    return found


def tdiff_dot(pattern, val_new, val_old, v, y, base=None, accumulate=False):
    """``y (+)= [base[0] - base[1]] + (J_new - J_old)' v`` for two value arrays on ``pattern``
    (``device.CSRPattern`` of J), all device tensors: one launch on the transposed pattern."""
    from . import _hip
    from .device import _p, stream_ptr
    tpat, perm = pattern.transpose()
    m, n = pattern.shape
    _hip.call("ipx_csr_tdiff_dot", n, m, pattern.nnz, _p(tpat.indptr), _p(tpat.indices), _p(perm),
              _p(tpat.tiles), tpat.ntiles, _p(val_new), _p(val_old), _p(v),
              _p(base[0]) if base is not None else None,
              _p(base[1]) if base is not None else None, _p(y), 1 if accumulate else 0,
              stream_ptr())
    return y


class LagrangianQN:
    """The one memory of a solve whose constraints carry a strategy.  ``resolve`` replaces the
    ``QNRequest``s among the Lagrangian's Hessian terms by the memory's ``LowRankTerm``, put
    first (``backend_hip.hessian_operator`` takes it as ``lowrank``); at every point but the
    first it forms ``y`` from the requests and the values kept from the previous point and
    calls ``ipx_lowrank_update`` with ``s = x - x_prev``.  The same ``x`` again (new multipliers
    across barrier levels) gives ``s = 0``, which the update kernel ignores and does not count.

    A sparse Jacobian on the pattern object of the previous point goes through
    ``ipx_csr_tdiff_dot``; a dense one, or a pattern that changed, through two transposed
    products (correct, unfused).  ``host_callbacks``: points, gradients, Jacobians and
    multipliers arrive as numpy / scipy objects and are uploaded here (a sparse Jacobian onto
    the previous point's pattern object when its structure is the same)."""

    def __init__(self, strategy, n, host_callbacks=False):
        self.strategy, self.n = strategy, int(n)
        self.host_callbacks = bool(host_callbacks)
        self.memory = None
        self.x_prev = self.g_prev = self.J_prev = None
        self._x_host = None
        self.fused_launches = self.fallback_terms = 0

    # ---- what the requests hold, on the device
    def _point(self, x):
        from .device import DVec
        if self.host_callbacks:
            return DVec.from_host(x)
        return x if isinstance(x, DVec) else DVec(x)

    def _gradient(self, g):
        import torch
        from .device import DVec
        if self.host_callbacks:
            return DVec.from_host(g)
        return g if isinstance(g, DVec) else DVec(g.to(torch.float64).reshape(-1))

    def _jacobian(self, J, prev):
        """-> DeviceCSR | DeviceDense"""
        import scipy.sparse as sps
        from .device import DeviceCSR
        from .dense import DeviceDense
        if not self.host_callbacks:
            return J
        if sps.issparse(J):
            return DeviceCSR.from_scipy(J, pattern=prev.pattern if isinstance(prev, DeviceCSR)
                                        else None)
        return DeviceDense.from_host(J)

    def _multipliers(self, v, m):
        from .device import DVec
        v = DVec.from_host(v) if self.host_callbacks else (v if isinstance(v, DVec) else DVec(v))
        if len(v) != m:
            from . import _hip
            raise _hip.IpxError("quasi-Newton constraint Hessian: %d multipliers for a Jacobian "
                                "of %d rows" % (len(v), m))
        return v

    # ---- the update
    def _y(self, g, jacs, vs):
        from .device import DVec, DeviceCSR, _empty
        y = None
        base = (g.t, self.g_prev.t) if g is not None else None
        for J, J_old, v in zip(jacs, self.J_prev, vs):
            if isinstance(J, DeviceCSR) and isinstance(J_old, DeviceCSR) \
                    and J.pattern is J_old.pattern:
                first = y is None
                if first:
                    y = DVec(_empty(self.n))
                tdiff_dot(J.pattern, J.val, J_old.val, v.t, y.t, base=base if first else None,
                          accumulate=not first)
                if first:
                    base = None
                self.fused_launches += 1
                continue
            if y is None and base is not None:
                y, base = g - self.g_prev, None
            c = J.T.dot(v) - J_old.T.dot(v)
            y = c if y is None else y + c
            self.fallback_terms += 1
        if y is None:
            y = g - self.g_prev
        return y

    def observe(self, x, requests):
        from . import _hip
        from .device import _p, stream_ptr
        if self.host_callbacks:
            if self._x_host is not None and np.array_equal(x, self._x_host):
                return self.memory.term             # the same point again: not an update
            self._x_host = np.array(x, dtype=float, copy=True)
        if self.memory is None:
            self.memory = _Memory(self.strategy, self.n)
        xd = self._point(x)
        if len(xd) != self.n:
            raise _hip.IpxError("quasi-Newton Hessian: a point of %d entries, the memory has %d"
                                % (len(xd), self.n))
        gs = [r for r in requests if r.g is not None]
        cons = [r for r in requests if r.J is not None]
        if len(gs) > 1 or (self.J_prev is not None and len(cons) != len(self.J_prev)):
            raise _hip.IpxError("quasi-Newton Hessian: the participating terms changed during a "
                                "solve")
        g = self._gradient(gs[0].g) if gs else None
        prev = self.J_prev if self.J_prev is not None else [None] * len(cons)
        jacs = [self._jacobian(r.J, p) for r, p in zip(cons, prev)]
        if self.x_prev is not None:
            vs = [self._multipliers(r.v, J.shape[0]) for r, J in zip(cons, jacs)]
            s = xd - self.x_prev
            y = self._y(g, jacs, vs)
            st = self.strategy
            _hip.call("ipx_lowrank_update", st.kind, self.n, st.memory, st.init_value,
                      st.threshold, _p(self.memory.W), _p(s.t), _p(y.t), _p(self.memory.state),
                      _p(self.memory.part), stream_ptr())
        # what the next pair needs of this point.  Host callbacks: everything was uploaded into
        # arrays of its own.  Device callbacks: the Jacobians are the memo's private copies
        # (fd_hessian.DeviceMemo: nnz doubles, or the dense buffer); the point and the gradient
        # may be buffers their owners write again
        copy = (lambda t: t) if self.host_callbacks else (lambda t: t.copy())
        self.x_prev = copy(xd)
        self.g_prev = copy(g) if g is not None else None
        self.J_prev = jacs
        return self.memory.term

    def resolve(self, terms, x):
        """A list of Hessian terms with its ``QNRequest``s replaced by the memory's term, put
        first; the other terms keep their order."""
        requests = [t for t in terms if isinstance(t, QNRequest)]
        if not requests:
            return list(terms)
        return [self.observe(x, requests)] + [t for t in terms if not isinstance(t, QNRequest)]

    def counts(self):
        return self.memory.counts() if self.memory is not None else (0, 0)
