"""numpy model of the host side of ``NestedDissectionNormalSolver`` (ipsolver/nested.py,
csrc/nested_order.hip): the nested-dissection order and the supernodal symbolic factorization as
include/ipx.h specifies them.  Plain Python and slow on purpose: what the library is compared with.
"""
import numpy as np
import scipy.sparse as sps


def pattern_of_aat(A):
    """Pattern of S = A A' as CSR with sorted columns (the diagonal included)."""
    B = sps.csr_matrix((np.ones(A.nnz, dtype=np.float32), A.indices, A.indptr), shape=A.shape)
    S = sps.csr_matrix(B.dot(B.T))
    S.sort_indices()
    return S


def _levels(indptr, indices, inside, start):
    """Breadth-first level of every row reached from ``start`` inside the part -> (rows in the
    order reached, their levels)."""
    seen = {start: 0}
    order = [start]
    head = 0
    while head < len(order):
        i = order[head]
        head += 1
        for j in indices[indptr[i]:indptr[i + 1]]:
            if j in inside and j not in seen:
                seen[j] = seen[i] + 1
                order.append(j)
    return order, [seen[i] for i in order]


def order(indptr, indices, leaf):
    """-> (perm: new position -> row, sn_ptr: the supernodes' ranges of positions).

    A part (ascending rows) of at most ``leaf`` rows is one supernode.  A larger part goes piece
    by piece, the connected pieces in the order of their lowest rows; a connected part larger than
    ``leaf``: breadth-first levels from its lowest row, restarted twice from the lowest row of the
    last level; fewer than three levels: one supernode; else the separator is the first level at
    which the cumulative count reaches half the part (ceiling), clamped to 1 ... levels - 2; the
    rows before it, the rows after it, then the separator."""
    n = len(indptr) - 1
    perm, sn_ptr = [], [0]

    def emit(rows):
        perm.extend(sorted(rows))
        sn_ptr.append(len(perm))

    def dissect(rows):
        if len(rows) <= leaf:
            return emit(rows)
        inside = set(rows)
        reached, lev = _levels(indptr, indices, inside, rows[0])
        if len(reached) < len(rows):                    # not connected: piece by piece
            left = inside
            while left:
                piece, _ = _levels(indptr, indices, left, min(left))
                left = left - set(piece)
                dissect(sorted(piece))
            return
        for _ in range(2):
            last = [i for i, l in zip(reached, lev) if l == lev[-1]]
            reached, lev = _levels(indptr, indices, inside, min(last))
        nlev = lev[-1] + 1
        if nlev < 3:
            return emit(rows)
        counts = np.cumsum(np.bincount(lev, minlength=nlev))
        cut = int(np.argmax(counts >= (len(rows) + 1) // 2))
        cut = min(max(cut, 1), nlev - 2)
        dissect(sorted(i for i, l in zip(reached, lev) if l < cut))
        dissect(sorted(i for i, l in zip(reached, lev) if l > cut))
        emit([i for i, l in zip(reached, lev) if l == cut])

    if n:
        dissect(list(range(n)))
    return np.array(perm, dtype=np.int32), np.array(sn_ptr, dtype=np.int32)


def symbolic(indptr, indices, perm, sn_ptr):
    """-> (parent, level, bnd_ptr, bnd, cmap).  ``bnd``: per supernode the later positions it
    couples to after fill, ascending; ``parent``: the owner of the first of them (-1: a root);
    ``level``: 0 for a supernode without children, else one more than the highest child's;
    ``cmap``: beside every boundary position its index in the parent's front (the parent's own
    positions, then its boundary)."""
    n, ns = len(perm), len(sn_ptr) - 1
    pos = np.empty(n, dtype=np.int64)
    pos[perm] = np.arange(n)
    owner = np.repeat(np.arange(ns), np.diff(sn_ptr))
    parent = np.full(ns, -1, dtype=np.int32)
    level = np.zeros(ns, dtype=np.int32)
    children = [[] for _ in range(ns)]
    bnds = []
    for j in range(ns):
        end = sn_ptr[j + 1]
        b = set()
        for p in range(sn_ptr[j], end):
            i = perm[p]
            b.update(q for q in pos[indices[indptr[i]:indptr[i + 1]]] if q >= end)
        for c in children[j]:
            b.update(q for q in bnds[c] if q >= end)
            level[j] = max(level[j], level[c] + 1)
        b = sorted(b)
        bnds.append(b)
        if b:
            parent[j] = owner[b[0]]
            children[parent[j]].append(j)
    bnd_ptr = np.concatenate(([0], np.cumsum([len(b) for b in bnds]))).astype(np.int64)
    bnd = np.array([q for b in bnds for q in b], dtype=np.int32)
    cmap = np.empty(len(bnd), dtype=np.int32)
    for j in range(ns):
        p = parent[j]
        if p < 0:
            continue
        front = list(range(sn_ptr[p], sn_ptr[p + 1])) + bnds[p]
        where = {q: k for k, q in enumerate(front)}
        cmap[bnd_ptr[j]:bnd_ptr[j + 1]] = [where[q] for q in bnds[j]]
    return parent, level, bnd_ptr, bnd, cmap


def random_sparse(m=300, n=420, seed=5):
    """A random sparse A (entries +-1, then ``2^-3 I`` beside it) whose A A' fills heavily."""
    rng = np.random.default_rng(seed)
    G = sps.random(m, n, density=0.012, random_state=rng, format="csr",
                   data_rvs=lambda k: rng.choice([-1.0, 1.0], size=k))
    A = sps.hstack((G, 0.125 * sps.identity(m)), format="csr")
    A.sort_indices()
    return A
