"""numpy model of the aggregate-block ("compact") and two-level preconditioners of
``IterativeNormalSolver`` (ipsolver/iterative.py, csrc/pcg.hip, csrc/aggregate.hip): the greedy
aggregation as include/ipx.h specifies it, the grouping of blocks into coarse rows, P, the
preconditioner as an explicit operator, and plain preconditioned CG.  Dense and slow on purpose:
what the device code is compared with.
"""
import numpy as np
import scipy.sparse as sps

BLOCK = 32


def aggregate_greedy(indptr, indices, cap):
    """Seeds in index order, assigned rows skipped; an aggregate starts as [seed]; its member list
    is walked from the head and every unassigned neighbour of a member, in the column order of
    its row, is appended and assigned at once while the aggregate has fewer than ``cap``
    members.  -> (agg, number of aggregates)"""
    n = len(indptr) - 1
    agg = np.full(n, -1, dtype=np.int32)
    count = 0
    for seed in range(n):
        if agg[seed] >= 0:
            continue
        members = [seed]
        agg[seed] = count
        head = 0
        while head < len(members) and len(members) < cap:
            i = members[head]
            head += 1
            for j in indices[indptr[i]:indptr[i + 1]]:
                if len(members) >= cap:
                    break
                if agg[j] < 0:
                    agg[j] = count
                    members.append(j)
        count += 1
    return agg, count


def pattern_of_aat(A):
    """Pattern of S = A A' as CSR with sorted columns (structural: no cancellation)."""
    B = sps.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    S = sps.csr_matrix(B.dot(B.T))
    S.sort_indices()
    return S


def quotient(S, agg, count):
    """Pattern of P'SP, P the indicator vectors of the aggregates."""
    m = S.shape[0]
    P = sps.csr_matrix((np.ones(m), (np.arange(m), agg)), shape=(m, count))
    Q = sps.csr_matrix(P.T.dot(S).dot(P))
    Q.sort_indices()
    return Q


class Aggregation:
    """Blocks of at most BLOCK rows; past ``coarse_max`` of them the coarse rows are groups of at
    most ``group = ceil(nblk / coarse_max)`` blocks, aggregated the same way on the quotient
    graph, and the blocks are renumbered so that each group's blocks are consecutive."""

    def __init__(self, A, coarse_max=4096, block=BLOCK):
        S = pattern_of_aat(A)
        agg, nblk = aggregate_greedy(S.indptr, S.indices, block)
        self.group = -(-nblk // coarse_max)
        if self.group > 1:
            Q = quotient(S, agg, nblk)
            of_block, ncoarse = aggregate_greedy(Q.indptr, Q.indices, self.group)
            by_group = np.argsort(of_block, kind="stable")
            renumber = np.empty(nblk, dtype=np.int32)
            renumber[by_group] = np.arange(nblk)
            agg, of_block = renumber[agg], of_block[by_group]
        else:
            of_block, ncoarse = np.arange(nblk), nblk
        self.agg, self.nblk, self.ncoarse = agg, nblk, ncoarse
        self.coarse_of = of_block[agg]
        m = A.shape[0]
        self.P = sps.csr_matrix((np.ones(m), (np.arange(m), self.coarse_of)), shape=(m, ncoarse))


def block_inverse(S, agg, nblk):
    """B^-1: the inverse of the diagonal blocks S[agg == b][:, agg == b], as a sparse matrix."""
    S = sps.csr_matrix(S)
    rows, cols, vals = [], [], []
    for b in range(nblk):
        idx = np.flatnonzero(agg == b)
        inv = np.linalg.inv(S[idx][:, idx].toarray())
        rows.append(np.repeat(idx, len(idx)))
        cols.append(np.tile(idx, len(idx)))
        vals.append(inv.ravel())
    m = S.shape[0]
    return sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                          shape=(m, m))


def preconditioner(A, ag, two_level=True):
    """r -> B^-1 r [+ P (P'SP)^-1 P'r] with S = A A'."""
    S = sps.csr_matrix(A.dot(A.T))
    Binv = block_inverse(S, ag.agg, ag.nblk)
    if not two_level:
        return lambda r: Binv.dot(r)
    P = ag.P
    X = np.linalg.inv(P.T.dot(S).dot(P).toarray())
    return lambda r: Binv.dot(r) + P.dot(X.dot(P.T.dot(r)))


def pcg(A, w, apply_M, rtol, maxit=2000):
    """Plain preconditioned CG on A A' v = w; -> (v, iterations until ||r|| <= rtol ||w||)."""
    S = sps.csr_matrix(A.dot(A.T))
    v, r = np.zeros_like(w), w.copy()
    z = apply_M(r)
    p, rz = z.copy(), r.dot(z)
    norm_w = np.linalg.norm(w)
    for it in range(1, maxit + 1):
        Sp = S.dot(p)
        alpha = rz / p.dot(Sp)
        v += alpha * p
        r -= alpha * Sp
        if np.linalg.norm(r) <= rtol * norm_w:
            return v, it
        z = apply_M(r)
        rz_next = r.dot(z)
        p = z + (rz_next / rz) * p
        rz = rz_next
    return v, maxit
