"""Shared by the tests of SparseCholesky's retained matrix, diagonal shift and refined solve: the numpy restatement of
the definition of A (the rule of the value scatter), of the compaction behind matrix_arrays(), of the refinement loop,
and the systems that need refinement."""
import numpy as np

from sparse_chol_helpers import csc_from_triplets
from sparse_ldlt_helpers import EPS, bordered_mass_system, ldlt_nopivot, ldlt_solve


# ---- the definition of A ---------------------------------------------------------------------------------------------
def kept_entries(perm, colp, rows):
    """(entry index, permuted row, permuted column) of the entries the value scatter reads: iperm[row] >= iperm[col]"""
    n = len(perm)
    iperm = np.empty(n, dtype=np.int64)
    iperm[np.asarray(perm)] = np.arange(n)
    cols = np.repeat(np.arange(n), np.diff(colp))
    pr, pc = iperm[np.asarray(rows)[:int(colp[-1])]], iperm[cols]
    keep = np.nonzero(pr >= pc)[0]
    return keep, pr[keep], pc[keep]


def kept_dense(perm, colp, rows, vals):
    """A in the caller's numbering: the kept entries summed at their place and mirrored"""
    n = len(perm)
    keep, pr, pc = kept_entries(perm, colp, rows)
    P = np.zeros((n, n))
    np.add.at(P, (pr, pc), np.asarray(vals)[keep])
    P = P + np.tril(P, -1).T
    A = np.zeros((n, n))
    A[np.ix_(perm, perm)] = P
    return A


def compact_values(perm, colp, rows, vals, table):
    """The compact value array restated from table = matrix_arrays(): the value index of a kept position is the one
    its lower-triangle copy carries in the table, and each value is the sum of its sources in entry order."""
    rowp, col, vidx, nd = table
    n = len(perm)
    r = np.repeat(np.arange(n), np.diff(rowp))
    low = r >= col
    assert sorted(vidx[low]) == list(range(nd))  # every value has exactly one lower-triangle copy
    where = {(int(i), int(j)): int(d) for i, j, d in zip(r[low], col[low], vidx[low])}
    keep, pr, pc = kept_entries(perm, colp, rows)
    aval = np.zeros(nd)
    for k, i, j in zip(keep, pr, pc):  # (entry order)
        aval[where[(int(i), int(j))]] += vals[k]
    return aval


def dense_from_table(n, rowp, col, vidx, aval):
    """the matrix in elimination order that the table and the compact values describe"""
    P = np.zeros((n, n))
    r = np.repeat(np.arange(n), np.diff(rowp))
    P[r, col] = aval[vidx]
    return P


# ---- refinement restated ---------------------------------------------------------------------------------------------
def eta_of(A, x, b):
    return float(np.abs(b - A @ x).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def refine_restated(A, shift, b, max_steps=5, tol=EPS):
    """The loop of solveRefinedDevice over ldlt_nopivot / ldlt_solve in the order given: (x, steps, [eta ...])"""
    L, s, _ = ldlt_nopivot(A + np.diag(shift))
    x = ldlt_solve(L, s, b)
    etas, k = [], 0
    while True:
        r = b - A @ x
        e = float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))
        etas.append(e)
        if not (e > tol) or k == max_steps or (k > 0 and not (e <= etas[-2] / 2)):
            return x, k, etas
        x = x + ldlt_solve(L, s, r)
        k += 1


# ---- systems that need it --------------------------------------------------------------------------------------------
def dense_to_csc(A):
    """compressed columns of the nonzero pattern of a dense symmetric matrix, with the whole diagonal"""
    n = A.shape[0]
    mask = (A != 0.0) | np.eye(n, dtype=bool)
    R, Cc = np.nonzero(mask)
    return csc_from_triplets(n, R, Cc, A[R, Cc])


def zero_corner_saddle(nx, delta=1e-6):
    """bordered_mass_system(nx) with the corner zeroed: (A, shift, nm); shift is -delta on the constraint rows"""
    K, nm = bordered_mass_system(nx)
    n = K.shape[0]
    K[np.arange(nm, n), np.arange(nm, n)] = 0.0
    shift = np.zeros(n)
    shift[nm:] = -delta
    return K, shift, nm


def singular_h_system(delta, n1=40, ncon=4):
    """[[H, B^T], [B, 0]] with H the Laplacian of the path graph (singular) and ncon rows of ten 0.25s: (A, shift, n1);
    shift is +delta on the first block and -delta on the constraint rows"""
    n = n1 + ncon
    A = np.zeros((n, n))
    i = np.arange(n1 - 1)
    A[i, i] += 1.0
    A[i + 1, i + 1] += 1.0
    A[i, i + 1] = A[i + 1, i] = -1.0
    per = n1 // ncon
    for c in range(ncon):
        A[n1 + c, c * per:(c + 1) * per] = A[c * per:(c + 1) * per, n1 + c] = 0.25
    shift = np.concatenate([np.full(n1, delta), np.full(ncon, -delta)])
    return A, shift, n1


def tiny_tridiagonal(n=40, eps=1e-10):
    """diag = +-eps alternating, off-diagonal 1: quasi-definite in the natural order, element growth 1 / eps"""
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, i] = np.where(i % 2 == 0, eps, -eps)
    A[i[:-1], i[:-1] + 1] = A[i[:-1] + 1, i[:-1]] = 1.0
    return A, np.zeros(n), (n + 1) // 2
