"""Shared by the dense-column tests of the CSR sparse constraints: patterns with extra variables that enter (nearly)
every row, and the numpy restatement of the low-rank solve
    S = S0 + V E V^T,  S0 = C + As D^-1 As^T = L L^T,  Yv = L^-1 V,  K = E^-1 + Yv^T Yv,
    S^-1 b = L^-T (t - Yv K^-1 Yv^T t),  t = L^-1 b."""
import numpy as np


def add_dense_columns(n, rowp, cols, r, first=False, fraction=1.0, seed=0):
    """Append r variables n .. n+r-1 to the pattern; each enters `fraction` of the rows (all of them at 1.0), listed
    first in the row (an unsorted row) or last.  Returns (n + r, rowp, cols)."""
    rng = np.random.default_rng(seed)
    w = len(rowp) - 1
    new_rowp, new_cols = [0], []
    member = np.ones((w, r), dtype=bool) if fraction >= 1.0 else rng.random((w, r)) < fraction
    for i in range(w):
        own = [int(c) for c in cols[rowp[i]:rowp[i + 1]]]
        extra = [n + j for j in range(r) if member[i, j]]
        new_cols += (extra[::-1] + own) if first else (own + extra)
        new_rowp.append(len(new_cols))
    return n + r, np.array(new_rowp, dtype=np.intc), np.array(new_cols, dtype=np.intc)


def split_matrices(A, d, c, dense_cols):
    """(S, S0, V, E) of the quasi-definite system with Jacobian A, D^-1 = diag(d), C = diag(c)."""
    J = np.asarray(dense_cols, dtype=int)
    keep = np.ones(A.shape[1], dtype=bool)
    keep[J] = False
    S = np.diag(c) + (A * d) @ A.T
    S0 = np.diag(c) + (A[:, keep] * d[keep]) @ A[:, keep].T
    return S, S0, A[:, J], d[J]


def woodbury_solve(L, perm, V, E, b):
    """S^-1 b from the factor L of P S0 P^T (perm[new] = old), dense triangular solves."""
    from numpy.linalg import solve

    t = solve(L, b[perm])
    if V.shape[1] > 0:
        Yv = solve(L, V[perm])
        K = np.diag(1.0 / E) + Yv.T @ Yv
        t = t - Yv @ solve(K, Yv.T @ t)
    y = solve(L.T, t)
    out = np.empty_like(y)
    out[perm] = y
    return out
