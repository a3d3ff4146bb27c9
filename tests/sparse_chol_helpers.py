"""Patterns and a numpy symbolic factorization shared by the sparse Cholesky tests."""
import numpy as np

KE = np.array([[4.0, 2.0, 2.0, 1.0], [2.0, 4.0, 1.0, 2.0], [2.0, 1.0, 4.0, 2.0], [1.0, 2.0, 2.0, 4.0]]) / 9.0


def mass_triplets(nx):
    """Bilinear mass matrix of an nx x nx mesh of four-node elements, two unknowns per node, element by element
    (entries shared by elements are repeated, not summed)."""
    n = 2 * (nx + 1) ** 2
    R, C, V = [], [], []
    for i in range(nx):
        for j in range(nx):
            nodes = [i + j * (nx + 1), i + 1 + j * (nx + 1), i + (j + 1) * (nx + 1), i + 1 + (j + 1) * (nx + 1)]
            for k in range(2):
                for a in range(4):
                    for b in range(4):
                        R.append(2 * nodes[a] + k)
                        C.append(2 * nodes[b] + k)
                        V.append(KE[a, b])
    return n, np.array(R), np.array(C), np.array(V)


def grid3_triplets(nx, ny, nz):
    """pattern of the 7-point stencil, every entry once"""
    ids = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    R, C = [ids.ravel()], [ids.ravel()]
    for a, b in ((ids[:-1], ids[1:]), (ids[:, :-1], ids[:, 1:]), (ids[:, :, :-1], ids[:, :, 1:])):
        R += [a.ravel(), b.ravel()]
        C += [b.ravel(), a.ravel()]
    return nx * ny * nz, np.concatenate(R), np.concatenate(C)


def tridiag_triplets(n):
    i = np.arange(n)
    R = np.concatenate([i, i[:-1], i[1:]])
    C = np.concatenate([i, i[1:], i[:-1]])
    V = np.concatenate([2.5 + 0.01 * (i % 7), -np.ones(n - 1), -np.ones(n - 1)])
    return n, R, C, V


def forest_triplets():
    """three blocks that share nothing: a chain of 30, a 7 x 6 five-point grid, a dense block of 9"""
    n1, R1, C1, V1 = tridiag_triplets(30)
    ids = np.arange(42).reshape(7, 6)
    R2, C2 = [ids.ravel()], [ids.ravel()]
    for a, b in ((ids[:-1], ids[1:]), (ids[:, :-1], ids[:, 1:])):
        R2 += [a.ravel(), b.ravel()]
        C2 += [b.ravel(), a.ravel()]
    R2, C2 = np.concatenate(R2), np.concatenate(C2)
    V2 = np.where(R2 == C2, 4.5, -1.0)
    G = np.random.default_rng(9).standard_normal((9, 9))
    D = G @ G.T / 9 + np.eye(9)
    R3, C3 = np.divmod(np.arange(81), 9)
    return (81, np.concatenate([R1, 30 + R2, 72 + R3]), np.concatenate([C1, 30 + C2, 72 + C3]),
            np.concatenate([V1, V2, D[R3, C3]]))


def csc_from_triplets(n, R, C, V=None):
    """compressed columns in the order the entries come (stable), duplicates kept"""
    order = np.argsort(C, kind="stable")
    colp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(colp, np.asarray(C) + 1, 1)
    colp = np.cumsum(colp).astype(np.intc)
    rows = np.asarray(R)[order].astype(np.intc)
    if V is None:
        return colp, rows
    return colp, rows, np.asarray(V, dtype=np.float64)[order]


def dense_from_csc(n, colp, rows, vals):
    A = np.zeros((n, n))
    cols = np.repeat(np.arange(n), np.diff(colp))
    np.add.at(A, (rows, cols), vals)
    return A


def symbolic_fill(n, colp, rows, perm):
    """(entries of the lower triangle of L, entries of each column of L) by a boolean dense Cholesky of the
    symmetrised, permuted pattern"""
    B = np.zeros((n, n), dtype=bool)
    cols = np.repeat(np.arange(n), np.diff(colp))
    B[rows, cols] = True
    B |= B.T
    B[np.arange(n), np.arange(n)] = True
    B = B[np.ix_(perm, perm)]
    for k in range(n):
        r = k + 1 + np.nonzero(B[k + 1:, k])[0]
        if len(r) > 1:
            B[np.ix_(r, r)] = True
    low = np.tril(B)
    return int(low.sum()), low.sum(axis=0)
