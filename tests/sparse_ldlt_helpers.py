"""Shared by the tests of SparseCholesky's LDLT mode: a numpy restatement of the no-pivot factorization
P A P^T = L S L^T (S = diag(+-1), positive diagonal of L) and the symmetric quasi-definite systems of the tests."""
import numpy as np

from sparse_chol_helpers import csc_from_triplets, grid3_triplets, mass_triplets, tridiag_triplets
from sparse_chol_packing_helpers import clique8_triplets

EPS = float(np.finfo(np.float64).eps)
PO_ERR_ARG = 2  # include/paropt_amd.h


# ---- the factorization restated --------------------------------------------------------------------------------------
def ldlt_nopivot(A):
    """(L, s, replaced) of the dense symmetric A in the order given, column by column as the device kernels do:
    s_k = sign(piv), l_kk = sqrt|piv|, l_ik = a_ik / (s_k l_kk), a_ij -= l_ik (s_k l_jk); a pivot that is exactly zero
    or NaN is replaced by +1 and listed in `replaced`."""
    W = np.array(A, dtype=np.float64)
    n = W.shape[0]
    L = np.zeros((n, n))
    s = np.ones(n)
    replaced = []
    for k in range(n):
        piv = W[k, k]
        if not (piv > 0.0 or piv < 0.0):
            replaced.append(k)
            piv = 1.0
        s[k] = -1.0 if piv < 0.0 else 1.0
        L[k, k] = np.sqrt(abs(piv))
        L[k + 1:, k] = W[k + 1:, k] / (s[k] * L[k, k])
        W[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], s[k] * L[k + 1:, k])
    return L, s, replaced


def ldlt_solve(L, s, b):
    """forward sweep with L, y_k <- s_k y_k, backward sweep with L^T"""
    from scipy.linalg import solve_triangular

    y = solve_triangular(L, b, lower=True)
    y = (y.T * s).T
    return solve_triangular(L.T, y, lower=False)


def inertia_of(s, replaced=()):
    """(positive, negative, replaced) as po_sparse_chol_inertia counts them"""
    neg = int((np.asarray(s) < 0).sum())
    return len(s) - neg - len(replaced), neg, len(replaced)


def eta(A, x, b):
    """the backward error of tests/test_gpu_sparse_chol.py"""
    return float(np.abs(b - A @ x).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def bound_for(A, b):
    """(the project's bound max(16 eta_LAPACK, 64 eps), eta_LAPACK), LAPACK = numpy.linalg.solve on the dense matrix"""
    e_lap = eta(A, np.linalg.solve(A, b), b)
    return max(16.0 * e_lap, 64.0 * EPS), e_lap


# ---- systems ---------------------------------------------------------------------------------------------------------
def dense_spd(n, seed):
    """tests/test_gpu_sparse_chol.py: dense_spd"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return G @ G.T / n + np.eye(n)


def dense_csc(A):
    """tests/test_gpu_sparse_chol.py: dense_csc"""
    n = A.shape[0]
    colp = (np.arange(n + 1) * n).astype(np.intc)
    rows = np.tile(np.arange(n, dtype=np.intc), n)
    return colp, rows, np.ascontiguousarray(A.T).ravel()


def dense_quasi_definite(n, seed):
    """[[E, B^T], [B, -F]] with E, F of the form G G^T / k + I (k their order), the negative block a third of the
    order, under a random symmetric permutation: every block column of the front holds both signs.  Returns (A, n2)."""
    rng = np.random.default_rng(seed)
    n2 = n // 3
    n1 = n - n2
    A = np.zeros((n, n))
    A[:n1, :n1] = dense_spd(n1, seed + 1)
    if n2 > 0:
        A[n1:, n1:] = -dense_spd(n2, seed + 2)
        B = rng.standard_normal((n2, n1)) / np.sqrt(n1)
        A[n1:, :n1] = B
        A[:n1, n1:] = B.T
    p = rng.permutation(n)
    return A[np.ix_(p, p)], n2


def flip_block(rows, colp, vals, neg):
    """The entries of an SPD matrix M (compressed columns) turned into those of [[M_PP, M_PN], [M_NP, -M_NN]], N the
    unknowns flagged in `neg`: symmetric quasi-definite, since M_PP and M_NN are principal blocks of an SPD matrix."""
    cols = np.repeat(np.arange(len(colp) - 1), np.diff(colp))
    neg = np.asarray(neg, dtype=bool)
    return np.where(neg[rows] & neg[cols], -vals, vals)


def grid3_system(dims, seed):
    """tests/test_gpu_sparse_chol.py: grid3_system"""
    n, R, C = grid3_triplets(*dims)
    rng = np.random.default_rng(seed)
    V = np.where(R == C, 0.0, -0.5)
    V[R == C] = 4.0 + 0.1 * rng.random(n)
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    return n, colp, rows, vals


def grid3_odd(dims):
    """the nodes (i, j, k) of the grid with i + j + k odd: no two of them are neighbours, nor two of the others"""
    i, j, k = np.unravel_index(np.arange(int(np.prod(dims))), dims)
    return (i + j + k) % 2 == 1


def grid3_quasi_definite(dims, seed=7):
    """grid3_system with the diagonal entry of every odd node negated: both diagonal blocks are diagonal and positive"""
    n, colp, rows, vals = grid3_system(dims, seed)
    odd = grid3_odd(dims)
    return n, colp, rows, flip_block(rows, colp, vals, odd), odd


def tridiag_quasi_definite(n):
    """tridiag_triplets(n) with the diagonal negated at the odd indices"""
    n, R, C, V = tridiag_triplets(n)
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    odd = np.arange(n) % 2 == 1
    return n, colp, rows, flip_block(rows, colp, vals, odd), odd


def clique8_quasi_definite(seed=3):
    """The clique8 pattern of the packing tests (natural order) with mixed signs: a strictly diagonally dominant
    matrix on the pattern, the block of vertex 1 and of the clique's vertices 3, 5, 6, 9 negated."""
    n, R, C = clique8_triplets()
    colp, rows = csc_from_triplets(n, R, C)
    cols = np.repeat(np.arange(n), np.diff(colp))
    W = np.random.default_rng(seed).uniform(0.1, 1.0, size=(n, n))
    W = W + W.T
    off = np.zeros((n, n))
    off[rows, cols] = -W[rows, cols]
    np.fill_diagonal(off, 0.0)
    diag = np.abs(off).sum(axis=1) + 1.0 + W.diagonal()
    vals = np.where(rows == cols, diag[rows], -W[rows, cols])
    neg = np.zeros(n, dtype=bool)
    neg[[1, 3, 5, 6, 9]] = True
    return n, colp, rows, flip_block(rows, colp, vals, neg), neg


def zero_pivot_system():
    """[[4, 2, 0], [2, 1, 1], [0, 1, 3]] as the first three unknowns of the tridiagonal of 40: in the natural order the
    second pivot is exactly 1 - 2 * 2 / 4 = 0.  Returns (n, colp, rows, vals, SPD vals of the same pattern)."""
    n, R, C, V = tridiag_triplets(40)
    colp, rows, spd = csc_from_triplets(n, R, C, V)
    cols = np.repeat(np.arange(n), np.diff(colp))
    head = np.array([[4.0, 2.0, 0.0], [2.0, 1.0, 1.0], [0.0, 1.0, 3.0]])
    vals = spd.copy()
    inside = (rows < 3) & (cols < 3)
    vals[inside] = head[rows[inside], cols[inside]]
    return n, colp, rows, vals, spd


PATCH, WEIGHT, DELTA = 2, 0.25, 1.0  # examples/sparse_ldlt_amd.cpp


def bordered_mass_system(nx):
    """K = [[M, B^T], [B, -DELTA I]] of examples/sparse_ldlt_amd.cpp, dense: M the mass matrix of mass_triplets(nx), one
    row of B per PATCH x PATCH patch of nodes with WEIGHT on every unknown of the patch.  Returns (K, rows of M)."""
    nm, R, C, V = mass_triplets(nx)
    side = nx + 1
    pside = (side + PATCH - 1) // PATCH
    n = nm + pside * pside
    K = np.zeros((n, n))
    np.add.at(K, (R, C), V)
    for ny in range(side):
        for nxi in range(side):
            con = nm + nxi // PATCH + (ny // PATCH) * pside
            for dof in range(2):
                u = 2 * (nxi + ny * side) + dof
                K[con, u] = K[u, con] = WEIGHT
    K[np.arange(nm, n), np.arange(nm, n)] = -DELTA
    return K, nm
