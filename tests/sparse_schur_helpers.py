"""Shared by the tests of SparseCholesky's Schur complement: a numpy restatement of the no-pivot PARTIAL elimination in
the handle's own elimination order, the dense formula S = A22 - A21 A11^-1 A12 with its error measure d(S), and the
systems of the tests."""
import json
import os

import numpy as np

from sparse_ldlt_helpers import EPS

PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                      "r27_sparse_schur_parity.json")


# ---- the partial elimination restated ----------------------------------------------------------------------------------
def partial_nopivot(A, perm, ns):
    """(S, signs) after eliminating the first n - ns unknowns of A[perm][:, perm] column by column as the device
    kernels do (sparse_ldlt_helpers.ldlt_nopivot stopped early): s_k = sign(piv), l_kk = sqrt|piv|,
    l_ik = a_ik / (s_k l_kk), a_ij -= l_ik (s_k l_jk).  With positive pivots it is the Cholesky elimination.  What is
    left in the last ns rows and columns is S, in the order perm lists the set."""
    W = np.array(A, dtype=np.float64)[np.ix_(perm, perm)]
    n = W.shape[0]
    signs = np.ones(n - ns)
    for k in range(n - ns):
        piv = W[k, k]
        signs[k] = -1.0 if piv < 0.0 else 1.0
        lkk = np.sqrt(abs(piv))
        col = W[k + 1:, k] / (signs[k] * lkk)
        W[k + 1:, k + 1:] -= np.outer(col, signs[k] * col)
    return W[n - ns:, n - ns:].copy(), signs


def schur_dense(A, idx):
    """(S_ref, scale, interior) by numpy.linalg.solve on the dense matrix: S_ref = A22 - A21 A11^-1 A12 in the order of
    idx and scale = max(|A22| + |A21| |A11^-1 A12|), the size of the terms S is the difference of."""
    n = A.shape[0]
    idx = np.asarray(idx, dtype=int)
    interior = np.setdiff1d(np.arange(n), idx)
    A22 = A[np.ix_(idx, idx)]
    if len(interior) == 0:
        return A22.copy(), float(np.abs(A22).max()), interior
    A11, A12, A21 = A[np.ix_(interior, interior)], A[np.ix_(interior, idx)], A[np.ix_(idx, interior)]
    X = np.linalg.solve(A11, A12)
    return A22 - A21 @ X, float((np.abs(A22) + np.abs(A21) @ np.abs(X)).max()), interior


def d_measure(S, S_ref, scale):
    return float(np.abs(S - S_ref).max() / scale)


def d_bound(A, idx, perm):
    """(bound, d_restate): max(16 d_restate, 64 eps), d_restate the measure of the host restatement in the handle's
    elimination order"""
    S_ref, scale, _ = schur_dense(A, idx)
    S_host, _ = partial_nopivot(A, perm, len(idx))
    d_restate = d_measure(S_host, S_ref, scale)
    return max(16.0 * d_restate, 64.0 * EPS), d_restate


def inertia_dense(M):
    """(positive, negative, zero) eigenvalues of the symmetric M"""
    w = np.linalg.eigvalsh(M) if M.shape[0] > 0 else np.zeros(0)
    return int((w > 0).sum()), int((w < 0).sum()), int((w == 0).sum())


# ---- systems -------------------------------------------------------------------------------------------------------------
def fanin_kkt(nblocks, order, ncon, delta=1.0, seed=5):
    """[[E, B^T], [B, -delta I]] with E block-diagonal, nblocks SPD blocks of the given order, and ncon constraints
    that each touch every block: reduced onto the constraints, every block is a child of the Schur supernode.
    Returns (K, nE), K dense."""
    rng = np.random.default_rng(seed)
    nE = nblocks * order
    n = nE + ncon
    K = np.zeros((n, n))
    for b in range(nblocks):
        G = rng.standard_normal((order, order))
        K[b * order:(b + 1) * order, b * order:(b + 1) * order] = G @ G.T / order + np.eye(order)
    B = rng.uniform(0.1, 1.0, size=(ncon, nE)) / np.sqrt(nE)
    K[nE:, :nE] = B
    K[:nE, nE:] = B.T
    K[np.arange(nE, n), np.arange(nE, n)] = -delta
    return K, nE


RECORDS = {}


def record(name, **values):
    """a measured value of the GPU tests; write_records() puts them all into profiles/r27_sparse_schur_parity.json"""
    RECORDS[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in values.items()}
    print(name, RECORDS[name])


def write_records():
    with open(PARITY, "w") as f:
        json.dump({"eps": EPS, "bounds": {"d": "d(S) <= max(16 d_restate, 64 eps)",
                                          "eta": "eta <= max(16 eta_lapack, 64 eps)"}, "cases": RECORDS}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
