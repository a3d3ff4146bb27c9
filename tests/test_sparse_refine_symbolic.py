"""SparseCholesky's retained matrix without a device: the table behind matrix_arrays() on analysis-only handles.

The table and a numpy restatement of the compaction (every kept entry -- iperm[row] >= iperm[col] -- summed in entry
order into the value its position carries) must give back, exactly, the matrix the value scatter puts into the factor:
the definition of A.  For a symmetric input that is the input; for a lower-triangle-only input under an ordering that
moves entries across the diagonal it is what the rule keeps, not the symmetrised input."""
import ctypes as C

import numpy as np
import pytest

from sparse_chol_helpers import (csc_from_triplets, dense_from_csc, forest_triplets, mass_triplets, tridiag_triplets)
from sparse_ldlt_helpers import PO_ERR_ARG
from sparse_refine_helpers import compact_values, dense_from_table, kept_dense


def lower_only():
    n, R, Cc, V = tridiag_triplets(40)
    low = R >= Cc
    return n, R[low], Cc[low], V[low]


CASES = {
    "tridiag_natural": (lambda: tridiag_triplets(40), "natural"),
    "tridiag_nd": (lambda: tridiag_triplets(40), "nd"),
    "mass3": (lambda: mass_triplets(3), "nd"),
    "forest": (forest_triplets, "nd"),
    "lower_only_nd": (lower_only, "nd"),
}


def analysed(name):
    import paropt_amd as pa

    make, order = CASES[name]
    n, R, Cc, V = make()
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    return pa.SparseCholesky(None, n, colp, rows, order=order, keep_matrix=True), n, colp, rows, vals


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_and_compaction_reproduce_the_matrix(name):
    s, n, colp, rows, vals = analysed(name)
    assert s.keep_matrix
    table = s.matrix_arrays()
    rowp, col, vidx, nd = table
    assert rowp[0] == 0 and len(rowp) == n + 1 and len(col) == len(vidx) == rowp[-1]
    r = np.repeat(np.arange(n), np.diff(rowp))
    # rows sorted by column, no position twice
    for i in range(n):
        c = col[rowp[i]:rowp[i + 1]]
        assert (np.diff(c) > 0).all(), (name, i)
    # the two copies of an off-diagonal entry share a value index; a diagonal entry has one copy
    pos = {(int(i), int(j)): int(d) for i, j, d in zip(r, col, vidx)}
    for (i, j), d in pos.items():
        assert pos[(j, i)] == d
    assert len(col) == 2 * nd - int((r == col).sum())
    assert vidx.min() == 0 and vidx.max() == nd - 1
    aval = compact_values(s.perm, colp, rows, vals, table)
    P = dense_from_table(n, rowp, col, vidx, aval)
    A = np.zeros((n, n))
    A[np.ix_(s.perm, s.perm)] = P
    want = kept_dense(s.perm, colp, rows, vals)
    assert np.array_equal(A, want), name
    assert np.array_equal(A, A.T)
    full = dense_from_csc(n, colp, rows, vals)
    if name == "lower_only_nd":
        iperm = np.argsort(s.perm)
        moved = [(i, j) for i, j in zip(rows, np.repeat(np.arange(n), np.diff(colp))) if iperm[i] < iperm[j]]
        assert moved  # the ordering does move entries across the diagonal: those are not read
        assert not np.array_equal(A, np.tril(full) + np.tril(full, -1).T)
        for i, j in moved:
            assert A[i, j] == 0.0 and A[j, i] == 0.0
    else:
        assert np.array_equal(A, full), name  # (sums of equal terms in the same order: exact)


def test_keep_matrix_round_trips_and_numeric_entries_are_refused():
    import paropt_amd as pa
    from paropt_amd.lib import lib

    n, R, Cc, V = tridiag_triplets(40)
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    s = pa.SparseCholesky(None, n, colp, rows)
    assert not s.keep_matrix
    with pytest.raises(pa.ParOptAMDError) as e:
        s.matrix_arrays()
    assert e.value.code == PO_ERR_ARG and "keep_matrix" in str(e.value)
    s.set_keep_matrix(True)
    assert s.keep_matrix
    first = s.matrix_arrays()
    s.set_keep_matrix(False)
    assert not s.keep_matrix
    s.set_keep_matrix(True)
    again = s.matrix_arrays()
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    on = C.c_int(-1)
    assert lib.po_sparse_chol_get_keep_matrix(s.handle, C.byref(on)) == 0 and on.value == 1
    # NULL handles
    assert lib.po_sparse_chol_set_keep_matrix(None, 1) == PO_ERR_ARG
    assert lib.po_sparse_chol_get_keep_matrix(None, C.byref(on)) == PO_ERR_ARG
    assert lib.po_sparse_chol_matrix_arrays(None, None, None, None, None) == PO_ERR_ARG
    assert lib.po_sparse_chol_set_diagonal_shift(None, None) == PO_ERR_ARG
    assert lib.po_sparse_chol_matvec(None, None, 0, None, 0, 1) == PO_ERR_ARG
    assert lib.po_sparse_chol_matvec_device(None, None, 0, None, 0, 1) == PO_ERR_ARG
    assert lib.po_sparse_chol_solve_refined(None, None, 1, 0, 5, -1.0, None, None, None) == PO_ERR_ARG
    assert lib.po_sparse_chol_solve_refined_device(None, None, 1, 0, 5, -1.0, None, None, None) == PO_ERR_ARG
    # the numeric entries on an analysis-only handle
    x = np.ones(n)
    for call in (lambda: s.set_diagonal_shift(np.zeros(n)), lambda: s.set_diagonal_shift(None), lambda: s.matvec(x),
                 lambda: s.solve_refined(x)):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG and "analysis-only" in str(e.value)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.po_sparse_chol_matvec_device(s.handle, xp, n, xp, n, 1) == PO_ERR_ARG
    assert lib.po_sparse_chol_solve_refined_device(s.handle, xp, 1, n, 5, -1.0, None, None, None) == PO_ERR_ARG
    assert b"analysis-only" in lib.po_last_error()
    with pytest.raises(ValueError):
        s.set_diagonal_shift(np.zeros(n + 1))
