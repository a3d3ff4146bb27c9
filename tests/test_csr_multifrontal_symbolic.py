"""Host analysis of the CSR sparse constraints for the multifrontal engine (CsrSymbolic(..., sparse_factor=
"multifrontal"), paropt_amd/csrc/csr.cpp: analyse_multifrontal).  No device.

  * the elimination order is the engine's own: SparseCholesky(None, lower(S0), order="nd").perm;
  * the assembly table (a, b) -> offset in the engine's L has one distinct destination inside the panels per
    structural entry of lower(S0), and placing the values of a dense random SPD S through it gives the L array that the
    engine's own value scatter of the same values gives (the engine reads whichever copy of an entry lies in the lower
    triangle after the permutation, so it is given both and the table names that copy);
  * with dense columns the table describes S0 and dense_pos follows the new order;
  * the row factor's accessors refuse a multifrontal handle (and the frontal ones a row handle), an unknown kind is
    refused.

SHAPES is shared with tests/test_gpu_csr_multifrontal.py: the supernode counts, levels and front sizes the patterns
were chosen for (they straddle kCholSmall = kCholNB = 32 and kCholTile = 64) are asserted here and there."""
import ctypes as C

import numpy as np
import pytest

from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern, grid_pattern, random_pattern

# name -> (n, rowp, cols); SHAPES[name] = (w, supernodes, levels, largest supernode, largest front)
PATTERNS = {
    "chain2": lambda: (300, *chain_pattern(300, 2, 1)),
    "grid_12_11": lambda: (12 * 11, *grid_pattern(12, 11)),
    "long_rows": lambda: (600, *random_pattern(600, 40, 150, 3)),
    "grid_26_24": lambda: (26 * 24, *grid_pattern(26, 24)),
    "grid_40_40": lambda: (40 * 40, *grid_pattern(40, 40)),
    "empty_rows": lambda: (50, np.array([0, 0, 2, 2, 3, 3], dtype=np.intc), np.array([4, 1, 4], dtype=np.intc)),
    "w0": lambda: (5, np.array([0], dtype=np.intc), np.zeros(0, dtype=np.intc)),
    "w1": lambda: (5, np.array([0, 2], dtype=np.intc), np.array([3, 1], dtype=np.intc)),
}
PO_ERR_ARG = 2  # include/paropt_amd.h
SHAPES = {
    "chain2": (299, 298, 13, 2, 3),
    "grid_12_11": (241, 131, 11, 21, 31),
    "long_rows": (40, 5, 4, 31, 37),
    "grid_26_24": (1198, 623, 14, 47, 71),
    "grid_40_40": (3120, 1599, 16, 78, 117),
    "empty_rows": (5, 4, 1, 2, 2),
    "w0": (0, 0, 0, 0, 0),
    "w1": (1, 1, 1, 1, 1),
}


def assert_shape(name, sym):
    """the symbolic facts a pattern was chosen for: an analysis change that moves them fails loudly"""
    got = (len(sym.perm), sym.num_snodes, sym.nlevels, sym.max_snode, sym.max_front)
    assert got == SHAPES[name], (name, got, SHAPES[name])


def lower_s0(n, rowp, cols, dense=()):
    """lower(S0) in compressed columns (both arrays int32) and the boolean pattern of S0, S0 = pattern of As As^T"""
    w = len(rowp) - 1
    B = np.zeros((w, n), dtype=bool)
    for i in range(w):
        B[i, cols[rowp[i]:rowp[i + 1]]] = True
    B[:, list(dense)] = False
    Bi = B.astype(np.int64)
    pat = (Bi @ Bi.T) > 0
    pat[np.arange(w), np.arange(w)] = True
    colp, rows = [0], []
    for j in range(w):
        rows += [int(i) for i in np.nonzero(pat[j:, j])[0] + j]
        colp.append(len(rows))
    return np.array(colp, dtype=np.intc), np.array(rows, dtype=np.intc), pat


def check_table(sym, pat, seed):
    w = len(sym.perm)
    a, b, dst = sym.ent_a, sym.ent_b, sym.ent_dst
    colp, rows, aptr, asrc, adst, lsize = sym.frontal_scatter()
    # one destination per structural lower entry, all distinct, all inside the panels
    assert len(a) == int(np.tril(pat).sum()) == sym.nnzS
    assert np.all(pat[a, b])
    assert len(set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))) == len(a)  # one per unordered pair
    assert len(np.unique(dst)) == len(dst)
    assert len(dst) == 0 or (dst.min() >= 0 and dst.max() < lsize)
    # a dense random SPD S through the table against the engine's scatter of the same values
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((w, w))
    S = G @ G.T + w * np.eye(w)
    L1 = np.zeros(lsize)
    L1[dst] = S[a, b]
    col_of = np.repeat(np.arange(w), np.diff(colp))
    vals = S[rows, col_of]
    L2 = np.zeros(lsize)
    for d in range(len(adst)):
        L2[adst[d]] = vals[asrc[aptr[d]:aptr[d + 1]]].sum()
    np.testing.assert_array_equal(L1, L2)
    # the position itself, from the supernode layout: the diagonal of column perm^-1 sits at the head of its column
    iperm = np.empty(w, dtype=np.int64)
    iperm[sym.perm] = np.arange(w)
    diag = {int(a[e]): int(dst[e]) for e in range(len(a)) if a[e] == b[e]}
    assert sorted(diag) == list(range(w))
    order = [diag[int(sym.perm[k])] for k in range(w)]
    assert order == sorted(order)  # columns of L are stored in elimination order


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_order_and_assembly_table(name):
    import paropt_amd as pa

    n, rowp, cols = PATTERNS[name]()
    w = len(rowp) - 1
    sym = pa.CsrSymbolic(n, rowp, cols, sparse_factor="multifrontal")
    assert_shape(name, sym)
    assert sorted(sym.perm.tolist()) == list(range(w))
    colp, rows, pat = lower_s0(n, rowp, cols)
    eng = pa.SparseCholesky(None, w, colp, rows, order="nd")
    np.testing.assert_array_equal(sym.perm, eng.perm)
    assert (sym.num_snodes, sym.nnzL, sym.nlevels) == (eng.num_snodes, eng.nnzL, eng.nlevels)
    np.testing.assert_array_equal(sym.snode_first, eng.snode_first)
    assert sym.nnz == int(rowp[-1])
    check_table(sym, pat, 7)
    # the row analysis of the same pattern is another order with (about) the same fill
    row = pa.CsrSymbolic(n, rowp, cols)
    assert row.nnzS == sym.nnzS
    if name not in ("long_rows",):
        assert row.nnzL == sym.nnzL


def test_dense_columns_follow_the_new_order():
    import paropt_amd as pa

    n, rowp, cols = add_dense_columns(624, *grid_pattern(26, 24), 2)
    sym = pa.CsrSymbolic(n, rowp, cols, dense_column_rows=600, sparse_factor="multifrontal")
    assert sym.dense_cols == [624, 625]
    assert_shape("grid_26_24", sym)  # S0 is the grid's own Schur complement
    colp, rows, pat = lower_s0(n, rowp, cols, dense=sym.dense_cols)
    np.testing.assert_array_equal(sym.perm, pa.SparseCholesky(None, len(rowp) - 1, colp, rows, order="nd").perm)
    plain = pa.CsrSymbolic(624, *grid_pattern(26, 24), sparse_factor="multifrontal")
    np.testing.assert_array_equal(sym.perm, plain.perm)
    np.testing.assert_array_equal(sym.ent_dst, plain.ent_dst)
    check_table(sym, pat, 8)
    # dense_pos = iperm[row] in the multifrontal order: the problem object shows it through its solves (GPU tests);
    # here the order itself differs from the row factor's, so a stale dense_pos could not go unnoticed there
    row = pa.CsrSymbolic(n, rowp, cols, dense_column_rows=600)
    assert not np.array_equal(row.perm, sym.perm)


def test_accessors_match_the_handle_and_unknown_kinds_are_refused():
    import paropt_amd as pa
    from paropt_amd import lib as L
    from paropt_amd.lib import ParOptAMDError

    n, rowp, cols = PATTERNS["grid_12_11"]()
    mf = pa.CsrSymbolic(n, rowp, cols, sparse_factor="multifrontal")
    row = pa.CsrSymbolic(n, rowp, cols)
    info7, info8 = (C.c_int64 * 7)(), (C.c_int64 * 8)()
    none6 = [None] * 6
    cnt, names, levels = C.c_int(), C.POINTER(C.c_char_p)(), L.c_int_p()
    assert L.lib.po_csr_symbolic_info(mf._h, info7) == PO_ERR_ARG
    assert "row factor" in L.lib.po_last_error().decode()
    assert L.lib.po_csr_symbolic_arrays(mf._h, *none6) == PO_ERR_ARG
    assert L.lib.po_csr_symbolic_kernel_forms(mf._h, 1, C.byref(cnt), C.byref(names), C.byref(levels)) == PO_ERR_ARG
    with pytest.raises(ParOptAMDError, match="row factor"):
        mf.kernel_forms(1)
    assert L.lib.po_csr_symbolic_frontal_info(row._h, info8) == PO_ERR_ARG
    assert L.lib.po_csr_symbolic_frontal_arrays(row._h, *none6, None, None) == PO_ERR_ARG
    assert L.lib.po_csr_symbolic_frontal_info(mf._h, info8) == 0 and info8[1] == mf.num_snodes
    # an unknown kind
    h = L.po_csr_symbolic()
    rp, cl = np.ascontiguousarray(rowp), np.ascontiguousarray(cols)
    rc = L.lib.po_csr_symbolic_create_factor(n, len(rowp) - 1, rp.ctypes.data_as(L.c_int_p),
                                             cl.ctypes.data_as(L.c_int_p), 0, 7, C.byref(h))
    assert rc == PO_ERR_ARG and "unknown sparse factor kind 7" in L.lib.po_last_error().decode()
    with pytest.raises(ValueError, match="sparse_factor"):
        pa.CsrSymbolic(n, rowp, cols, sparse_factor="supernodal")
    # the existing entries keep their meaning: _create_split is the row factor
    assert row.nfronts >= 0 and row.sparse_factor == "rows"
