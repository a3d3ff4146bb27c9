"""The host analysis of pa.SparseCholesky with a Schur set, on analysis-only handles (no device): the set is ordered
last in the caller's order as one final supernode that nothing else joins, the ordering type applies to the interior,
the fill is that of the pattern plus the set as a clique, the Schur supernode is in no packed group; ns = 0 is the
plain analysis and ns = n works; refusals.  The numpy restatement of the partial elimination that the GPU tests take
their bound from (sparse_schur_helpers.partial_nopivot) is checked against the dense formula here."""
import ctypes as C

import numpy as np
import pytest

from sparse_chol_helpers import (csc_from_triplets, dense_from_csc, forest_triplets, grid3_triplets, mass_triplets,
                                 symbolic_fill, tridiag_triplets)
from sparse_chol_packing_helpers import pack_cap
from sparse_ldlt_helpers import EPS, PO_ERR_ARG
from sparse_schur_helpers import d_measure, partial_nopivot, schur_dense


def pattern(name):
    if name == "tridiag":
        n, R, Cc, _ = tridiag_triplets(40)
    elif name == "grid3":
        n, R, Cc = grid3_triplets(5, 4, 3)
    elif name == "forest":
        n, R, Cc, _ = forest_triplets()
    else:
        n, R, Cc, _ = mass_triplets(4)
    colp, rows = csc_from_triplets(n, R, Cc)
    return n, colp, rows


def schur_sets(name, n):
    rng = np.random.default_rng(len(name))
    sets = {"one": [n // 3], "scattered8": [int(v) for v in rng.permutation(n)[:8]],
            "many33": [int(v) for v in rng.permutation(n)[:33]]}
    assert sets["scattered8"] != sorted(sets["scattered8"])  # given unsorted
    if name == "grid3":
        sets["plane"] = [int(v) for v in np.arange(60).reshape(5, 4, 3)[2].ravel()]  # splits the grid in two
    if name == "forest":
        sets["in_grid_block"] = [30 + int(v) for v in np.arange(42).reshape(7, 6)[3]]  # inside one component
    return sets


CASES = [(name, key) for name in ("tridiag", "grid3", "forest", "mass4")
         for key in ("one", "scattered8", "many33", "plane", "in_grid_block")
         if not (key == "plane" and name != "grid3") and not (key == "in_grid_block" and name != "forest")]


def with_clique(n, colp, rows, sc):
    """the pattern plus the set as a clique"""
    cols = np.repeat(np.arange(n), np.diff(colp))
    a, b = np.meshgrid(sc, sc, indexing="ij")
    return csc_from_triplets(n, np.concatenate([rows, a.ravel()]), np.concatenate([cols, b.ravel()]))


def check_schur_structure(s, n, colp, rows, sc):
    ns = len(sc)
    assert s.num_schur == ns and s.schur_indices.tolist() == list(sc)
    assert sorted(s.perm.tolist()) == list(range(n))
    assert s.perm[n - ns:].tolist() == list(sc)  # last, in the order given
    info = s.schur_info()
    J = info["snode"]
    assert J == s.num_snodes - 1 and s.snode_first[J] == n - ns and s.snode_first[J + 1] == n
    assert s.snode_parent[J] == -1  # no rows below it
    kids = s.snode_parent >= 0
    assert (s.snode_parent[kids] > np.nonzero(kids)[0]).all()
    assert (s.snode_level[s.snode_parent[kids]] > s.snode_level[kids]).all()
    level = np.zeros(s.num_snodes, dtype=int)
    for K in range(s.num_snodes):  # children come first: the level is the height
        if s.snode_parent[K] >= 0:
            level[s.snode_parent[K]] = max(level[s.snode_parent[K]], level[K] + 1)
    assert np.array_equal(level, s.snode_level) and s.nlevels == level.max() + 1
    assert info["children"] == int((s.snode_parent == J).sum())
    c2, r2 = with_clique(n, colp, rows, sc)
    nnzL, colcount = symbolic_fill(n, c2, r2, s.perm)
    assert s.nnzL == nnzL
    sizes = np.diff(s.snode_first)
    below = colcount[s.snode_first[:-1]] - sizes
    assert below[J] == 0 and int((sizes * (sizes + 1) // 2 + below * sizes).sum()) == nnzL
    assert ((below == 0) == ~kids).all()
    assert (info["gather_entries"] > 0) == (info["children"] > 0)
    forms = s.kernel_forms(33)
    assert list(forms)[-2:] == ["schur_gather", "schur_fwd"] and len(forms) == 10
    assert forms["schur_gather"] == (1 if info["children"] else 0) and forms["schur_fwd"] == 2 * forms["schur_gather"]


@pytest.mark.parametrize("order", ["nd", "natural", "natural_perm"])
@pytest.mark.parametrize("name,key", CASES)
def test_schur_set_is_the_last_supernode(name, key, order):
    import paropt_amd as pa

    n, colp, rows = pattern(name)
    sc = schur_sets(name, n)[key]
    perm = None
    if order == "natural_perm":
        interior = np.setdiff1d(np.arange(n), sc)
        perm = np.concatenate([np.random.default_rng(4).permutation(interior), sc])
    s = pa.SparseCholesky(None, n, colp, rows, order=order.split("_")[0], perm=perm, schur=sc)
    check_schur_structure(s, n, colp, rows, sc)
    if perm is not None:  # the reported order is a postorder of the caller's elimination tree: the same fill
        assert s.nnzL == symbolic_fill(n, *with_clique(n, colp, rows, sc), perm)[0]
    if order == "nd":
        assert np.array_equal(s.perm, pa.SparseCholesky(None, n, colp, rows, order="amd", schur=sc).perm)
    if name == "forest" and key == "in_grid_block":  # the components that do not touch the set stay separate roots
        assert (s.snode_parent < 0).sum() >= 3
    for cap in (2, 16):
        with pack_cap(cap):
            p = pa.SparseCholesky(None, n, colp, rows, order=order.split("_")[0], perm=perm, schur=sc)
        g = p.packing()
        J = p.schur_info()["snode"]
        assert g["cap"] == cap and np.array_equal(p.perm, s.perm)
        assert not ((g["group_first"] <= J) & (J <= g["group_root"])).any()


@pytest.mark.parametrize("name", ["tridiag", "grid3", "forest", "mass4"])
@pytest.mark.parametrize("order", ["nd", "natural"])
def test_an_empty_set_is_the_plain_analysis(name, order):
    import paropt_amd as pa

    n, colp, rows = pattern(name)
    for cap in (None, 2):
        with pack_cap(cap):
            a = pa.SparseCholesky(None, n, colp, rows, order=order)
            b = pa.SparseCholesky(None, n, colp, rows, order=order, schur=[])
        for f in ("perm", "snode_first", "snode_parent", "snode_level"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        for f in ("size", "num_snodes", "nnzL", "nlevels", "max_snode", "max_front", "work_bytes", "block_width"):
            assert getattr(a, f) == getattr(b, f), f
        assert a.kernel_forms(40) == b.kernel_forms(40) and len(b.kernel_forms()) == 8
        pa_, pb_ = a.packing(), b.packing()
        assert all(np.array_equal(pa_[k], pb_[k]) for k in pa_)
        assert b.num_schur == 0 and b.schur_info() == {"num_schur": 0, "snode": -1, "children": 0, "gather_entries": 0}
        assert a.schur_info() == b.schur_info() and len(a.schur_indices) == 0


@pytest.mark.parametrize("order", ["nd", "natural"])
def test_the_whole_matrix_as_the_set(order):
    import paropt_amd as pa

    n, colp, rows = pattern("grid3")
    sc = [int(v) for v in np.random.default_rng(2).permutation(n)]
    s = pa.SparseCholesky(None, n, colp, rows, order=order, schur=sc)
    assert s.num_snodes == 1 and s.perm.tolist() == sc and s.nnzL == n * (n + 1) // 2
    assert s.schur_info() == {"num_schur": n, "snode": 0, "children": 0, "gather_entries": 0}


def test_refusals():
    import paropt_amd as pa
    import paropt_amd.lib as L

    n, colp, rows = pattern("tridiag")
    for bad, word in (([3, 7, 3], "repeated"), ([3, n], "out of range"), ([-1], "out of range")):
        with pytest.raises(pa.ParOptAMDError) as e:
            pa.SparseCholesky(None, n, colp, rows, schur=bad)
        assert e.value.code == PO_ERR_ARG
        assert word in str(e.value)
    sc = [5, 2, 9]
    interior = np.setdiff1d(np.arange(n), sc)
    for perm in (np.concatenate([interior, [2, 5, 9]]),      # the set last, another order
                 np.concatenate([sc, interior]),             # the set first
                 np.arange(n)):
        with pytest.raises(pa.ParOptAMDError) as e:
            pa.SparseCholesky(None, n, colp, rows, order="natural", perm=perm, schur=sc)
        assert "perm must list the set last" in str(e.value)
    notperm = np.concatenate([interior, sc])
    notperm[0] = notperm[1]
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.SparseCholesky(None, n, colp, rows, order="natural", perm=notperm, schur=sc)
    assert "not a permutation" in str(e.value)
    # the C entry: the same answers as return values; numeric entries on an analysis-only handle
    h = L.po_sparse_chol()
    idx = np.array([3, 3], dtype=np.intc)
    args = (None, n, colp.ctypes.data_as(L.c_int_p), rows.ctypes.data_as(L.c_int_p), 2, None)
    assert L.lib.po_sparse_chol_create_schur(*args, 2, idx.ctypes.data_as(L.c_int_p), C.byref(h)) == PO_ERR_ARG
    assert L.lib.po_sparse_chol_create_schur(*args, n + 1, idx.ctypes.data_as(L.c_int_p), C.byref(h)) == PO_ERR_ARG
    assert L.lib.po_sparse_chol_create_schur(*args, 2, None, C.byref(h)) == PO_ERR_ARG
    s = pa.SparseCholesky(None, n, colp, rows, schur=sc)
    x = np.ones(n)
    px = x.ctypes.data_as(L.c_double_p)
    for call in (lambda: L.lib.po_sparse_chol_get_schur(s.handle, px, 3),
                 lambda: L.lib.po_sparse_chol_solve_condense(s.handle, px, 1, n),
                 lambda: L.lib.po_sparse_chol_solve_expand(s.handle, px, 1, n)):
        assert call() == PO_ERR_ARG and b"analysis-only" in L.lib.po_last_error()
    i4 = (C.c_int64 * 4)()
    assert L.lib.po_sparse_chol_schur_info(None, i4) == PO_ERR_ARG and b"null argument" in L.lib.po_last_error()


@pytest.mark.parametrize("name", ["tridiag", "forest", "mass4"])
def test_the_restatement_agrees_with_the_dense_formula(name):
    """sparse_schur_helpers.partial_nopivot in the handle's own order against numpy.linalg.solve: the d_restate the GPU
    tests multiply by 16 is a few eps, both for an SPD matrix and for a quasi-definite one"""
    import paropt_amd as pa

    n, R, Cc, V = {"tridiag": tridiag_triplets(40), "forest": forest_triplets(), "mass4": mass_triplets(4)}[name]
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    A = dense_from_csc(n, colp, rows, vals)
    sc = schur_sets(name, n)["scattered8"]
    s = pa.SparseCholesky(None, n, colp, rows, schur=sc)
    for M in (A, A - 2.0 * np.diag(np.isin(np.arange(n), sc) * A.diagonal())):  # the second: A22's diagonal negated
        S_ref, scale, _ = schur_dense(M, sc)
        S_host, signs = partial_nopivot(M, s.perm, len(sc))
        assert (signs > 0).all() and np.array_equal(S_host, S_host.T)
        assert d_measure(S_host, S_ref, scale) <= 64.0 * EPS
