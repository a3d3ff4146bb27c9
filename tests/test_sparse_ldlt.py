"""SparseCholesky's LDLT mode without a device: the public entries on analysis-only handles, the launch plan that does
not depend on the mode, and the numpy restatement of the no-pivot L S L^T (sparse_ldlt_helpers.py) that the GPU tests
measure against -- checked here against numpy.linalg on the systems of those tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import csc_from_triplets, dense_from_csc, forest_triplets, tridiag_triplets
from sparse_ldlt_helpers import (EPS, PO_ERR_ARG, bordered_mass_system, bound_for, clique8_quasi_definite,
                                 dense_quasi_definite, eta, grid3_odd, grid3_quasi_definite, inertia_of, ldlt_nopivot,
                                 ldlt_solve, tridiag_quasi_definite, zero_pivot_system)

SYMBOLS = ("po_sparse_chol_set_factorization", "po_sparse_chol_get_factorization", "po_sparse_chol_inertia")
PATTERNS = {"tridiag": lambda: tridiag_triplets(200)[:3], "forest": lambda: forest_triplets()[:3]}


def handle(name, **kw):
    import paropt_amd as pa

    n, R, Cc = PATTERNS[name]()
    colp, rows = csc_from_triplets(n, R, Cc)
    return pa.SparseCholesky(None, n, colp, rows, **kw)


def test_symbols_are_declared_and_bound():
    from paropt_amd.lib import lib

    header = open(os.path.join(ROOT, "include", "paropt_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(po_sparse_chol h" % name, header), name
        assert getattr(lib, name).restype is C.c_int
    assert re.search(r"PO_CHOL_LLT = 0, PO_CHOL_LDLT = 1", header)
    assert "quasi-definite" in header.lower() and "only as good as its pivots" in header


def test_set_and_get_on_an_analysis_only_handle():
    from paropt_amd.lib import lib

    s = handle("tridiag")
    assert s.factorization == "llt"
    s.set_factorization("ldlt")
    assert s.factorization == "ldlt"
    kind = C.c_int(-1)
    assert lib.po_sparse_chol_get_factorization(s.handle, C.byref(kind)) == 0 and kind.value == 1
    s.set_factorization("llt")
    assert s.factorization == "llt"
    assert handle("forest", factorization="ldlt").factorization == "ldlt"
    with pytest.raises(ValueError):
        s.set_factorization("lu")


def test_bad_arguments_are_refused_with_a_message():
    import paropt_amd as pa
    from paropt_amd.lib import lib

    s = handle("tridiag", factorization="ldlt")
    assert lib.po_sparse_chol_set_factorization(s.handle, 7) == PO_ERR_ARG
    assert b"7" in lib.po_last_error()
    assert s.factorization == "ldlt"  # (the refused call changed nothing)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.set_factorization(7)
    assert e.value.code == PO_ERR_ARG
    kind = C.c_int(0)
    out = (C.c_int64 * 3)()
    assert lib.po_sparse_chol_set_factorization(None, 1) == PO_ERR_ARG
    assert lib.po_last_error()
    assert lib.po_sparse_chol_get_factorization(None, C.byref(kind)) == PO_ERR_ARG
    assert lib.po_sparse_chol_inertia(None, out) == PO_ERR_ARG
    # no numeric part, no inertia
    assert lib.po_sparse_chol_inertia(s.handle, out) == PO_ERR_ARG
    assert b"analysis-only" in lib.po_last_error()
    with pytest.raises(pa.ParOptAMDError):
        s.inertia()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_the_launch_plan_and_the_info_do_not_depend_on_the_mode(name):
    from paropt_amd.lib import lib

    llt, ldlt = handle(name), handle(name, factorization="ldlt")
    for nv in (1, 33):
        assert llt.kernel_forms(nv) == ldlt.kernel_forms(nv)
    assert "sign" not in " ".join(ldlt.kernel_forms())
    assert llt.getInfo() == ldlt.getInfo()
    a, b = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    assert lib.po_sparse_chol_info(llt.handle, a) == 0 and lib.po_sparse_chol_info(ldlt.handle, b) == 0
    assert list(a) == list(b)
    assert np.array_equal(llt.perm, ldlt.perm) and np.array_equal(llt.snode_first, ldlt.snode_first)
    assert llt.packing()["factor_levels"] == ldlt.packing()["factor_levels"]
    # switching an existing handle changes nothing either
    before = llt.kernel_forms(3)
    llt.set_factorization("ldlt")
    assert llt.kernel_forms(3) == before


# ---- the restatement -------------------------------------------------------------------------------------------------
def restated(A, b):
    L, s, replaced = ldlt_nopivot(A)
    assert (np.diag(L) > 0).all() and np.array_equal(np.abs(s), np.ones(len(s)))
    return ldlt_solve(L, s, b), inertia_of(s, replaced), (L, s)


def eig_inertia(A):
    w = np.linalg.eigvalsh(A)
    return int((w > 0).sum()), int((w < 0).sum()), 0


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 129])
def test_restatement_on_a_dense_quasi_definite_matrix(n):
    A, n2 = dense_quasi_definite(n, 100 + n)
    b = np.random.default_rng(n).standard_normal(n)
    x, inertia, (L, s) = restated(A, b)
    assert inertia == (n - n2, n2, 0) == eig_inertia(A)
    assert np.abs(L @ np.diag(s) @ L.T - A).max() <= 64 * EPS * np.abs(A).sum(axis=1).max()
    assert eta(A, x, b) <= bound_for(A, b)[0]


def test_restatement_on_the_sparse_systems_of_the_device_tests():
    systems = {}
    n, colp, rows, vals, odd = grid3_quasi_definite((5, 4, 3))
    systems["grid3"] = (dense_from_csc(n, colp, rows, vals), int(odd.sum()))
    assert int(grid3_odd((12, 12, 12)).sum()) == 864 and int(grid3_odd((14, 13, 11)).sum()) == 1001
    n, colp, rows, vals, odd = tridiag_quasi_definite(200)
    systems["tridiag"] = (dense_from_csc(n, colp, rows, vals), 100)
    n, colp, rows, vals, neg = clique8_quasi_definite()
    systems["clique8"] = (dense_from_csc(n, colp, rows, vals), 5)
    K, nm = bordered_mass_system(8)
    assert nm == 162 and K.shape[0] == 162 + 25
    systems["bordered_mass"] = (K, 25)
    for name, (A, nneg) in systems.items():
        n = A.shape[0]
        assert np.array_equal(A, A.T)
        b = np.random.default_rng(5).standard_normal(n)
        for p in (np.arange(n), np.random.default_rng(6).permutation(n)):  # every symmetric permutation has it
            Ap = A[np.ix_(p, p)]
            x, inertia, _ = restated(Ap, b[p])
            assert inertia == (n - nneg, nneg, 0) == eig_inertia(A), name
            assert eta(Ap, x, b[p]) <= bound_for(Ap, b[p])[0], name


def test_restatement_replaces_an_exactly_zero_pivot():
    n, colp, rows, vals, spd = zero_pivot_system()
    A = dense_from_csc(n, colp, rows, vals)
    assert np.array_equal(A[:3, :3], [[4.0, 2.0, 0.0], [2.0, 1.0, 1.0], [0.0, 1.0, 3.0]]) and A[3, 2] == -1.0
    L, s, replaced = ldlt_nopivot(A)
    assert replaced == [1] and inertia_of(s, replaced)[2] == 1
    assert np.isfinite(ldlt_solve(L, s, np.ones(n))).all()
    assert ldlt_nopivot(dense_from_csc(n, colp, rows, spd))[2] == []
