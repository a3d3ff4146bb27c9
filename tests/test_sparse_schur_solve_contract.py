"""The factored Schur complement of pa.SparseCholesky without a device: the header declares the six entries, the numeric
ones refuse an analysis-only handle with a message, po_sparse_chol_schur_solve_info reports the panel width W and the
launch count of the panel loop, and the numpy restatement of the solves the GPU tests bound (ldlt_nopivot and
triangular solves, sparse_ldlt_helpers) is no worse than LAPACK on them, so the factor 16 in the bound is all margin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import csc_from_triplets, tridiag_triplets
from sparse_ldlt_helpers import PO_ERR_ARG, bound_for, dense_spd, eta, ldlt_nopivot, ldlt_solve
from sparse_schur_helpers import fanin_kkt

ENTRIES = ("po_sparse_chol_schur_factor", "po_sparse_chol_schur_factor_device", "po_sparse_chol_schur_solve",
           "po_sparse_chol_schur_solve_device", "po_sparse_chol_schur_inertia", "po_sparse_chol_schur_solve_info")


def test_the_header_declares_the_entries():
    import paropt_amd.lib as L

    text = open(os.path.join(ROOT, "include", "paropt_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(po_sparse_chol h, " % name, code), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert "FACTORED SCHUR COMPLEMENT" in text


def dense_pattern(n):
    colp = (np.arange(n + 1) * n).astype(np.intc)
    rows = np.tile(np.arange(n, dtype=np.intc), n)
    return colp, rows


def test_numeric_entries_refuse_an_analysis_only_handle():
    import paropt_amd as pa
    import paropt_amd.lib as L

    n, R, Cc, _ = tridiag_triplets(40)
    colp, rows = csc_from_triplets(n, R, Cc)
    s = pa.SparseCholesky(None, n, colp, rows, schur=[5, 2, 9])
    x = np.ones(9)
    px = x.ctypes.data_as(L.c_double_p)
    info = C.c_int()
    i3 = (C.c_int64 * 3)()
    for call in (lambda: L.lib.po_sparse_chol_schur_factor(s.handle, None, 3, C.byref(info)),
                 lambda: L.lib.po_sparse_chol_schur_factor(s.handle, px, 3, C.byref(info)),
                 lambda: L.lib.po_sparse_chol_schur_factor_device(s.handle, None, 3, C.byref(info)),
                 lambda: L.lib.po_sparse_chol_schur_solve(s.handle, px, 1, 3),
                 lambda: L.lib.po_sparse_chol_schur_solve_device(s.handle, None, 1, 3),
                 lambda: L.lib.po_sparse_chol_schur_inertia(s.handle, i3)):
        assert call() == PO_ERR_ARG and b"analysis-only" in L.lib.po_last_error()
    for call in (s.factor_schur, lambda: s.schur_solve(np.ones(3)), s.schur_inertia):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG and "analysis-only" in str(e.value)
    i4 = (C.c_int64 * 4)()
    assert L.lib.po_sparse_chol_schur_solve_info(None, i4) == PO_ERR_ARG and b"null argument" in L.lib.po_last_error()
    assert L.lib.po_sparse_chol_schur_solve_info(s.handle, None) == PO_ERR_ARG


def launches_of_the_panel_loop(ns, W):
    """forward: every panel its diagonal block, every panel but the last the rows below it; backward the same"""
    panels = -(-ns // W)
    return 2 * (2 * panels - 1) if ns > 0 else 0


def test_solve_info_reports_the_panel_loop():
    import paropt_amd as pa

    n0, R, Cc, _ = tridiag_triplets(40)
    colp0, rows0 = csc_from_triplets(n0, R, Cc)
    plain = pa.SparseCholesky(None, n0, colp0, rows0)
    info = plain.schur_solve_info()
    W = info["panel_width"]
    assert W in (64, 128, 256) and W % plain.block_width == 0
    assert info == {"panel_width": W, "launches": 0, "factor_bytes": 0, "factored": False}
    for ns in (1, W, W + 1, 2 * W + 1):
        n = ns + 7
        colp, rows = dense_pattern(n)
        s = pa.SparseCholesky(None, n, colp, rows, schur=list(range(3, 3 + ns)))
        info = s.schur_solve_info()
        assert info["panel_width"] == W and not info["factored"] and info["factor_bytes"] == 0
        assert info["launches"] == launches_of_the_panel_loop(ns, W), (ns, info)
        # nothing else about the handle moves: the ten kernel forms, the last two the Schur gathers
        forms = s.kernel_forms(33)
        assert len(forms) == 10 and list(forms)[-2:] == ["schur_gather", "schur_fwd"]
    assert [launches_of_the_panel_loop(ns, W) for ns in (1, W, W + 1, 2 * W + 1)] == [2, 2, 6, 10]


def restated_eta_over_bound(A, B):
    L_, s_, replaced = ldlt_nopivot(A)
    assert not replaced
    worst = 0.0
    for b in B:
        x = ldlt_solve(L_, s_, b)
        worst = max(worst, eta(A, x, b) / bound_for(A, b)[0])
    return worst


@pytest.mark.parametrize("case", ["fanin255", "fanin257", "fanin513", "fanin255|add", "fanin257|add", "fanin513|add",
                                  "dense300"])
def test_the_restatement_sits_far_below_the_bound(case):
    """The systems of tests/test_gpu_sparse_schur_solve.py at the panel widths 128 and 256, the set ordered last.  The
    bound is max(16 eta_LAPACK, 64 eps); the no-pivot factorization and triangular solves in numpy stay under a
    sixteenth of it, max(eta_LAPACK, 4 eps) -- no pivoting costs these definite-block systems nothing against LAPACK,
    so the whole factor 16 is margin for the device's summation orders.  (Measured here: 0.006 to 0.012 of the bound.)"""
    if case == "dense300":
        A = dense_spd(300, 11)
        sc = np.random.default_rng(3).permutation(300)[:260]
        perm = np.concatenate([np.setdiff1d(np.arange(300), sc), sc])
        A = A[np.ix_(perm, perm)]
    else:
        ns = int(case[5:8])
        nblocks = 60 if ns == 513 else 40
        A, nE = fanin_kkt(nblocks, 3, ns)
        if case.endswith("|add"):
            G = np.random.default_rng(23).standard_normal((ns, 5)) / np.sqrt(ns)
            A[nE:, nE:] -= G @ G.T / 7.0
    B = np.random.default_rng(17).standard_normal((3, A.shape[0]))
    worst = restated_eta_over_bound(A, B)
    print(case, "restated eta / bound", worst)
    assert worst <= 1.0 / 16.0
