"""pa.SparseCholesky on the device with a retained matrix: the symmetric product, the diagonal shift and the refined
solve (factor A + diag(shift), refine against A).

Product: componentwise |y - A x| <= (p + 1) eps (|A| |x|), p the longest row -- the bound of a length-p dot product in
any order -- against the dense numpy product, and bit-for-bit equalities wherever the result must not depend on
something (the other columns of the panel, factor(), the factorization kind, the shift).

Refinement: the quantity and the bound are those of tests/test_gpu_sparse_ldlt.py, eta(x) = ||b - A x||_inf /
(||A||_inf ||x||_inf + ||b||_inf) <= max(16 eta_LAPACK, 64 eps).  The systems that need it (a zero corner with a shift,
a singular leading block, diagonal entries of 1e-10) start seven orders of magnitude above that bound after the plain
solve -- asserted, so that the cases discriminate -- and end below it.  The numpy restatement of the loop
(sparse_refine_helpers.refine_restated, in the device's elimination order) gives the step count to compare with.
Every measured eta, step count and inertia goes to profiles/r26_sparse_refine_parity.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import csc_from_triplets, dense_from_csc, forest_triplets, mass_triplets
from sparse_ldlt_helpers import (EPS, PO_ERR_ARG, bound_for, dense_csc, dense_quasi_definite, eta, grid3_quasi_definite,
                                 tridiag_quasi_definite)
from sparse_refine_helpers import (dense_to_csc, refine_restated, singular_h_system, tiny_tridiagonal,
                                   zero_corner_saddle)

pytestmark = pytest.mark.gpu

PARITY = {}
NRHS = (1, 3, 32, 33)


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    path = os.path.join(ROOT, "profiles", "r26_sparse_refine_parity.json")
    with open(path, "w") as f:
        json.dump({"eps": EPS, "bound": "eta <= max(16 eta_lapack, 64 eps)", "cases": PARITY}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


def keeper(ctx, n, colp, rows, vals, order="nd", factorization="ldlt", shift=None):
    import paropt_amd as pa

    s = pa.SparseCholesky(ctx, n, colp, rows, order=order, factorization=factorization, keep_matrix=True)
    if shift is not None:
        s.set_diagonal_shift(shift)
    s.set_values(vals)
    return s


def longest_row(s):
    return int(np.diff(s.matrix_arrays()[0]).max())


# ---- product -----------------------------------------------------------------------------------------------------------
def product_systems():
    n, colp, rows, vals, _ = tridiag_quasi_definite(40)
    yield "tridiag40|natural", n, colp, rows, vals, "natural", "ldlt"
    yield "tridiag40|nd", n, colp, rows, vals, "nd", "ldlt"
    n, colp, rows, vals, _ = grid3_quasi_definite((5, 4, 3))
    yield "grid3_5x4x3", n, colp, rows, vals, "nd", "ldlt"
    n, R, Cc, V = mass_triplets(3)
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    yield "mass3|llt", n, colp, rows, vals, "nd", "llt"
    A, _ = dense_quasi_definite(70, 5)
    colp, rows, vals = dense_csc(A)
    yield "dense70", 70, colp, rows, vals, "nd", "ldlt"
    n, R, Cc, V = forest_triplets()
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    yield "forest", n, colp, rows, vals, "nd", "llt"


@pytest.mark.parametrize("case", list(product_systems()), ids=lambda c: c[0])
def test_product_against_numpy_and_column_by_column(ctx, case):
    from paropt_amd.lib import lib

    name, n, colp, rows, vals, order, kind = case
    s = keeper(ctx, n, colp, rows, vals, order=order, factorization=kind)
    A = dense_from_csc(n, colp, rows, vals)
    p = longest_row(s)
    assert p == int((A != 0).sum(axis=1).max())
    if name == "dense70":
        assert s.max_front > 64 and p > 64  # one front wider than a tile, rows longer than a wavefront
    X = np.random.default_rng(41).standard_normal((33, n))
    singles = [s.matvec(X[j]) for j in range(33)]
    worst = 0.0
    for nrhs in NRHS:
        Y = s.matvec(X[:nrhs])
        assert Y.shape == (nrhs, n)
        for j in range(nrhs):
            assert np.array_equal(Y[j], singles[j]), (name, nrhs, j)
    for j in range(33):
        err, scale = np.abs(singles[j] - A @ X[j]), np.abs(A) @ np.abs(X[j])
        worst = max(worst, float((err / scale).max()))
        assert (err <= (p + 1) * EPS * scale).all(), (name, j, float((err / scale).max()))
    PARITY["product|" + name] = {"longest_row": p, "worst_error_over_|A||x|": worst, "bound": (p + 1) * EPS}
    print("product", name, PARITY["product|" + name])
    # ldx > n, through the C entry: what lies between the columns of y is left alone
    ld = n + 3
    xin = np.zeros((3, ld))
    xin[:, :n] = X[:3]
    yout = np.full((3, ld), 7.0)
    dp = C.POINTER(C.c_double)
    assert lib.po_sparse_chol_matvec(s.handle, xin.ctypes.data_as(dp), ld, yout.ctypes.data_as(dp), ld, 3) == 0
    assert np.array_equal(yout[:, :n], np.array(singles[:3])) and (yout[:, n:] == 7.0).all()
    # unchanged by factor(), by the factorization kind and by a shift with new values
    ref = np.array(singles[:3])
    s.factor()
    assert np.array_equal(s.matvec(X[:3]), ref)
    s.set_factorization("llt" if kind == "ldlt" else "ldlt")
    assert np.array_equal(s.matvec(X[:3]), ref)
    s.set_factorization(kind)
    s.set_diagonal_shift(np.linspace(0.5, 1.5, n))
    s.set_values(vals)
    assert np.array_equal(s.matvec(X[:3]), ref)
    s.factor()
    assert np.array_equal(s.matvec(X[:3]), ref)
    s.close()


def test_product_on_device_tensors(ctx):
    import torch

    n, colp, rows, vals, _ = grid3_quasi_definite((5, 4, 3))
    s = keeper(ctx, n, colp, rows, vals)
    X = np.random.default_rng(42).standard_normal((33, n))
    dev = torch.device("cuda", ctx.device())
    x, y = torch.from_numpy(X).to(dev), torch.zeros((33, n), dtype=torch.float64, device=dev)
    assert s.matvec_tensor(x, y) is y
    assert np.array_equal(y.cpu().numpy(), s.matvec(X))
    assert np.array_equal(x.cpu().numpy(), X)
    s.close()


# ---- the shift ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["llt", "ldlt"])
def test_shift_is_factored_but_not_retained(ctx, kind):
    """without keeping, the handle simply solves the shifted system; with it, the product still sees A"""
    import paropt_amd as pa

    n, R, Cc, V = mass_triplets(3)
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    A = dense_from_csc(n, colp, rows, vals)
    shift = np.linspace(0.25, 0.75, n)
    b = np.random.default_rng(43).standard_normal(n)
    s = pa.SparseCholesky(ctx, n, colp, rows, factorization=kind)
    s.set_diagonal_shift(shift)
    s.set_values(vals)
    assert s.factor() == 0 and s.inertia() == (n, 0, 0)
    As = A + np.diag(shift)
    x = s.solve(b)
    assert eta(As, x, b) <= bound_for(As, b)[0]
    assert eta(A, x, b) > 1e-3  # (it is not the solution of the unshifted system)
    # cleared, the next values give the unshifted system back
    s.set_diagonal_shift(None)
    s.set_values(vals)
    assert s.factor() == 0
    assert eta(A, s.solve(b), b) <= bound_for(A, b)[0]
    s.close()


# ---- refinement where it is needed -------------------------------------------------------------------------------------
def needy_systems():
    for nx in (3, 4):
        for order in ("natural", "nd"):
            yield "saddle%d|%s" % (nx, order), zero_corner_saddle(nx), order, "saddle"
    for delta in (1e-6, 1e-8):
        for order in ("natural", "nd"):
            yield "singularH|%g|%s" % (delta, order), singular_h_system(delta), order, "singular"
    yield "tridiag1e-10|natural", tiny_tridiagonal(), "natural", "tiny"


@pytest.mark.parametrize("case", list(needy_systems()), ids=lambda c: c[0])
def test_refinement_where_it_is_needed(ctx, case):
    name, (A, shift, nm), order, family = case
    n = A.shape[0]
    colp, rows, vals = dense_to_csc(A)
    s = keeper(ctx, n, colp, rows, vals, order=order, shift=shift if shift.any() else None)
    assert s.factor() == 0
    inertia = s.inertia()
    b = np.random.default_rng(44).standard_normal(n)
    bound, e_lap = bound_for(A, b)
    x, info = s.solve_refined(b)
    e0, e1, steps = float(info["eta0"][0]), float(info["eta"][0]), int(info["steps"][0])
    e_plain, e_np = eta(A, s.solve(b), b), eta(A, x, b)
    perm = s.perm
    _, k_ref, etas_ref = refine_restated(A[np.ix_(perm, perm)], shift[perm], b[perm])
    p = longest_row(s)
    PARITY[name] = {"eta0_device": e0, "eta_device": e1, "eta_numpy_of_x": e_np, "eta_plain_solve": e_plain,
                    "eta_lapack": e_lap, "bound": bound, "steps": steps, "steps_restatement": k_ref,
                    "etas_restatement": etas_ref, "inertia": list(inertia), "longest_row": p}
    print(name, PARITY[name])
    assert e0 > bound and e_plain > bound, (name, e0, e_plain, bound)  # the case discriminates
    assert np.isfinite(x).all()
    assert e_np <= bound, (name, e_np, bound)
    assert e_np / (p + 2) <= e1 <= e_np * (p + 2), (name, e1, e_np)
    assert steps <= k_ref + 1, (name, steps, k_ref)
    if family == "saddle":
        assert inertia == (nm, n - nm, 0)
    elif family == "singular":
        assert inertia == (40, 4, 0)
    s.close()


# ---- refinement where it is not needed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["dense70", "grid3_5x4x3"])
def test_refinement_where_it_is_not_needed(ctx, system):
    if system == "dense70":
        A, _ = dense_quasi_definite(70, 5)
        n = 70
        colp, rows, vals = dense_csc(A)
    else:
        n, colp, rows, vals, _ = grid3_quasi_definite((5, 4, 3))
        A = dense_from_csc(n, colp, rows, vals)
    s = keeper(ctx, n, colp, rows, vals)
    assert s.factor() == 0
    B = np.random.default_rng(45).standard_normal((3, n))
    plain = s.solve(B)
    X0, info0 = s.solve_refined(B, max_steps=0)
    assert np.array_equal(X0, plain) and (info0["steps"] == 0).all()
    assert np.array_equal(info0["eta0"], info0["eta"])
    X, info = s.solve_refined(B)
    for j in range(3):
        bound, e_lap = bound_for(A, B[j])
        e_np = eta(A, X[j], B[j])
        PARITY["%s|rhs%d" % (system, j)] = {"eta0_device": float(info["eta0"][j]), "eta_device": float(info["eta"][j]),
                                            "eta_numpy_of_x": e_np, "eta_lapack": e_lap, "bound": bound,
                                            "steps": int(info["steps"][j])}
        print(system, j, PARITY["%s|rhs%d" % (system, j)])
        if info["steps"][j] == 0:
            assert np.array_equal(X[j], plain[j])
        assert e_np <= bound and info["eta0"][j] == info0["eta0"][j]
    s.close()


# ---- column independence, stopping -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saddle3(ctx):
    A, shift, nm = zero_corner_saddle(3)
    n = A.shape[0]
    colp, rows, vals = dense_to_csc(A)
    s = keeper(ctx, n, colp, rows, vals, shift=shift)
    assert s.factor() == 0
    B = np.random.default_rng(46).standard_normal((33, n))
    B[0] *= 1e8
    B[17] *= 1e-8
    yield s, A, B
    s.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_every_column_equals_the_column_alone(saddle3):
    s, A, B = saddle3
    X, info = s.solve_refined(B)
    assert info["steps"].max() >= 1
    for j in range(33):
        xj, ij = s.solve_refined(B[j])
        assert same_bits(X[j], xj), j
        assert info["steps"][j] == ij["steps"][0]
        assert same_bits(info["eta0"][j:j + 1], ij["eta0"]) and same_bits(info["eta"][j:j + 1], ij["eta"]), j


def test_stopping_rules(saddle3):
    import torch

    s, A, B = saddle3
    n = A.shape[0]
    plain = s.solve(B[:3])
    X, info = s.solve_refined(B[:3], tol=1.0)
    assert (info["steps"] == 0).all() and np.array_equal(X, plain)
    X1, info1 = s.solve_refined(B[:3], max_steps=1)
    full, info_full = s.solve_refined(B[:3])
    assert (info1["steps"] == 1).all() and (info_full["steps"] >= 1).all()
    assert (info1["eta"] < info1["eta0"]).all() and np.array_equal(info1["eta0"], info_full["eta0"])
    # one NaN in one right-hand side: that column stops at once with a NaN eta, the others do not notice
    Bn = B[:5].copy()
    Bn[2, 7] = np.nan
    Xn, infon = s.solve_refined(Bn)
    assert infon["steps"][2] == 0 and np.isnan(infon["eta"][2]) and np.isnan(infon["eta0"][2])
    ref, info_ref = s.solve_refined(B[:5])
    for j in (0, 1, 3, 4):
        assert same_bits(Xn[j], ref[j]) and infon["steps"][j] == info_ref["steps"][j]
        assert same_bits(infon["eta"][j:j + 1], info_ref["eta"][j:j + 1])
    # the device entry gives the bits of the host entry
    t = torch.from_numpy(B[:3]).to(torch.device("cuda", s.ctx.device()))
    tt, info_t = s.solve_refined_tensor(t)
    assert tt is t and np.array_equal(t.cpu().numpy(), full) and np.array_equal(info_t["steps"], info_full["steps"])
    PARITY["saddle3|stopping"] = {"steps_default": info_full["steps"].tolist(), "eta_after_one": info1["eta"].tolist(),
                                  "eta_default": info_full["eta"].tolist()}


# ---- errors, memory ----------------------------------------------------------------------------------------------------
def test_errors_come_with_a_message(ctx):
    import paropt_amd as pa
    from paropt_amd.lib import lib

    n, colp, rows, vals, _ = tridiag_quasi_definite(40)
    b = np.ones(n)
    s = pa.SparseCholesky(ctx, n, colp, rows, factorization="ldlt")
    s.set_values(vals)
    assert s.factor() == 0
    for call in (lambda: s.matvec(b), lambda: s.solve_refined(b)):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG and "keep_matrix" in str(e.value)
        assert b"keep_matrix" in lib.po_last_error()
    s.set_keep_matrix(True)
    with pytest.raises(pa.ParOptAMDError) as e:  # (the values went into the factor before keeping was on)
        s.matvec(b)
    assert "values" in str(e.value)
    s.set_values(vals)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.solve_refined(b)
    assert e.value.code == PO_ERR_ARG and "before factor()" in str(e.value)
    # another pattern while keeping: the lower triangle only
    cols = np.repeat(np.arange(n), np.diff(colp))
    low = rows >= cols
    colp2 = np.concatenate([[0], np.cumsum(np.bincount(cols[low], minlength=n))]).astype(np.intc)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.set_values(colp2, rows[low], vals[low])
    assert e.value.code == PO_ERR_ARG and "creation pattern" in str(e.value)
    s.set_keep_matrix(False)
    s.set_values(colp2, rows[low], vals[low])  # (allowed again)
    with pytest.raises(ValueError):
        s.set_diagonal_shift(np.zeros(n - 1))
    with pytest.raises(pa.ParOptAMDError):
        s.solve_refined(np.ones((2, n)), max_steps=0)  # keeping is off
    s.close()


def test_everything_is_freed_with_the_handle(ctx):
    import paropt_amd as pa

    ctx.synchronize()
    before = pa.live_objects()
    A, shift, nm = zero_corner_saddle(3)
    n = A.shape[0]
    colp, rows, vals = dense_to_csc(A)
    s = keeper(ctx, n, colp, rows, vals, shift=shift)
    assert s.factor() == 0
    s.matvec(np.ones((40, n)))
    s.solve_refined(np.ones((40, n)))
    assert pa.live_objects()[1] > before[1]
    s.close()
    assert pa.live_objects() == before
