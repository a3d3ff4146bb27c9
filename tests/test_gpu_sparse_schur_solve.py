"""pa.SparseCholesky with a Schur set: factoring S~ = S + add on the device (factor_schur), the dense sweeps with it
(schur_solve), the whole solve() and solve_refined() on such a handle.

One measure, the project's: eta(A, x, b) = max|b - A x| / (||A||_inf max|x| + max|b|) <= max(16 eta_LAPACK, 64 eps)
(sparse_ldlt_helpers.eta, bound_for; tests/test_sparse_schur_solve_contract.py shows the numpy restatement at a
sixteenth of that bound or less on these systems).  Every measured value goes to
profiles/r28_sparse_schur_solve_parity.json.
Systems: those of tests/test_gpu_sparse_schur.py and, with W the panel width of the dense sweeps read from
schur_solve_info(), fanin_kkt(40, 3, ns) (LDLT, S negative definite) with ns in {W - 1, W + 1, 2 W + 1} and
dense_spd(ns + 40) (LLT) with a scattered set of ns = 2 W + 1: the smallest shapes that cross one and two panel edges.
nrhs in (1, 3, 32, 33) (either side of a slab and of the groups of 8 columns), packing caps (0, 2, 16)."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import dense_from_csc
from sparse_chol_packing_helpers import pack_cap
from sparse_ldlt_helpers import EPS, PO_ERR_ARG, bound_for, dense_csc, dense_spd, eta
from sparse_refine_helpers import dense_to_csc, refine_restated, singular_h_system, zero_corner_saddle
from sparse_schur_helpers import fanin_kkt, inertia_dense
from test_gpu_sparse_schur import CAPS, LDLT, LLT, NRHS, handle
from test_gpu_sparse_schur import system as schur_system

pytestmark = pytest.mark.gpu

PARITY = os.path.join(ROOT, "profiles", "r28_sparse_schur_solve_parity.json")
RECORDS = {}
_SYS = {}
PANEL = ["fanin_W-1", "fanin_W+1", "fanin_2W+1", "dense_2W+1"]
ALL = LLT + LDLT + ["fanin300"] + PANEL


def record(name, **values):
    RECORDS[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in values.items()}
    print(name, RECORDS[name])


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    with open(PARITY, "w") as f:
        json.dump({"eps": EPS, "bound": "eta <= max(16 eta_lapack, 64 eps)", "panel_width": panel_width(),
                   "cases": RECORDS}, f, indent=1, sort_keys=True)
        f.write("\n")


def panel_width():
    import paropt_amd as pa

    if "W" not in _SYS:
        colp, rows, _ = dense_csc(np.eye(2))
        _SYS["W"] = pa.SparseCholesky(None, 2, colp, rows, schur=[1]).schur_solve_info()["panel_width"]
    return _SYS["W"]


def system(name):
    """the dict of test_gpu_sparse_schur.system plus G, 33 right-hand sides for S~; made once and left alone"""
    if name in _SYS:
        return _SYS[name]
    if name not in PANEL:
        k = dict(schur_system(name))
    else:
        W = panel_width()
        ns = {"fanin_W-1": W - 1, "fanin_W+1": W + 1, "fanin_2W+1": 2 * W + 1, "dense_2W+1": 2 * W + 1}[name]
        if name.startswith("fanin"):
            K, nE = fanin_kkt(40, 3, ns)
            n = K.shape[0]
            colp, rows, vals = dense_to_csc(K)
            sc, kind = np.arange(nE, n), "ldlt"
        else:
            n = ns + 40
            colp, rows, vals = dense_csc(dense_spd(n, 11))
            sc, kind = np.random.default_rng(3).permutation(n)[:ns], "llt"
        k = dict(n=n, colp=colp, rows=rows, vals=vals, A=dense_from_csc(n, colp, rows, vals),
                 sc=[int(v) for v in sc], kind=kind, B=np.random.default_rng(17).standard_normal((33, n)))
    k["G"] = np.random.default_rng(19).standard_normal((33, len(k["sc"])))
    _SYS[name] = k
    return k


def factored(ctx, k, cap=None, add=None, **kw):
    s = handle(ctx, k, cap=cap, **kw)
    assert s.factor_schur(add) == 0
    return s


def worst_eta(M, X, B, who):
    worst = 0.0
    for j in range(B.shape[0]):
        bound, e_lap = bound_for(M, B[j])
        e = eta(M, X[j], B[j])
        worst = max(worst, e / bound)
        assert e <= bound, (who, j, e, e_lap, bound)
    return worst


def definite_add(k, seed):
    """-+ G G^T / 7 with G of order ns and entries N(0, 1 / ns): S~ stays as definite as S is"""
    ns = len(k["sc"])
    G = np.random.default_rng(seed).standard_normal((ns, ns)) / np.sqrt(ns)
    return (-1.0 if k["kind"] == "ldlt" else 1.0) * (G @ G.T) / 7.0


def with_add(k, add):
    A = k["A"].copy()
    A[np.ix_(k["sc"], k["sc"])] += add
    return A


# ---- 1, 2: the dense solve, the whole solve -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_schur_solve(ctx, name):
    k = system(name)
    s = factored(ctx, k)
    S = s.schur()
    X2 = s.schur_solve(k["G"])
    assert X2.shape == k["G"].shape and np.isfinite(X2).all()
    info = s.schur_solve_info()
    assert info["factored"] and info["factor_bytes"] >= 8 * len(k["sc"]) ** 2
    record("schur_solve|" + name, worst_eta_over_bound=worst_eta(S, X2, k["G"], name), ns=len(k["sc"]),
           launches=info["launches"])
    s.close()


@pytest.mark.parametrize("name", ALL)
def test_whole_solve(ctx, name):
    k = system(name)
    s = factored(ctx, k)
    B, sc = k["B"], k["sc"]
    X = s.solve(B)
    worst = worst_eta(k["A"], X, B, name)
    Z = s.condense(B)
    Z[:, sc] = s.schur_solve(Z[:, sc])
    assert np.array_equal(s.expand(Z), X), name  # bit for bit
    record("solve|" + name, worst_eta_over_bound=worst)
    s.close()


# ---- 3: bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid3_s33", "grid3_qd", "fanin_W+1", "dense_2W+1"])
def test_bits_do_not_depend_on_nrhs_cap_or_entry(ctx, name):
    import torch

    k = system(name)
    B, G = k["B"], k["G"]
    s0 = factored(ctx, k, cap=0)
    X, X2 = s0.solve(B), s0.schur_solve(G)
    for nrhs in NRHS:  # a column's bits do not depend on the columns beside it
        assert np.array_equal(s0.solve(B[:nrhs]), X[:nrhs]), (name, nrhs)
        assert np.array_equal(s0.schur_solve(G[:nrhs]), X2[:nrhs]), (name, nrhs)
    for j in (0, 7, 32):
        assert np.array_equal(s0.solve(B[j]), X[j]) and np.array_equal(s0.schur_solve(G[j]), X2[j]), (name, j)
    for cap in CAPS[1:]:
        s = factored(ctx, k, cap=cap)
        assert s.packing()["cap"] == cap
        assert np.array_equal(s.solve(B), X) and np.array_equal(s.schur_solve(G), X2), (name, cap)
        s.close()
    # host entry against device entry
    dev = torch.device("cuda", ctx.device())
    t = torch.tensor(B, dtype=torch.float64, device=dev)
    assert s0.solve_tensor(t) is t and np.array_equal(t.cpu().numpy(), X)
    t = torch.tensor(G, dtype=torch.float64, device=dev)
    assert s0.schur_solve_tensor(t) is t and np.array_equal(t.cpu().numpy(), X2)
    assert s0.factor_schur_tensor() == 0  # again, through the device entry: the same factor
    assert np.array_equal(s0.solve(B), X)
    s0.close()


# ---- 4: inertia -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_inertia(ctx, name):
    k = system(name)
    s = factored(ctx, k)
    ns = len(k["sc"])
    sp, sn, sr = s.schur_inertia()
    assert sp + sn + sr == ns
    if k["kind"] == "ldlt":
        pos, neg, rep = s.inertia()
        assert pos + neg + rep == k["n"] - ns  # (inertia() keeps speaking of the interior)
        assert (pos + sp, neg + sn, rep + sr) == inertia_dense(k["A"]), name
    else:
        assert (sp, sn, sr) == (ns, 0, 0) and s.inertia() == (k["n"] - ns, 0, 0)
    s.close()


# ---- 5: add -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid3_s33", "grid3_qd", "fanin_W+1", "dense_2W+1"])
def test_add(ctx, name):
    import paropt_amd as pa
    import torch

    k = system(name)
    B = k["B"][:3]
    s = handle(ctx, k, keep_matrix=True)
    S = s.schur()
    for seed in (23, 29):  # the second with no factor() in between
        add = definite_add(k, seed)
        assert s.factor_schur(add) == 0
        assert np.array_equal(s.schur(), S)  # bit for bit
        X = s.solve(B)
        record("add|%s|%d" % (name, seed), worst_eta_over_bound=worst_eta(with_add(k, add), X, B, name))
        X2 = s.schur_solve(k["G"][:3])
        worst_eta(S + add, X2, k["G"][:3], name)
        with pytest.raises(pa.ParOptAMDError) as e:
            s.solve_refined(B)
        assert e.value.code == PO_ERR_ARG and "add" in str(e.value) and "retained" in str(e.value)
        t = torch.tensor(add, dtype=torch.float64, device=torch.device("cuda", ctx.device()))
        assert s.factor_schur_tensor(t) == 0
        assert np.array_equal(s.solve(B), X)  # the device entry reads the same triangle
    # only the lower triangle of add is read
    assert s.factor_schur(np.tril(add)) == 0 and np.array_equal(s.solve(B), X)
    # without one again: the plain system, and the refined solve is allowed
    assert s.factor_schur() == 0 and np.array_equal(s.schur(), S)
    worst_eta(k["A"], s.solve(B), B, name)
    xr, info = s.solve_refined(B)
    worst_eta(k["A"], xr, B, name)
    s.close()


# ---- 6: the refined solve ---------------------------------------------------------------------------------------------
def needy_systems():
    for nx in (3, 4):
        for order in ("natural", "nd"):
            yield "saddle%d|%s" % (nx, order), zero_corner_saddle(nx), order
    for delta in (1e-6, 1e-8):
        for order in ("natural", "nd"):
            yield "singularH|%g|%s" % (delta, order), singular_h_system(delta), order


@pytest.mark.parametrize("case", list(needy_systems()), ids=lambda c: c[0])
def test_refined_solve_on_the_zero_corner(ctx, case):
    """the systems and the acceptance rule of tests/test_gpu_sparse_refine.py, the zero block as the Schur set"""
    import paropt_amd as pa

    name, (A, shift, nm), order = case
    n = A.shape[0]
    colp, rows, vals = dense_to_csc(A)
    s = pa.SparseCholesky(ctx, n, colp, rows, order=order, factorization="ldlt", keep_matrix=True,
                          schur=list(range(nm, n)))
    s.set_diagonal_shift(shift)
    s.set_values(vals)
    assert s.factor() == 0 and s.factor_schur() == 0
    assert s.inertia() == (nm, 0, 0) and s.schur_inertia() == (0, n - nm, 0)
    b = np.random.default_rng(44).standard_normal(n)
    bound, e_lap = bound_for(A, b)
    x, info = s.solve_refined(b)
    e0, e1, steps = float(info["eta0"][0]), float(info["eta"][0]), int(info["steps"][0])
    e_plain, e_np = eta(A, s.solve(b), b), eta(A, x, b)
    perm = s.perm
    _, k_ref, etas_ref = refine_restated(A[np.ix_(perm, perm)], shift[perm], b[perm])
    p = int(np.diff(s.matrix_arrays()[0]).max())
    record("refined|" + name, eta0_device=e0, eta_device=e1, eta_numpy_of_x=e_np, eta_plain_solve=e_plain,
           eta_lapack=e_lap, bound=bound, steps=steps, steps_restatement=k_ref, etas_restatement=etas_ref)
    assert e0 > bound and e_plain > bound, (name, e0, e_plain, bound)  # the case discriminates
    assert np.isfinite(x).all()
    assert e_np <= bound, (name, e_np, bound)
    assert e_np / (p + 2) <= e1 <= e_np * (p + 2), (name, e1, e_np)
    assert steps <= k_ref + 1, (name, steps, k_ref)
    s.close()


# ---- 7: pivots --------------------------------------------------------------------------------------------------------
def test_llt_reports_the_first_non_positive_pivot(ctx):
    import paropt_amd as pa

    k = system("dense_2W+1")
    n, ns = k["n"], len(k["sc"])
    s = handle(ctx, k)
    S = s.schur()
    for kk in (0, 40, ns - 1):  # the first block, a later block of the first panel, the last pivot
        add = np.zeros((ns, ns))
        add[kk, kk] = -100.0 * S.diagonal().max()  # pivot kk <= S_kk + add_kk < 0; no earlier pivot sees the entry
        assert s.factor_schur(add) == 1 + n - ns + kk
        with pytest.raises(pa.ParOptAMDError) as e:
            s.schur_inertia()
        assert e.value.code == PO_ERR_ARG and "replaced" in str(e.value)
    assert s.factor_schur() == 0 and s.schur_inertia() == (ns, 0, 0)
    s.close()


def test_ldlt_replaces_a_zero_first_pivot(ctx):
    import paropt_amd as pa

    n = 40
    rng = np.random.default_rng(31)
    A = rng.standard_normal((n, n))
    A = A + A.T + np.diag(np.where(np.arange(n) % 2 == 0, 6.0, -6.0))
    A[0, 0] = 0.0
    colp, rows, vals = dense_csc(A)
    s = pa.SparseCholesky(ctx, n, colp, rows, factorization="ldlt", schur=list(range(n)))
    s.set_values(vals)
    assert s.factor() == 0 and s.inertia() == (0, 0, 0)
    assert s.factor_schur() == 1
    sp, sn, sr = s.schur_inertia()
    assert sr == 1 and sp + sn + sr == n
    s.close()


# ---- 8: the whole matrix as the set -----------------------------------------------------------------------------------
def test_the_handle_as_a_dense_solver(ctx):
    import paropt_amd as pa

    n = 130
    A = dense_spd(n, 11)
    colp, rows, vals = dense_csc(A)
    sc = [int(v) for v in np.random.default_rng(6).permutation(n)]
    s = pa.SparseCholesky(ctx, n, colp, rows, schur=sc)
    s.set_values(vals)
    assert s.factor() == 0 and s.factor_schur() == 0
    assert s.inertia() == (0, 0, 0) and s.schur_inertia() == (n, 0, 0)
    B = np.random.default_rng(17).standard_normal((33, n))
    X = s.solve(B)
    record("dense130_all", worst_eta_over_bound=worst_eta(A, X, B, "dense130_all"))
    assert np.array_equal(s.schur_solve(B[:, sc]), X[:, sc])  # the same sweeps, in the order of the set
    s.close()


# ---- 9: contract ------------------------------------------------------------------------------------------------------
def test_contract(ctx):
    import ctypes as C
    import gc

    import paropt_amd as pa
    import paropt_amd.lib as L

    gc.collect()
    ctx.synchronize()
    before = pa.live_objects()
    k = system("grid3_qd")
    n, ns = k["n"], len(k["sc"])
    s = handle(ctx, k, factor=False)
    for call in (s.factor_schur, lambda: s.schur_solve(np.ones(ns))):  # before factor()
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG and "factor()" in str(e.value)
    assert s.factor() == 0
    with pytest.raises(pa.ParOptAMDError) as e:  # the old refusal, and the new way out
        s.solve(np.ones(n))
    assert "solve_condense()" in str(e.value) and "solve_expand()" in str(e.value) and "schur_factor()" in str(e.value)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.schur_solve(np.ones(ns))
    assert e.value.code == PO_ERR_ARG and "schur_factor()" in str(e.value)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.schur_inertia()
    assert "before schur_factor()" in str(e.value)
    work = s.work_bytes, s.kernel_forms(33)
    live = pa.live_objects()
    add = np.zeros((ns, ns))
    info = C.c_int()
    assert L.lib.po_sparse_chol_schur_factor(s.handle, add.ctypes.data_as(L.c_double_p), ns - 1,
                                             C.byref(info)) == PO_ERR_ARG
    assert b"ldadd" in L.lib.po_last_error()
    assert pa.live_objects() == live  # nothing is allocated before the first factorization of S
    assert s.factor_schur() == 0
    assert pa.live_objects()[1] >= live[1] + 8 * ns * ns and s.schur_solve_info()["factor_bytes"] >= 8 * ns * ns
    assert (s.work_bytes, s.kernel_forms(33)) == work
    x = np.ones((2, ns))
    px = x.ctypes.data_as(L.c_double_p)
    assert L.lib.po_sparse_chol_schur_solve(s.handle, px, -1, ns) == PO_ERR_ARG
    assert L.lib.po_sparse_chol_schur_solve(s.handle, px, 2, ns - 1) == PO_ERR_ARG and b"ldx2" in L.lib.po_last_error()
    assert L.lib.po_sparse_chol_schur_solve(s.handle, px, 0, ns) == 0
    assert L.lib.po_sparse_chol_schur_solve(s.handle, None, 1, ns) == PO_ERR_ARG
    s.solve(np.ones((40, n)))
    s.set_values(k["vals"])  # ends all of it
    for call in (lambda: s.solve(np.ones(n)), lambda: s.schur_solve(np.ones(ns)), s.factor_schur):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG
    assert not s.schur_solve_info()["factored"]
    assert s.factor() == 0
    with pytest.raises(pa.ParOptAMDError) as e:  # factor() alone does not factor S
        s.solve(np.ones(n))
    assert "solve_condense()" in str(e.value)
    assert s.factor_schur() == 0
    worst_eta(k["A"], s.solve(k["B"][:2]), k["B"][:2], "contract")
    # a handle without a set
    p = pa.SparseCholesky(ctx, n, k["colp"], k["rows"], factorization="ldlt")
    p.set_values(k["vals"])
    assert p.factor() == 0
    for call in (p.factor_schur, lambda: p.schur_solve(np.ones(0)), p.schur_inertia):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert e.value.code == PO_ERR_ARG
    p.close()
    s.close()
    ctx.synchronize()
    assert pa.live_objects() == before
