"""pa.SparseCholesky in LDLT mode on the device: P A P^T = L S L^T of symmetric quasi-definite matrices, no pivoting.

The quantity compared and the bound are those of tests/test_gpu_sparse_chol.py: the normwise backward error
eta(x) = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) and eta_device <= max(16 eta_LAPACK, 64 eps), LAPACK being
numpy.linalg.solve on the dense matrix (LU with partial pivoting: the matrices are indefinite).  The numpy restatement
of the no-pivot factorization (sparse_ldlt_helpers.ldlt_nopivot) alone reaches 7e-17 to 9e-16 on these systems against
a bound of 1.4e-14, so the bound is of the method's order; its eta is recorded beside the device's where the system is
small enough to restate, and its signs give the expected inertia.  Where a result must not depend on something (the
mode on a matrix whose signs are all +, the packing cap, the number of right-hand sides) the comparison is bit for bit:
multiplying by +-1.0 is exact.  Every measured eta and inertia goes to profiles/r22_sparse_ldlt_parity.json."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import dense_from_csc, symbolic_fill
from sparse_chol_packing_helpers import pack_cap
from sparse_ldlt_helpers import (EPS, bordered_mass_system, bound_for, clique8_quasi_definite, dense_csc,
                                 dense_quasi_definite, dense_spd, eta, grid3_quasi_definite, grid3_system, inertia_of,
                                 ldlt_nopivot, ldlt_solve, tridiag_quasi_definite, zero_pivot_system)

pytestmark = pytest.mark.gpu

PARITY = {}
_GRID = {}
CAPS = (0, 2, 16)
NRHS = (1, 3, 32, 33)


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    path = os.path.join(ROOT, "profiles", "r22_sparse_ldlt_parity.json")
    with open(path, "w") as f:
        json.dump({"eps": EPS, "bound": "eta <= max(16 eta_lapack, 64 eps)", "cases": PARITY}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


def check_solution(name, A, x, b, inertia, restate=False):
    bound, e_lap = bound_for(A, b)
    e_dev = eta(A, x, b)
    PARITY[name] = {"eta_device": e_dev, "eta_lapack": e_lap, "bound": bound, "inertia": list(inertia)}
    if restate:
        L, s, replaced = ldlt_nopivot(A)
        PARITY[name]["eta_restatement"] = eta(A, ldlt_solve(L, s, b), b)
        assert tuple(inertia) == inertia_of(s, replaced), (name, inertia)  # (Sylvester: whatever the order)
    print(name, PARITY[name])
    assert np.isfinite(x).all()
    assert e_dev <= bound, (name, e_dev, e_lap)


def ldlt_solver(ctx, n, colp, rows, vals, order="nd", cap=None):
    import paropt_amd as pa

    with pack_cap(cap):
        s = pa.SparseCholesky(ctx, n, colp, rows, order=order, factorization="ldlt")
    assert s.factorization == "ldlt"
    s.set_values(vals)
    assert s.factor() == 0
    return s


def block_width():
    import paropt_amd as pa

    return pa.SparseCholesky(None, 1, [0, 1], [0]).block_width


def grid_case(ctx, dims):
    """the quasi-definite grid, its factored handle and 33 right-hand sides; made once and left alone"""
    if dims not in _GRID:
        n, colp, rows, vals, odd = grid3_quasi_definite(dims)
        _GRID[dims] = dict(n=n, colp=colp, rows=rows, vals=vals, odd=odd, s=ldlt_solver(ctx, n, colp, rows, vals),
                           A=dense_from_csc(n, colp, rows, vals),
                           B=np.random.default_rng(21).standard_normal((33, n)))
    return _GRID[dims]


# 1
def test_one_dense_front(ctx):
    NB = block_width()
    for n in (1, 5, NB - 1, NB, NB + 1, 200, 4 * NB + 1):
        A, n2 = dense_quasi_definite(n, 100 + n)
        colp, rows, vals = dense_csc(A)
        b = np.random.default_rng(n).standard_normal(n)
        s = ldlt_solver(ctx, n, colp, rows, vals)
        assert s.num_snodes == 1 and s.max_front == n
        assert s.inertia() == (n - n2, n2, 0)
        check_solution("dense_n%d" % n, A, s.solve(b), b, s.inertia(), restate=True)


# 2
@pytest.mark.parametrize("dims", [(12, 12, 12), (14, 13, 11)])
def test_tree_of_blocked_fronts(ctx, dims):
    k = grid_case(ctx, dims)
    s, n = k["s"], k["n"]
    NB = s.block_width
    assert s.max_snode > 2 * NB and s.max_snode % NB != 0  # more than two block columns and a partial one
    sizes = np.diff(s.snode_first)
    nnzL, colcount = symbolic_fill(n, k["colp"], k["rows"], s.perm)
    assert nnzL == s.nnzL
    below = colcount[s.snode_first[:-1]] - sizes
    assert ((sizes > NB) & (below > 0)).any()  # a blocked front that also has an update matrix
    assert s.max_front == (sizes + below).max()
    nodd = int(k["odd"].sum())
    assert (n - nodd, nodd) == {(12, 12, 12): (864, 864), (14, 13, 11): (1001, 1001)}[dims]
    assert s.inertia() == (n - nodd, nodd, 0)
    b = np.random.default_rng(3).standard_normal(n)
    check_solution("grid3_%dx%dx%d" % dims, k["A"], s.solve(b), b, s.inertia())


# 3
@pytest.mark.parametrize("system", ["grid3_12x12x12", "dense_4NB+1"])
def test_all_plus_signs_give_the_bits_of_cholesky(ctx, system):
    import paropt_amd as pa

    if system.startswith("grid3"):
        n, colp, rows, vals = grid3_system((12, 12, 12), 7)
    else:
        n = 4 * block_width() + 1
        colp, rows, vals = dense_csc(dense_spd(n, 100 + n))
    B = np.random.default_rng(31).standard_normal((3, n))
    llt = pa.SparseCholesky(ctx, n, colp, rows)
    llt.set_values(vals)
    assert llt.factor() == 0 and llt.inertia() == (n, 0, 0)
    X = llt.solve(B)
    plus = ldlt_solver(ctx, n, colp, rows, vals)
    assert plus.inertia() == (n, 0, 0)
    assert np.array_equal(plus.solve(B), X)
    minus = ldlt_solver(ctx, n, colp, rows, -vals)
    assert minus.inertia() == (0, n, 0)
    assert np.array_equal(minus.solve(B), -X)
    A = dense_from_csc(n, colp, rows, vals)
    check_solution(system + "|minus", -A, minus.solve(B[0]), B[0], minus.inertia())


def packed_systems():
    n, colp, rows, vals, neg = tridiag_quasi_definite(200)
    yield "tridiag200", n, colp, rows, vals, "nd", int(neg.sum())
    n, colp, rows, vals, neg = clique8_quasi_definite()
    yield "clique8", n, colp, rows, vals, "natural", int(neg.sum())


# 4
def test_packing_does_not_change_bits(ctx):
    for name, n, colp, rows, vals, order, nneg in packed_systems():
        A = dense_from_csc(n, colp, rows, vals)
        B = np.random.default_rng(17).standard_normal((3, n))
        ref = None
        for cap in CAPS:
            s = ldlt_solver(ctx, n, colp, rows, vals, order=order, cap=cap)
            assert s.packing()["cap"] == cap and (s.kernel_forms()["pack_factor"] > 0) == (cap > 0)
            X = s.solve(B)
            assert s.inertia() == (n - nneg, nneg, 0)
            if ref is None:
                ref = X
            assert np.array_equal(X, ref), (name, cap, float(np.abs(X - ref).max()))
            for j in range(3):
                check_solution("%s|cap%d|rhs%d" % (name, cap, j), A, X[j], B[j], s.inertia(), restate=True)


# 5
def test_every_rhs_column_equals_the_single_solve(ctx):
    k = grid_case(ctx, (12, 12, 12))
    n, colp, rows, vals, _ = tridiag_quasi_definite(200)
    tri = ldlt_solver(ctx, n, colp, rows, vals, cap=16)
    assert tri.kernel_forms()["pack_fwd"] > 0
    for s, B in ((k["s"], k["B"]), (tri, np.random.default_rng(22).standard_normal((33, n)))):
        singles = [s.solve(B[j]) for j in range(33)]
        for nrhs in NRHS:
            X = s.solve(B[:nrhs])
            assert X.shape == (nrhs, s.size)
            for j in range(nrhs):
                assert np.array_equal(X[j], singles[j]), (s.size, nrhs, j)


# 6
def test_zero_pivot_is_reported_and_survived(ctx):
    import paropt_amd as pa

    n, colp, rows, vals, spd = zero_pivot_system()
    s = pa.SparseCholesky(ctx, n, colp, rows, order="natural", factorization="ldlt")
    s.set_values(vals)
    info = s.factor()
    pos = int(np.nonzero(s.perm == 1)[0][0])
    assert np.array_equal(s.perm[:3], [0, 1, 2])  # (the natural order eliminates 0 before 1: the pivot is the zero)
    assert info == 1 + pos, (info, pos)
    inertia = s.inertia()
    assert inertia[2] == 1 and sum(inertia) == n
    assert inertia == inertia_of(*ldlt_nopivot(dense_from_csc(n, colp, rows, vals))[1:])
    assert np.isfinite(s.solve(np.ones(n))).all()
    PARITY["zero_pivot"] = {"info": info, "inertia": list(inertia)}
    s.set_factorization("llt")
    s.set_values(vals)  # (Cholesky on the same values: the pivot is reported, the pivots it replaces are not counted)
    assert s.factor() == 1 + pos
    with pytest.raises(pa.ParOptAMDError) as e:
        s.inertia()
    assert "does not count" in str(e.value)
    s.set_values(spd)
    assert s.factor() == 0 and s.inertia() == (n, 0, 0)
    A = dense_from_csc(n, colp, rows, spd)
    b = np.random.default_rng(61).standard_normal(n)
    check_solution("zero_pivot|llt_refill", A, s.solve(b), b, s.inertia())


# 7
def test_mode_switching_and_refactoring_on_one_handle(ctx):
    import torch

    import paropt_amd as pa

    n, colp, rows, spd = grid3_system((12, 12, 12), 7)
    k = grid_case(ctx, (12, 12, 12))
    B = k["B"][:3]
    s = pa.SparseCholesky(ctx, n, colp, rows)
    s.set_values(spd)
    assert s.factor() == 0 and s.inertia() == (n, 0, 0)
    first = s.solve(B)
    s.set_factorization("ldlt")
    s.set_values(k["vals"])
    assert s.factor() == 0 and s.inertia() == (864, 864, 0)
    X = s.solve(B)
    assert np.array_equal(X, k["s"].solve(B))  # (a handle that never was anything else)
    check_solution("grid3_12x12x12|switched", k["A"], X[0], B[0], s.inertia())
    # device values and device right-hand sides in LDLT mode
    dev = torch.device("cuda", ctx.device())
    s.set_values_device(torch.from_numpy(k["vals"]).to(dev))
    assert s.factor() == 0 and s.inertia() == (864, 864, 0)
    t = torch.from_numpy(B).to(dev)
    assert s.solve_tensor(t) is t
    assert np.array_equal(t.cpu().numpy(), X)
    t1 = torch.from_numpy(B[0]).to(dev)
    assert np.array_equal(s.solve_tensor(t1).cpu().numpy(), X[0])
    s.set_factorization("llt")
    assert s.factorization == "llt"
    s.set_values(spd)
    assert s.factor() == 0 and s.inertia() == (n, 0, 0)
    assert np.array_equal(s.solve(B), first)


# 8
def test_cpp_example(ctx, tmp_path):
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "sparse_ldlt_amd"], env=env,
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "examples", "sparse_ldlt_amd")
    res = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    K, nm = bordered_mass_system(8)
    n = K.shape[0]
    assert "inertia: %d %d 0" % (nm, n - nm) in res.stdout.splitlines()
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("||x - e||_inf:")][-1]
    err = float(line.split(":")[1])
    e = np.ones(n)
    bound, _ = bound_for(K, K @ e)
    PARITY["bordered_mass8|cpp_example"] = {"x_err_device": err, "bound": 16.0 * bound}
    assert err <= 16.0 * bound * np.abs(e).max(), (err, bound)
