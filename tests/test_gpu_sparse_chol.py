"""pa.SparseCholesky on the device: the multifrontal factorization and its solves against LAPACK's dense Cholesky.

The quantity compared is the normwise backward error eta(x) = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), with
A x computed in numpy from the input entries.  The measure is the dense Cholesky solve of the same system
(scipy.linalg.cho_solve, LAPACK potrf/potrs), computed here: a direct solve is unique up to round-off.  The device must
reach eta <= max(16 eta_LAPACK, 64 eps): another elimination order and another blocking change the constant of the
backward-error bound, not its order, fp64 MFMA is plain IEEE fma, and the 64 eps floor is for the cases where LAPACK
happens to be exact (on the mass matrix with b = A 1 it returns eta = 1 eps).  Where x = e is known, also
||x - e||_inf <= 16 * (that bound); 16 is the condition number of the mass matrix at every size.
Every measured eta goes to profiles/r17_sparse_chol_parity.json."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import (csc_from_triplets, dense_from_csc, forest_triplets, grid3_triplets, mass_triplets,
                                 symbolic_fill, tridiag_triplets)

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
PARITY = {}
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    path = os.path.join(ROOT, "profiles", "r17_sparse_chol_parity.json")
    with open(path, "w") as f:
        json.dump({"eps": EPS, "bound": "eta <= max(16 eta_lapack, 64 eps)", "cases": PARITY}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


def eta(A, x, b):
    return float(np.abs(b - A @ x).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def lapack_solve(key, A, b):
    """dense Cholesky solve, computed once per system"""
    if key not in _REF:
        from scipy.linalg import cho_factor, cho_solve

        _REF[key] = cho_solve(cho_factor(A, lower=True), b)
    return _REF[key]


def check_solution(name, A, x, b, exact=None):
    xl = lapack_solve(name.split("|")[0], A, b)
    e_dev, e_lap = eta(A, x, b), eta(A, xl, b)
    bound = max(16.0 * e_lap, 64.0 * EPS)
    PARITY[name] = {"eta_device": e_dev, "eta_lapack": e_lap, "bound": bound}
    if exact is not None:
        PARITY[name]["x_err_device"] = float(np.abs(x - exact).max())
        PARITY[name]["x_err_lapack"] = float(np.abs(xl - exact).max())
    print(name, PARITY[name])
    assert np.isfinite(x).all()
    assert e_dev <= bound, (name, e_dev, e_lap)
    if exact is not None:
        assert np.abs(x - exact).max() <= 16.0 * bound, (name, np.abs(x - exact).max())


def factor_and_solve(ctx, n, colp, rows, vals, b, order="nd", perm=None):
    import paropt_amd as pa

    s = pa.SparseCholesky(ctx, n, colp, rows, order=order, perm=perm)
    s.set_values(vals)
    assert s.factor() == 0
    return s, s.solve(b)


def dense_spd(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return G @ G.T / n + np.eye(n)


def dense_csc(A):
    n = A.shape[0]
    colp = (np.arange(n + 1) * n).astype(np.intc)
    rows = np.tile(np.arange(n, dtype=np.intc), n)
    return colp, rows, np.ascontiguousarray(A.T).ravel()


def block_width():
    import paropt_amd as pa

    return pa.SparseCholesky(None, 1, [0, 1], [0]).block_width


def test_one_dense_front(ctx):
    NB = block_width()
    for n in (1, 5, NB - 1, NB, NB + 1, 200, 4 * NB + 1):
        A = dense_spd(n, 100 + n)
        colp, rows, vals = dense_csc(A)
        b = np.random.default_rng(n).standard_normal(n)
        s, x = factor_and_solve(ctx, n, colp, rows, vals, b)
        assert s.num_snodes == 1 and s.max_front == n and s.nnzL == n * (n + 1) // 2
        check_solution("dense_n%d" % n, A, x, b)


def grid3_system(dims, seed):
    n, R, C = grid3_triplets(*dims)
    rng = np.random.default_rng(seed)
    V = np.where(R == C, 0.0, -0.5)  # (six neighbours of -1/2 under a diagonal of 4: strictly diagonally dominant)
    V[R == C] = 4.0 + 0.1 * rng.random(n)
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    return n, colp, rows, vals


@pytest.mark.parametrize("dims", [(12, 12, 12), (14, 13, 11)])
def test_fronts_off_the_tile_size(ctx, dims):
    n, colp, rows, vals = grid3_system(dims, 7)
    A = dense_from_csc(n, colp, rows, vals)
    b = np.random.default_rng(3).standard_normal(n)
    s, x = factor_and_solve(ctx, n, colp, rows, vals, b)
    NB = s.block_width
    assert s.max_snode > 2 * NB and s.max_snode % NB != 0  # more than two block columns and a partial one
    sizes = np.diff(s.snode_first)
    nnzL, colcount = symbolic_fill(n, colp, rows, s.perm)
    assert nnzL == s.nnzL
    below = colcount[s.snode_first[:-1]] - sizes
    assert ((sizes > NB) & (below > 0)).any()  # a blocked front that also has an update matrix
    assert s.max_front == (sizes + below).max()
    check_solution("grid3_%dx%dx%d" % dims, A, x, b)


def mass_system(nx):
    n, R, C, V = mass_triplets(nx)
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    return n, colp, rows, vals


@pytest.mark.parametrize("order", ["nd", "amd", "natural"])
def test_mass_matrix_40(ctx, order):
    n, colp, rows, vals = mass_system(40)
    assert n == 3362
    A = dense_from_csc(n, colp, rows, vals)
    b = A @ np.ones(n)
    s, x = factor_and_solve(ctx, n, colp, rows, vals, b, order=order)
    check_solution("mass40|" + order, A, x, b, exact=np.ones(n))


def test_mass_matrix_12_user_perm(ctx):
    n, colp, rows, vals = mass_system(12)
    A = dense_from_csc(n, colp, rows, vals)
    b = A @ np.ones(n)
    perm = np.random.default_rng(5).permutation(n)
    s, x = factor_and_solve(ctx, n, colp, rows, vals, b, order="natural", perm=perm)
    check_solution("mass12|user_perm", A, x, b, exact=np.ones(n))


def test_deep_and_flat_trees(ctx):
    n, R, C, V = tridiag_triplets(1000)
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    A = dense_from_csc(n, colp, rows, vals)
    b = np.random.default_rng(11).standard_normal(n)
    for order in ("natural", "nd"):
        s, x = factor_and_solve(ctx, n, colp, rows, vals, b, order=order)
        check_solution("tridiag1000|" + order, A, x, b)
    n = 300
    d = 1.0 + np.random.default_rng(12).random(n)
    colp, rows = np.arange(n + 1, dtype=np.intc), np.arange(n, dtype=np.intc)
    b = np.random.default_rng(13).standard_normal(n)
    s, x = factor_and_solve(ctx, n, colp, rows, d, b)
    assert s.nlevels == 1 and s.num_snodes == n
    check_solution("diag300", np.diag(d), x, b)
    n, R, C, V = forest_triplets()
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    A = dense_from_csc(n, colp, rows, vals)
    b = np.random.default_rng(14).standard_normal(n)
    s, x = factor_and_solve(ctx, n, colp, rows, vals, b)
    assert (s.snode_parent < 0).sum() >= 3
    check_solution("forest3", A, x, b)


def test_every_rhs_column_equals_the_single_solve(ctx):
    n, colp, rows, vals = grid3_system((12, 12, 12), 7)
    B = np.random.default_rng(21).standard_normal((17, n))
    import paropt_amd as pa

    s = pa.SparseCholesky(ctx, n, colp, rows)
    s.set_values(vals)
    assert s.factor() == 0
    singles = [s.solve(B[j]) for j in range(17)]
    for nrhs in (1, 3, 17):
        X = s.solve(B[:nrhs])
        assert X.shape == (nrhs, n)
        for j in range(nrhs):
            assert np.array_equal(X[j], singles[j]), (nrhs, j)


def test_deterministic_and_refactoring(ctx):
    import paropt_amd as pa

    n, colp, rows, vals = grid3_system((12, 12, 12), 7)
    A = dense_from_csc(n, colp, rows, vals)
    b = np.random.default_rng(31).standard_normal(n)
    s = pa.SparseCholesky(ctx, n, colp, rows)
    xs = []
    for _ in range(2):
        s.set_values(vals)
        assert s.factor() == 0
        xs.append(s.solve(b))
    s2, x2 = factor_and_solve(ctx, n, colp, rows, vals, b)
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], x2)
    # the same object with other values: nothing stale in the arena or the panels
    _, _, _, vals2 = grid3_system((12, 12, 12), 8)
    vals2 = vals2 * 3.0
    A2 = dense_from_csc(n, colp, rows, vals2)
    s.set_values(vals2)
    assert s.factor() == 0
    check_solution("grid3_12x12x12_refactored", A2, s.solve(b), b)
    fresh, xf = factor_and_solve(ctx, n, colp, rows, vals2, b)
    assert np.array_equal(s.solve(b), xf)
    assert not np.array_equal(xf, xs[0])


def test_value_forms(ctx):
    import paropt_amd as pa

    n, R, C, V = mass_triplets(12)  # element by element: every entry of A is the sum of up to four duplicates
    colp, rows, vals = csc_from_triplets(n, R, C, V)
    assert len(rows) > len(set(zip(rows.tolist(), np.repeat(np.arange(n), np.diff(colp)).tolist())))
    A = dense_from_csc(n, colp, rows, vals)
    b = A @ np.ones(n)
    s, x = factor_and_solve(ctx, n, colp, rows, vals, b)
    check_solution("mass12|duplicates", A, x, b, exact=np.ones(n))
    # the general form with the entries of every column in another order
    rng = np.random.default_rng(41)
    order = np.concatenate([colp[j] + rng.permutation(colp[j + 1] - colp[j]) for j in range(n)])
    s.set_values(colp, rows[order], vals[order])
    assert s.factor() == 0
    x2 = s.solve(b)
    check_solution("mass12|permuted_entries", A, x2, b, exact=np.ones(n))
    # unique entries (no duplicate sums whose order could differ): bit for bit the creation-pattern form
    nt, Rt, Ct, Vt = tridiag_triplets(200)
    cp, rw, vl = csc_from_triplets(nt, Rt, Ct, Vt)
    bt = np.random.default_rng(42).standard_normal(nt)
    st, xt = factor_and_solve(ctx, nt, cp, rw, vl, bt)
    flip = np.concatenate([np.arange(cp[j], cp[j + 1])[::-1] for j in range(nt)])
    st.set_values(cp, rw[flip], vl[flip])
    assert st.factor() == 0
    assert np.array_equal(st.solve(bt), xt)
    # an entry outside the factor's pattern is refused
    cp2 = cp.copy()
    cp2[1:] += 1
    rw2 = np.concatenate([[nt - 1], rw]).astype(np.intc)  # (nt-1, 0): far off the three diagonals
    with pytest.raises(pa.ParOptAMDError) as e:
        st.set_values(cp2, rw2, np.concatenate([[1.0], vl]))
    assert "outside the pattern" in str(e.value)


def test_indefinite_matrix_is_reported_and_survived(ctx):
    import paropt_amd as pa

    n, colp, rows, vals = mass_system(40)
    A = dense_from_csc(n, colp, rows, vals)
    s = pa.SparseCholesky(ctx, n, colp, rows)
    bad = 1234
    cols = np.repeat(np.arange(n), np.diff(colp))
    hit = np.nonzero((rows == bad) & (cols == bad))[0]
    v = vals.copy()
    v[hit] = 0.0
    v[hit[0]] = -1.0
    s.set_values(v)
    info = s.factor()
    pos = int(np.nonzero(s.perm == bad)[0][0])
    assert 1 <= info <= 1 + pos, (info, pos)
    assert np.isfinite(s.solve(np.ones(n))).all()
    s.set_values(vals)
    assert s.factor() == 0
    b = A @ np.ones(n)
    check_solution("mass40|after_indefinite", A, s.solve(b), b, exact=np.ones(n))


def test_solve_tensor_equals_solve(ctx):
    import torch

    import paropt_amd as pa

    n, colp, rows, vals = mass_system(12)
    s = pa.SparseCholesky(ctx, n, colp, rows)
    dev = torch.device("cuda", ctx.device())
    s.set_values_device(torch.from_numpy(vals).to(dev))
    assert s.factor() == 0
    B = np.random.default_rng(51).standard_normal((3, n))
    X = s.solve(B)
    t = torch.from_numpy(B).to(dev)
    ptr = t.data_ptr()
    out = s.solve_tensor(t)
    assert out is t and t.data_ptr() == ptr
    assert np.array_equal(t.cpu().numpy(), X)
    t1 = torch.from_numpy(B[0]).to(dev)
    assert np.array_equal(s.solve_tensor(t1).cpu().numpy(), X[0])


def test_cpp_example(ctx, tmp_path):
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "sparse_cholesky_amd"], env=env,
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "examples", "sparse_cholesky_amd")
    res = subprocess.run([exe, "24", "ND"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("||x - e||_inf:")][-1]
    err = float(line.split(":")[1])
    n, colp, rows, vals = mass_system(24)
    A = dense_from_csc(n, colp, rows, vals)
    b = A @ np.ones(n)
    xl = lapack_solve("mass24", A, b)
    bound = max(16.0 * eta(A, xl, b), 64.0 * EPS)
    PARITY["mass24|cpp_example"] = {"x_err_device": err, "bound": 16.0 * bound}
    assert err <= 16.0 * bound, (err, bound)
    for key in ("Setup/order time", "Set values  time", "Factor time", "Solve time"):
        assert key in res.stdout
