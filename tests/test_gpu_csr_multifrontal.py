"""GPU: the CSR sparse constraints on the multifrontal engine (Problem(..., sparse_factor="multifrontal"),
po_problem_set_sparse_factor): S0 assembled straight into the front panels of ParOptSparseCholesky's engine, its
factorization, and the pointer-table panel sweeps of paropt_amd/csrc/sparse_chol.hip behind every solve.

The patterns and the symbolic facts they were chosen for (tests/test_csr_multifrontal_symbolic.py: SHAPES) straddle
the engine's constants kCholSmall = kCholNB = 32 and kCholTile = 64; every test asserts them before it uses the device.
Tolerances are those of tests/test_gpu_csr.py, tests/test_gpu_csr_dense_columns.py and tests/test_gpu_csr_forms.py."""
import gc
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern, dense_jacobian, grid_pattern
from test_csr_multifrontal_symbolic import PATTERNS, SHAPES, assert_shape

pytestmark = pytest.mark.gpu

TOL_MAT = 1e-11  # tests/test_gpu_csr_forms.py
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def _vec(ctx, arr):
    import paropt_amd as pa

    return pa.PVec(ctx, len(arr)).from_numpy(np.asarray(arr, dtype=float))


def pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=0, sparse_factor="multifrontal", before=None):
    """tests/test_gpu_csr.py: PatternProblem (fixed Jacobian entries, linear sparse constraints) on the chosen engine,
    with the entries uploaded by one gradient evaluation; before(prob) is called ahead of that evaluation"""
    import paropt_amd as pa

    A = dense_jacobian(n, rowp, cols, data)

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=len(rowp) - 1, nwinequality=len(rowp) - 1, rowp=rowp, cols=cols,
                             dense_column_rows=dense_column_rows, sparse_factor=sparse_factor)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = 1.0 - A @ x
            return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x)])

        def evalSparseObjConGradient(self, x, g, Ac, d):
            g[:] = 2.0 * x
            Ac[0][:] = -1.0
            d[:] = data
            return 0

    prob = _P()
    assert prob.sparse_factor == sparse_factor
    if before is not None:
        before(prob)
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()
    return prob, A


def symbolic_shape(name, n, rowp, cols, dense_column_rows=0):
    import paropt_amd as pa

    assert_shape(name, pa.CsrSymbolic(n, rowp, cols, dense_column_rows=dense_column_rows,
                                      sparse_factor="multifrontal"))


def check_solves(ctx, prob, A, n, w, rng, r=0, sparse_factor="multifrontal"):
    """factor + apply with and without bw against np.linalg.solve on the dense S (tests/test_gpu_csr.py:
    test_quasidef_solve_matches_dense), C left alone, a repeated factor + apply bit-identical; the factor line names
    supernodes on the multifrontal engine and levels on the row factor"""
    import paropt_amd as pa

    x = _vec(ctx, np.full(n, 0.5))
    d = rng.uniform(0.2, 3.0, size=n)
    c = rng.uniform(0.05, 2.0, size=w)
    S = np.diag(c) + (A * d) @ A.T
    dv, cv = _vec(ctx, d), _vec(ctx, c)
    pa.quasidef_factor(prob, x, dv, cv)
    np.testing.assert_array_equal(cv.to_numpy(), c)
    info = pa.quasidef_factor_info(prob)
    assert info and "nnz(L)" in info and "nnz(K)" in info and "sparsity(L)" in info, info
    assert ("nsnodes" if sparse_factor == "multifrontal" else "nlevels") in info, info
    assert info.endswith(" ndense %d" % r) if r else "ndense" not in info, info
    for with_bw in (True, False):
        bx = rng.standard_normal(n)
        bw = rng.standard_normal(w) if with_bw else None
        yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
        pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, bx), _vec(ctx, bw) if with_bw else None, yx, yw)
        rhs = (bw if with_bw else 0.0) - A @ (d * bx)
        yw_ref = np.linalg.solve(S, rhs)
        yx_ref = d * (bx + A.T @ yw_ref)
        err_w = float(np.abs(yw.to_numpy() - yw_ref).max())
        err_x = float(np.abs(yx.to_numpy() - yx_ref).max())
        print("solve bw=%s: |dyw| %.3e of %.3e, |dyx| %.3e of %.3e" % (with_bw, err_w, np.abs(yw_ref).max(), err_x,
                                                                      np.abs(yx_ref).max()))
        np.testing.assert_allclose(yw.to_numpy(), yw_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yw_ref).max()))
        np.testing.assert_allclose(yx.to_numpy(), yx_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yx_ref).max()))
    yx1, yw1 = yx.to_numpy(), yw.to_numpy()
    pa.quasidef_factor(prob, x, dv, cv)
    yx2, yw2 = pa.PVec(ctx, n), pa.PVec(ctx, w)
    pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, bx), None, yx2, yw2)
    np.testing.assert_array_equal(yw2.to_numpy(), yw1)
    np.testing.assert_array_equal(yx2.to_numpy(), yx1)


SOLVE_PATTERNS = sorted(k for k in PATTERNS if k != "w0")


@pytest.mark.parametrize("name", SOLVE_PATTERNS)
def test_quasidef_solve_matches_dense(ctx, name):
    n, rowp, cols = PATTERNS[name]()
    w = len(rowp) - 1
    symbolic_shape(name, n, rowp, cols)
    rng = np.random.default_rng(5)
    data = rng.uniform(-1.5, 1.5, size=int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data)
    check_solves(ctx, prob, A, n, w, rng)


def test_no_sparse_rows_at_all(ctx):
    """w = 0 through the CSR entry point on the multifrontal engine (tests/test_gpu_csr.py:
    test_empty_and_tiny_csr_patterns)"""
    import paropt_amd as pa

    n, rowp, cols = PATTERNS["w0"]()
    symbolic_shape("w0", n, rowp, cols)
    prob = pa.SeparableProblem(ctx, "quadratic", 1, 1).setChain(2, 1, sparse_factor="multifrontal")
    assert prob.nwcon == 0 and prob.sparse_factor == "multifrontal"
    ip = pa.InteriorPoint(prob, dict(OPTS, max_major_iters=5))
    ip.optimize()
    assert ip.getOptimizedSparse() is None


def hash_panel(ctx, n, nv):
    """tests/test_gpu_csr_forms.py: hash-filled columns with a different mean each, device and numpy"""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    step = 0.1 if nv <= 80 else 0.01
    idx = np.arange(n, dtype=np.uint64)
    V = [pa.PVec(ctx, n).fill_hash(0, 20 + j, 0, 2.0, -1.0 + step * j) for j in range(nv)]
    P = np.stack([-1.0 + step * j + 2.0 * po.u01(0, 20 + j, idx) for j in range(nv)], axis=1)
    return V, P


_GRID = {}


def grid_case(ctx):
    """grid_pattern(26, 24) on the device with its factor, and the numpy side of the same S; made once"""
    import paropt_amd as pa
    from scipy.linalg import cho_factor

    if not _GRID:
        n, rowp, cols = PATTERNS["grid_26_24"]()
        w = len(rowp) - 1
        symbolic_shape("grid_26_24", n, rowp, cols)
        rng = np.random.default_rng(5)
        data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
        prob, A = pattern_problem(ctx, n, rowp, cols, data)
        d = rng.uniform(0.2, 3.0, size=n)
        c = rng.uniform(0.5, 2.0, size=w)
        S = np.diag(c) + (A * d) @ A.T
        x, dv, cv = _vec(ctx, np.full(n, 0.5)), _vec(ctx, d), _vec(ctx, c)
        pa.quasidef_factor(prob, x, dv, cv)
        _GRID.update(n=n, w=w, prob=prob, A=A, d=d, S=S, chol=cho_factor(S, lower=True), x=x, dv=dv, cv=cv,
                     norm=float(np.abs(S).sum(axis=1).max()))
    return _GRID


@pytest.mark.parametrize("nv", [1, 5, 33, 97])
def test_gram_correction(ctx, nv):
    """pa.quasidef_gram across the 32-column slab of the sweeps and the 96-column slab of the pointer tables: W2 and
    the correction vector against dense numpy in the measures and bounds of tests/test_gpu_csr_forms.py
    (test_panel_solves_stand_alone); every column of the 97-wide panel equals the column solved alone, bit for bit."""
    import paropt_amd as pa
    from scipy.linalg import cho_solve

    k = grid_case(ctx)
    V, P = hash_panel(ctx, k["n"], nv)
    alpha = np.random.default_rng(nv).standard_normal(nv)
    W2, out = pa.quasidef_gram(k["prob"], k["x"], k["dv"], k["cv"], V, alpha=alpha)
    out = out.to_numpy()
    U = k["A"] @ (k["d"][:, None] * P)
    Wref = U.T @ cho_solve(k["chol"], U)
    dg = np.sqrt(np.abs(np.diag(Wref)))
    err = float((np.abs(W2 - Wref) / np.outer(dg, dg)).max())

    def eta(y, b):
        return float(np.abs(b - k["S"] @ y).max() / (k["norm"] * np.abs(y).max() + np.abs(b).max()))

    b = U @ alpha
    e_dev, e_lap = eta(-out, b), eta(cho_solve(k["chol"], b), b)
    bound = max(16.0 * e_lap, 64.0 * EPS) + 2.0 * 2 * EPS  # (rows of Aw have 2 entries)
    print("gram nv=%d: W err %.3e (bound %.0e), eta device %.3e lapack %.3e bound %.3e" % (nv, err, TOL_MAT, e_dev,
                                                                                         e_lap, bound))
    assert np.isfinite(W2).all() and np.isfinite(out).all()
    assert err <= TOL_MAT
    np.testing.assert_array_equal(W2, W2.T)
    assert e_dev <= bound
    if nv == 97:
        for j in range(nv):
            e = np.zeros(nv)
            e[j] = 1.0
            wide = pa.quasidef_gram(k["prob"], k["x"], k["dv"], k["cv"], V, alpha=e)[1].to_numpy()
            narrow = pa.quasidef_gram(k["prob"], k["x"], k["dv"], k["cv"], [V[j]], alpha=[1.0])[1].to_numpy()
            np.testing.assert_array_equal(wide, narrow, err_msg="column %d" % j)


def test_half_solved_panel_columns_equal_the_single_solve(ctx):
    """The forward sweep itself: W2[j, j] = |L^-1 U_j|^2 of a 97-wide panel (slabs of 32, 32, 32, 1 columns) equals
    the 1 x 1 Gram of the column alone, bit for bit, for every column."""
    import paropt_amd as pa

    k = grid_case(ctx)
    V, _ = hash_panel(ctx, k["n"], 97)
    W2, _ = pa.quasidef_gram(k["prob"], k["x"], k["dv"], k["cv"], V)
    for j in (0, 1, 31, 32, 63, 64, 95, 96):
        W1, _ = pa.quasidef_gram(k["prob"], k["x"], k["dv"], k["cv"], [V[j]])
        assert W1[0, 0] == W2[j, j], (j, W1[0, 0], W2[j, j])


DENSE_CASES = {
    "chain2_r1": lambda: ("chain2", add_dense_columns(300, *chain_pattern(300, 2, 1), 1), 100, 1),
    "chain2_r2": lambda: ("chain2", add_dense_columns(300, *chain_pattern(300, 2, 1), 2), 100, 2),
    "chain2_r9": lambda: ("chain2", add_dense_columns(300, *chain_pattern(300, 2, 1), 9), 100, 9),
    "grid_26_24_r2": lambda: ("grid_26_24", add_dense_columns(26 * 24, *grid_pattern(26, 24), 2), 600, 2),
}


@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_dense_columns_on_the_multifrontal_engine(ctx, name):
    shape, (n, rowp, cols), min_rows, r = DENSE_CASES[name]()
    w = len(rowp) - 1
    symbolic_shape(shape, n, rowp, cols, dense_column_rows=min_rows)
    rng = np.random.default_rng(5)
    data = rng.uniform(-1.5, 1.5, size=int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=min_rows)
    assert prob.dense_columns == list(range(n - r, n))
    check_solves(ctx, prob, A, n, w, rng, r=r)


def test_gram_with_dense_columns(ctx):
    """the solved-panel form (CsrDenseColumnSolver) over the new sweeps: forward, low-rank step, backward"""
    import paropt_amd as pa

    shape, (n, rowp, cols), min_rows, r = DENSE_CASES["grid_26_24_r2"]()
    w = len(rowp) - 1
    rng = np.random.default_rng(6)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=min_rows)
    d, c = rng.uniform(0.2, 3.0, size=n), rng.uniform(0.5, 2.0, size=w)
    S = np.diag(c) + (A * d) @ A.T
    x, dv, cv = _vec(ctx, np.full(n, 0.5)), _vec(ctx, d), _vec(ctx, c)
    pa.quasidef_factor(prob, x, dv, cv)
    nv = 33
    V, P = hash_panel(ctx, n, nv)
    alpha = rng.standard_normal(nv)
    W2, out = pa.quasidef_gram(prob, x, dv, cv, V, alpha=alpha)
    U = A @ (d[:, None] * P)
    Wref = U.T @ np.linalg.solve(S, U)
    dg = np.sqrt(np.abs(np.diag(Wref)))
    err = float((np.abs(W2 - Wref) / np.outer(dg, dg)).max())
    ref = -np.linalg.solve(S, U @ alpha)
    print("gram with dense columns: W err %.3e, |dout| %.3e of %.3e" % (err, np.abs(out.to_numpy() - ref).max(),
                                                                      np.abs(ref).max()))
    assert err <= TOL_MAT
    np.testing.assert_allclose(out.to_numpy(), ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))


OPTS = {"abs_res_tol": 1e-8, "starting_point_strategy": "affine_step", "barrier_strategy": "monotone",
        "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0, "qn_subspace_size": 6, "qn_type": "bfgs",
        "max_major_iters": 40}  # tests/test_gpu_csr.py


def test_interior_point_on_grid_pattern(ctx):
    """The problem of tests/test_gpu_csr.py: test_interior_point_on_grid_pattern_with_fronts on the multifrontal
    engine against the numpy oracle with a dense S, to that test's tolerances."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    nx, ny = 26, 24
    n = nx * ny
    rowp, cols = grid_pattern(nx, ny)
    w = len(rowp) - 1
    symbolic_shape("grid_26_24", n, rowp, cols)
    rng = np.random.default_rng(11)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    A = dense_jacobian(n, rowp, cols, data)
    xt = rng.uniform(0.2, 0.8, size=n)
    b = A @ rng.uniform(0.3, 0.6, size=n) + 0.05  # cw = b - A x >= 0 is feasible
    a0 = rng.uniform(0.5, 1.0, size=n)

    def f_g(x):
        return float(np.sum((x - xt) ** 2)), 2.0 * (x - xt)

    class P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=w, nwinequality=w, rowp=rowp, cols=cols,
                             sparse_factor="multifrontal")

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = b - A @ x
            return 0, f_g(x)[0], np.array([0.45 * np.sum(a0) - a0 @ x])

        def evalSparseObjConGradient(self, x, g, Ac, d):
            g[:] = f_g(x)[1]
            Ac[0][:] = -a0
            d[:] = -data  # the Jacobian of cw = b - A x
            return 0

    class O:
        comm = po.SelfComm()
        nlocal, c, nwcon, nwineq, csr_form = n, 1, w, w, True

        def vars_and_bounds(self):
            return np.full(n, 0.5), np.zeros(n), np.ones(n)

        def eval_obj_con(self, x):
            self._cw = b - A @ x
            return 0, f_g(x)[0], np.array([0.45 * np.sum(a0) - a0 @ x])

        def eval_obj_con_gradient(self, x):
            return 0, f_g(x)[1], [-a0.copy()]

        def eval_sparse_con(self, x):
            return self._cw.copy()

        def sparse_jacobian_dense(self):
            return -A

        def add_sparse_jacobian(self, alpha, px, out):
            out -= alpha * (A @ px)
            return out

        def add_sparse_jacobian_transpose(self, alpha, pzw, out):
            out -= alpha * (A.T @ pzw)
            return out

    opts = dict(OPTS, max_major_iters=60)
    prob = P()
    ip = pa.InteriorPoint(prob, opts)
    ip.optimize()
    assert "nsnodes" in pa.quasidef_factor_info(prob)
    oip = po.InteriorPoint(O(), dict(opts))
    oip.optimize()
    zw = ip.getOptimizedSparse()[0].to_numpy()
    print("counters", tuple(ip.getIterationCounters()), (oip.niter, oip.neval, oip.ngeval), "fobj",
          ip.getObjective()[0], oip.fobj, "|dx| %.3e |dzw| %.3e of %.3e" % (
              np.abs(ip.getOptimizedPoint()[0].to_numpy() - oip.vars.x).max(), np.abs(zw - oip.vars.zw).max(),
              np.abs(oip.vars.zw).max()))
    assert tuple(ip.getIterationCounters()) == (oip.niter, oip.neval, oip.ngeval)
    assert abs(ip.getObjective()[0] - oip.fobj) <= 1e-8 * max(1.0, abs(oip.fobj))
    np.testing.assert_allclose(ip.getOptimizedPoint()[0].to_numpy(), oip.vars.x, rtol=0, atol=1e-7)
    np.testing.assert_allclose(zw, oip.vars.zw, rtol=0, atol=1e-6 * max(1.0, np.abs(oip.vars.zw).max()))


@pytest.mark.parametrize("dense_vars", [0, 2])
def test_builtin_chain_on_both_engines(ctx, dense_vars):
    """setChain(..., sparse_factor=...), its dense variables included: the two engines take the same path"""
    import paropt_amd as pa

    runs = {}
    for kind in ("rows", "multifrontal"):
        prob = pa.SeparableProblem(ctx, "convex", 500, 3).setChain(
            3, 2, True, dense_vars=dense_vars, dense_column_rows=100 if dense_vars else 0, sparse_factor=kind)
        assert prob.sparse_factor == kind and len(prob.dense_columns) == dense_vars
        ip = pa.InteriorPoint(prob, dict(OPTS, max_major_iters=60))
        ip.optimize()
        info = pa.quasidef_factor_info(prob)
        assert ("nsnodes" in info) == (kind == "multifrontal"), info
        assert info.endswith(" ndense %d" % dense_vars) if dense_vars else "ndense" not in info, info
        runs[kind] = (tuple(ip.getIterationCounters()), ip.getObjective()[0], ip.getOptimizedPoint()[0].to_numpy())
    print({k: v[:2] for k, v in runs.items()})
    assert runs["rows"][0] == runs["multifrontal"][0]
    assert abs(runs["rows"][1] - runs["multifrontal"][1]) <= 1e-8 * max(1.0, abs(runs["rows"][1]))
    np.testing.assert_allclose(runs["multifrontal"][2], runs["rows"][2], rtol=0, atol=1e-7)


def test_non_spd_is_reported_and_the_next_factor_succeeds(ctx):
    """tests/test_gpu_csr.py: test_non_spd_is_reported on the multifrontal engine; the text names the permuted index
    (every pivot fails here and the smallest index is kept: 0), and good data factor afterwards"""
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    n, rowp, cols = PATTERNS["chain2"]()
    w = len(rowp) - 1
    data = np.ones(int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data)
    x = _vec(ctx, np.full(n, 0.5))
    with pytest.raises(ParOptAMDError, match="non-positive pivot in row 0 of the permuted.*min C -1.000e\\+01"):
        pa.quasidef_factor(prob, x, _vec(ctx, np.ones(n)), _vec(ctx, np.full(w, -10.0)))
    # one bad row: its own permuted index
    sym = pa.CsrSymbolic(n, rowp, cols, sparse_factor="multifrontal")
    pos = 137
    c_bad = np.full(w, 1.0)
    c_bad[sym.perm[pos]] = -10.0
    with pytest.raises(ParOptAMDError, match="non-positive pivot in row %d of the permuted" % pos):
        pa.quasidef_factor(prob, x, _vec(ctx, np.full(n, 0.25)), _vec(ctx, c_bad))
    check_solves(ctx, prob, A, n, w, np.random.default_rng(9))


def test_setter_refusals(ctx):
    import paropt_amd as pa
    from paropt_amd import lib as L

    prob = pa.SeparableProblem(ctx, "convex", 64, 2)
    assert prob.sparse_factor == "rows"
    assert L.lib.po_problem_set_sparse_factor(prob.handle, 2) != 0
    assert "unknown kind 2" in L.lib.po_last_error().decode()
    assert L.lib.po_problem_set_sparse_factor(prob.handle, 1) == 0 and prob.sparse_factor == "multifrontal"
    assert L.lib.po_problem_set_sparse_factor(prob.handle, 0) == 0
    prob.setChain(3, 2)
    assert L.lib.po_problem_set_sparse_factor(prob.handle, 1) != 0
    assert "already set" in L.lib.po_last_error().decode()
    assert prob.sparse_factor == "rows"
    with pytest.raises(ValueError, match="sparse_factor"):
        pa.SeparableProblem(ctx, "convex", 64, 2).setChain(3, 2, sparse_factor="frontal")


def test_grouped_pattern_ignores_the_setting_until_it_falls_back(ctx):
    """A block-diagonal pattern is recognised as the grouped form (no factor at all); with non-uniform entries it falls
    back to the CSR form, and then on the engine that was asked for."""
    import paropt_amd as pa

    n, (rowp, cols) = 240, chain_pattern(240, 4, 4)
    w = len(rowp) - 1
    rng = np.random.default_rng(3)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data)  # (the gradient evaluation writes non-uniform entries)
    assert prob.sparse_factor == "multifrontal"
    check_solves(ctx, prob, A, n, w, rng)


def test_facade_example_names_supernodes(tmp_path):
    """examples/sparse_rosenbrock_amd.cpp with factor=multifrontal (ParOptSparseProblem::setSparseFactor), in the
    manner of tests/test_cpp_quasidef_example.py: the reference's trajectory, and a factor line with supernodes"""
    from conftest import load_golden

    exe = str(tmp_path / "sparse_rosenbrock_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "sparse_rosenbrock_amd.cpp"),
                           "-L" + os.path.join(ROOT, "paropt_amd"), "-lparopt_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "paropt_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    res = subprocess.run([exe, "nvars=100", "factor=multifrontal"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    g, _ = load_golden("ipcsr_rosenbrock_n100_chain2")
    np.testing.assert_array_equal(np.array([out["niter"], out["neval"], out["ngeval"]]), g["final/counters"])
    assert abs(out["fobj"] - g["final/fobj"][0]) <= 1e-6 * max(1.0, abs(g["final/fobj"][0]))
    np.testing.assert_allclose(out["xnorm"], g["final/norms"][0], rtol=1e-7)
    assert "nsnodes" in out["factor_info"] and "nnz(L)" in out["factor_info"], out["factor_info"]


def test_multifrontal_problems_give_their_memory_back():
    """tests/test_gpu_leaks.py's counters around ten multifrontal problems, interior point and stand-alone solves"""
    import paropt_amd as pa

    ctx = pa.Context(0)
    gc.collect()
    base, base_mirrors = pa.live_objects(), pa.live_host_mirrors()
    n, rowp, cols = PATTERNS["grid_12_11"]()
    data = np.random.default_rng(1).uniform(0.5, 1.5, size=int(rowp[-1]))
    for it in range(10):
        if it % 2:
            prob = pa.SeparableProblem(ctx, "convex", 200, 2).setChain(3, 2, sparse_factor="multifrontal")
            ip = pa.InteriorPoint(prob, dict(OPTS, max_major_iters=5))
            ip.optimize()
            del ip
        else:
            prob, _ = pattern_problem(ctx, n, rowp, cols, data)
            x, dv, cv = _vec(ctx, np.full(n, 0.5)), _vec(ctx, np.ones(n)), _vec(ctx, np.ones(len(rowp) - 1))
            pa.quasidef_factor(prob, x, dv, cv)
            del x, dv, cv
        del prob
        gc.collect()
        ctx.synchronize()
        assert pa.live_objects() == base, (it, pa.live_objects(), base)
        assert pa.live_host_mirrors() == base_mirrors
    ctx.close()
