"""GPU: the device arrays of the sparse factors are owned (DevArray, paropt_amd/csrc/core.hpp) and counted.  Every
scenario takes pa.live_objects() first and demands the same pair after everything it made is gone, in the manner of
tests/test_gpu_csr_multifrontal.py: test_multifrontal_problems_give_their_memory_back; while a factor is alive the
byte count is above the base, which is what shows that L, the arena, the index tables, the dense-column panels and the
LDLT sign array are in it at all."""
import gc

import numpy as np
import pytest

from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern
from sparse_ldlt_helpers import bound_for, eta, tridiag_quasi_definite
from test_csr_multifrontal_symbolic import PATTERNS
from test_gpu_csr_multifrontal import _vec, check_solves, hash_panel, pattern_problem

pytestmark = pytest.mark.gpu


def settled(ctx):
    import paropt_amd as pa

    gc.collect()
    ctx.synchronize()
    return pa.live_objects()


def test_stand_alone_solver_gives_its_arrays_back():
    """Ten rounds of create, use, destroy of pa.SparseCholesky: LDLT on the odd rounds (the sign array is allocated on
    demand), values by the creation pattern and by another pattern (the lower triangle alone, entries of every column
    reversed: the temporary scatter tables), solves of 1 and of 40 right-hand sides (two slabs; the host-solve buffer
    grows), and an analysis-only object."""
    import paropt_amd as pa

    ctx = pa.Context(0)
    base = settled(ctx)
    n, colp, rows, qd_vals, odd = tridiag_quasi_definite(200)
    cols = np.repeat(np.arange(n), np.diff(colp))
    spd_vals = np.where((rows == cols) & odd[rows], -qd_vals, qd_vals)
    keep = np.nonzero(rows >= cols)[0]
    low = np.concatenate([keep[cols[keep] == j][::-1] for j in range(n)])
    low_colp = np.concatenate([[0], np.cumsum(np.bincount(cols[keep], minlength=n))]).astype(np.intc)
    B = np.random.default_rng(2).standard_normal((40, n))
    for it in range(10):
        ldlt = it % 2 == 1
        vals = qd_vals if ldlt else spd_vals
        # (natural order: the lower triangle of the input is the permuted-lower triangle that is read)
        s = pa.SparseCholesky(ctx, n, colp, rows, order="natural", factorization="ldlt" if ldlt else "llt")
        alive = pa.live_objects()
        assert alive[0] == base[0] and alive[1] > base[1] + 8 * s.nnzL, (it, alive, base)
        s.set_values(vals)
        assert s.factor() == 0
        x1 = s.solve(B[0])
        s.set_values(low_colp, rows[low], vals[low])
        assert s.factor() == 0
        assert s.inertia() == ((n - int(odd.sum()), int(odd.sum()), 0) if ldlt else (n, 0, 0))
        assert np.array_equal(s.solve(B[0]), x1)
        X = s.solve(B)
        assert X.shape == (40, n) and np.array_equal(X[0], x1)
        A = np.zeros((n, n))
        A[rows, cols] = vals
        for j in (0, 31, 32, 39):  # both slabs, to the bound of tests/test_gpu_sparse_ldlt.py
            assert eta(A, X[j], B[j]) <= bound_for(A, B[j])[0], (it, j)
        assert pa.live_objects()[1] > alive[1]  # the buffer of the 40-column host solve (and the sign array)
        h = pa.SparseCholesky(None, n, colp, rows)
        assert h.nnzL > 0
        del h, s
        assert settled(ctx) == base, (it, pa.live_objects(), base)
    ctx.close()


@pytest.mark.parametrize("sparse_factor", ["rows", "multifrontal"])
def test_problem_with_dense_columns_gives_its_arrays_back(sparse_factor):
    """CsrSparse behind a problem, with dense columns: Gram corrections of 8 and then of 40 columns grow the solved
    panel and the dense partials; all of it is gone with the problem."""
    import paropt_amd as pa

    ctx = pa.Context(0)
    base = settled(ctx)
    n0, rowp0, cols0 = PATTERNS["grid_12_11"]()
    n, rowp, cols = add_dense_columns(n0, rowp0, cols0, 2)
    w = len(rowp) - 1
    rng = np.random.default_rng(4)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    prob, A = pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=w // 2, sparse_factor=sparse_factor)
    assert prob.dense_columns == [n - 2, n - 1]
    d, c = rng.uniform(0.2, 3.0, size=n), rng.uniform(0.5, 2.0, size=w)
    S = np.diag(c) + (A * d) @ A.T
    x, dv, cv = _vec(ctx, np.full(n, 0.5)), _vec(ctx, d), _vec(ctx, c)
    pa.quasidef_factor(prob, x, dv, cv)
    before = pa.live_objects()[1]
    for nv in (8, 40):
        V, P = hash_panel(ctx, n, nv)
        W2, _ = pa.quasidef_gram(prob, x, dv, cv, V)
        U = A @ (d[:, None] * P)
        Wref = U.T @ np.linalg.solve(S, U)
        dg = np.sqrt(np.abs(np.diag(Wref)))
        assert float((np.abs(W2 - Wref) / np.outer(dg, dg)).max()) <= 1e-11  # tests/test_gpu_csr_forms.py: TOL_MAT
        del V
    gc.collect()
    assert pa.live_objects()[1] > before  # the 40-column panel and its partials stay with the problem
    del prob, x, dv, cv
    assert settled(ctx) == base, (pa.live_objects(), base)
    ctx.close()


@pytest.mark.parametrize("sparse_factor", ["rows", "multifrontal"])
def test_light_pattern_keeps_its_value_array_through_the_upgrade(sparse_factor):
    """The grouped chain pattern of test_grouped_pattern_ignores_the_setting_until_it_falls_back: the gradient
    evaluation writes non-uniform entries, the analysis runs after all, and the user-visible value array is the same
    device array with those entries in it."""
    import paropt_amd as pa

    ctx = pa.Context(0)
    base = settled(ctx)
    n, (rowp, cols) = 240, chain_pattern(240, 4, 4)
    w = len(rowp) - 1
    rng = np.random.default_rng(3)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    seen = {}

    def before(prob):
        t = prob.getSparseJacobianData(device=True)[2]
        seen["ptr"], seen["light_bytes"] = t.data_ptr(), pa.live_objects()[1]
        assert not t.any().item()

    prob, A = pattern_problem(ctx, n, rowp, cols, data, sparse_factor=sparse_factor, before=before)
    rp, cl, t = prob.getSparseJacobianData(device=True)
    assert t.data_ptr() == seen["ptr"]
    np.testing.assert_array_equal(t.cpu().numpy(), data)
    np.testing.assert_array_equal(prob.getSparseJacobianData()[2], data)
    np.testing.assert_array_equal(rp, rowp)
    np.testing.assert_array_equal(cl, cols)
    assert pa.live_objects()[1] > seen["light_bytes"]  # the analysis' tables and the factor came on top
    check_solves(ctx, prob, A, n, w, rng, sparse_factor=sparse_factor)
    del prob, t
    assert settled(ctx) == base, (pa.live_objects(), base)
    ctx.close()
