"""GPU: dense columns of the CSR sparse constraints solved by low-rank update (paropt_amd/csrc/csr.{cpp,hip},
CsrDenseColumnSolver in quasidef.cpp).  S = C + Aw D^-1 Aw^T = S0 + V E V^T: the sparse Cholesky factors S0, the
r dense columns come back through K = E^-1 + (L^-1 V)^T (L^-1 V).

  * the quasi-definite solve against a dense numpy solve of the whole system (the model is
    test_gpu_csr.test_quasidef_solve_matches_dense: same problem class, data ranges and 1e-10 tolerances);
  * the products, reached the way the existing tests reach them: Aw and the fused transposed product through the
    quasi-definite apply, the plain transposed product inside the interior point, the column sum through the
    Hessian of the built-in chain constraints;
  * w = 70001: several workgroups in the two-stage panel product, residual of the quasi-definite system against the
    numpy restatement of the same solve;
  * the pattern the analysis used to refuse (w = 39999, one epigraph column), in the automatic mode;
  * an interior-point run with the columns split off against the same run on the direct path."""
import numpy as np
import pytest

from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern, dense_jacobian, grid_pattern
from test_gpu_csr import _vec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


class DensePatternProblem:
    """test_gpu_csr.PatternProblem (fixed Jacobian entries, linear sparse constraints) with the dense-column rule
    handed to the constructor."""

    def __new__(cls, ctx, n, rowp, cols, data, dense_column_rows):
        import paropt_amd as pa

        class _P(pa.Problem):
            def __init__(self):
                super().__init__(ctx, n, 1, 1, nwcon=len(rowp) - 1, nwinequality=len(rowp) - 1, rowp=rowp,
                                 cols=cols, dense_column_rows=dense_column_rows)

            def getVarsAndBounds(self, x, lb, ub):
                x[:] = 0.5
                lb[:] = 0.0
                ub[:] = 1.0

            def evalSparseObjCon(self, x, sparse):
                sparse[:] = 1.0 - dense_jacobian(n, rowp, cols, data) @ x
                return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x)])

            def evalSparseObjConGradient(self, x, g, A, d):
                g[:] = 2.0 * x
                A[0][:] = -1.0
                d[:] = data
                return 0

        return _P()


def _only_entry_dense():
    rowp = np.array([0, 0, 2, 2, 3, 3] + [3 + 2 * k for k in range(1, 41)], dtype=np.intc)
    cols = np.array([4, 1, 4] + [c for k in range(40) for c in (5 + k, 6 + k)], dtype=np.intc)
    return add_dense_columns(50, rowp, cols, 1)


# name -> ((n, rowp, cols), dense_column_rows, r)
CASES = {
    "chain2_r1": lambda: (add_dense_columns(300, *chain_pattern(300, 2, 1), 1), 100, 1),
    "chain2_r2": lambda: (add_dense_columns(300, *chain_pattern(300, 2, 1), 2), 100, 2),
    "chain2_r9": lambda: (add_dense_columns(300, *chain_pattern(300, 2, 1), 9), 100, 9),  # crosses the 8-column sweep
    # smallest sizes.  (A single row with a single entry is the grouped pattern and never reaches the CSR form; at
    # w = 1 every column of the row has one entry, so both qualify and S0 = C.)
    "w1_r2": lambda: ((3, np.array([0, 2], dtype=np.intc), np.array([0, 2], dtype=np.intc)), 1, 2),
    "w2_r1": lambda: ((4, np.array([0, 2, 4], dtype=np.intc), np.array([0, 3, 2, 3], dtype=np.intc)), 2, 1),
    "chain5_rev_r2": lambda: (add_dense_columns(257, *chain_pattern(257, 5, 2, reverse=True), 2, first=True), 100, 2),
    "grid_fronts_r2": lambda: (add_dense_columns(26 * 24, *grid_pattern(26, 24), 2), 600, 2),
    "only_entry_dense_r1": lambda: (_only_entry_dense(), 40, 1),
    "sixty_percent_r1": lambda: (add_dense_columns(300, *chain_pattern(300, 2, 1), 1, fraction=0.6, seed=3), 100, 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_quasidef_solve_matches_dense(ctx, name):
    import paropt_amd as pa

    (n, rowp, cols), min_rows, r = CASES[name]()
    w = len(rowp) - 1
    rng = np.random.default_rng(5)
    data = rng.uniform(-1.5, 1.5, size=int(rowp[-1]))
    prob = DensePatternProblem(ctx, n, rowp, cols, data, min_rows)
    assert len(prob.dense_columns) == r and prob.dense_columns == sorted(prob.dense_columns)
    assert prob.dense_columns == ([0, 2] if name == "w1_r2" else list(range(n - r, n)))
    x = _vec(ctx, np.full(n, 0.5))
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()  # one gradient evaluation uploads the entries
    A = dense_jacobian(n, rowp, cols, data)
    d = rng.uniform(0.2, 3.0, size=n)
    c = rng.uniform(0.05, 2.0, size=w)
    S = np.diag(c) + (A * d) @ A.T
    dv, cv = _vec(ctx, d), _vec(ctx, c)
    pa.quasidef_factor(prob, x, dv, cv)
    np.testing.assert_array_equal(cv.to_numpy(), c)
    info = pa.quasidef_factor_info(prob)
    assert info and "nnz(L)" in info and info.endswith(" ndense %d" % r), info
    if name == "grid_fronts_r2":
        assert pa.CsrSymbolic(n, rowp, cols, dense_column_rows=min_rows).nfronts > 0
    for with_bw in (True, False):
        bx = rng.standard_normal(n)
        bw = rng.standard_normal(w) if with_bw else None
        yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
        pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, bx), _vec(ctx, bw) if with_bw else None, yx, yw)
        rhs = (bw if with_bw else 0.0) - A @ (d * bx)
        yw_ref = np.linalg.solve(S, rhs)
        yx_ref = d * (bx + A.T @ yw_ref)  # (the fused transposed product, dense columns included)
        np.testing.assert_allclose(yw.to_numpy(), yw_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yw_ref).max()))
        np.testing.assert_allclose(yx.to_numpy(), yx_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yx_ref).max()))
    # a repeated factor + apply is bit-identical (no atomics, fixed summation order)
    yx1, yw1 = yx.to_numpy(), yw.to_numpy()
    pa.quasidef_factor(prob, x, dv, cv)
    yx2, yw2 = pa.PVec(ctx, n), pa.PVec(ctx, w)
    pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, bx), None, yx2, yw2)
    np.testing.assert_array_equal(yw2.to_numpy(), yw1)
    np.testing.assert_array_equal(yx2.to_numpy(), yx1)


def test_unsplit_factor_line_is_unchanged(ctx):
    import paropt_amd as pa

    (n, rowp, cols), _, _ = CASES["chain2_r2"]()
    data = np.ones(int(rowp[-1]))
    prob = DensePatternProblem(ctx, n, rowp, cols, data, -1)
    assert prob.dense_columns == []
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()
    pa.quasidef_factor(prob, _vec(ctx, np.full(n, 0.5)), _vec(ctx, np.ones(n)), _vec(ctx, np.ones(len(rowp) - 1)))
    assert "ndense" not in pa.quasidef_factor_info(prob)


# ---- large patterns: chain2 plus r variables in every row, products by index arithmetic ------------------------------
class _Chain:
    """Aw of chain_pattern(n0, 2, 1) plus r dense variables, entries `data`, without a dense matrix."""

    def __init__(self, n0, r, seed):
        self.n, self.rowp, self.cols = add_dense_columns(n0, *chain_pattern(n0, 2, 1), r)
        self.n0, self.r, self.w = n0, r, n0 - 1
        rng = np.random.default_rng(seed)
        self.data = rng.uniform(-1.5, 1.5, size=int(self.rowp[-1]))
        self.rows = np.repeat(np.arange(self.w), 2 + r)
        self.d = rng.uniform(0.2, 3.0, size=self.n)
        self.c = rng.uniform(0.05, 2.0, size=self.w)
        self.bx, self.bw = rng.standard_normal(self.n), rng.standard_normal(self.w)

    def mult(self, x):
        return np.bincount(self.rows, weights=self.data * x[self.cols], minlength=self.w)

    def mult_t(self, y):
        return np.bincount(self.cols, weights=self.data * y[self.rows], minlength=self.n)

    def residual(self, yx, yw):
        """max-norms of D yx - Aw^T yw - bx and Aw yx + C yw - bw, scaled by max(1, |y|_inf)"""
        scale = max(1.0, np.abs(yx).max(), np.abs(yw).max())
        r1 = yx / self.d - self.mult_t(yw) - self.bx
        r2 = self.mult(yx) + self.c * yw - self.bw
        return np.abs(r1).max() / scale, np.abs(r2).max() / scale

    def numpy_solve(self):
        """The same low-rank solve in numpy with a banded (here tridiagonal) Cholesky of S0, natural order."""
        w, r, d = self.w, self.r, self.d
        a = self.data.reshape(w, 2 + r)
        diag = self.c + a[:, 0] ** 2 * d[:w] + a[:, 1] ** 2 * d[1:w + 1]
        off = a[:-1, 1] * d[1:w] * a[1:, 0]
        V, E = a[:, 2:].copy(), d[self.n0:]
        ld, lo = np.empty(w), np.empty(w - 1)
        ld[0] = np.sqrt(diag[0])
        for i in range(1, w):
            lo[i - 1] = off[i - 1] / ld[i - 1]
            ld[i] = np.sqrt(diag[i] - lo[i - 1] ** 2)
        rhs = np.column_stack([self.bw - self.mult(d * self.bx), V])
        for i in range(w):  # forward, all r + 1 columns at once
            if i:
                rhs[i] -= lo[i - 1] * rhs[i - 1]
            rhs[i] /= ld[i]
        t, Yv = rhs[:, 0], rhs[:, 1:]
        K = np.diag(1.0 / E) + Yv.T @ Yv
        t = t - Yv @ np.linalg.solve(K, Yv.T @ t)
        for i in range(w - 1, -1, -1):
            if i < w - 1:
                t[i] -= lo[i] * t[i + 1]
            t[i] /= ld[i]
        return d * (self.bx + self.mult_t(t)), t

    def problem(self, ctx, dense_column_rows):
        import paropt_amd as pa

        m = self

        class _P(pa.Problem):
            def __init__(self):
                super().__init__(ctx, m.n, 1, 1, nwcon=m.w, nwinequality=m.w, rowp=m.rowp, cols=m.cols,
                                 dense_column_rows=dense_column_rows)

            def getVarsAndBounds(self, x, lb, ub):
                x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

            def evalSparseObjCon(self, x, sparse):
                sparse[:] = 1.0 - m.mult(x)
                return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x) / m.n])

            def evalSparseObjConGradient(self, x, g, A, dat):
                g[:] = 2.0 * x
                A[0][:] = -1.0 / m.n
                dat[:] = m.data
                return 0

        return _P()

    def device_solve(self, ctx, prob):
        import paropt_amd as pa

        x = _vec(ctx, np.full(self.n, 0.5))
        dv, cv = _vec(ctx, self.d), _vec(ctx, self.c)
        pa.quasidef_factor(prob, x, dv, cv)
        yx, yw = pa.PVec(ctx, self.n), pa.PVec(ctx, self.w)
        pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, self.bx), _vec(ctx, self.bw), yx, yw)
        return yx.to_numpy(), yw.to_numpy()


def _residual_check(m, got, what):
    ref = m.residual(*m.numpy_solve())
    dev = m.residual(*got)
    print("%s: residual (first block, second block) device %.3e %.3e, numpy restatement %.3e %.3e" % (
        (what,) + dev + ref))
    for k in range(2):
        assert dev[k] <= max(1e-12, 100.0 * ref[k]), (what, k, dev, ref)


def test_multi_block_reduction(ctx):
    """w = 70001 (odd, 69 workgroups in the first stage of the panel product), r = 3.  The bound is 100 x the residual
    of the numpy restatement of the same solve on the same data, floor 1e-12.  Measured on an MI355X:
    device 5.3e-14 / 5.1e-12 against numpy 2.5e-17 / 8.8e-11 (first / second block; the second is the conditioning
    of the system at this size, not the method)."""
    import paropt_amd as pa

    m = _Chain(70002, 3, 17)
    assert m.w == 70001
    prob = m.problem(ctx, 1000)
    assert prob.dense_columns == [70002, 70003, 70004]
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()
    _residual_check(m, m.device_solve(ctx, prob), "w=70001 r=3")
    assert pa.quasidef_factor_info(prob).endswith(" ndense 3")


def test_refused_size_runs(ctx):
    """The pattern the analysis refused before the rule (w = 39999, one epigraph column), in the automatic mode."""
    import paropt_amd as pa

    m = _Chain(40000, 1, 23)
    assert (m.n, m.w) == (40001, 39999)
    prob = m.problem(ctx, 0)  # refused at this line without the rule
    assert prob.dense_columns == [40000]
    ip = pa.InteriorPoint(prob, {"max_major_iters": 3, "qn_subspace_size": 5})
    ip.optimize()
    x, z = ip.getOptimizedPoint()[:2]
    zw = ip.getOptimizedSparse()[0].to_numpy()
    assert np.all(np.isfinite(x.to_numpy())) and np.all(np.isfinite(z)) and np.all(np.isfinite(zw))
    assert ip.getIterationCounters()[0] == 3
    _residual_check(m, m.device_solve(ctx, prob), "w=39999 r=1 (automatic)")


# ---- interior point: split against unsplit ----------------------------------------------------------------------------
def _ip_problem(ctx, dense_column_rows):
    """Strictly convex separable objective, bounds [0, 1], one dense constraint and the linear sparse constraints
    cw = b - Aw x >= 0 on chain2 (w = 299) plus two variables that enter every row."""
    import paropt_amd as pa

    n, rowp, cols = add_dense_columns(300, *chain_pattern(300, 2, 1), 2)
    w = len(rowp) - 1
    rng = np.random.default_rng(11)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    A = dense_jacobian(n, rowp, cols, data)
    xt = rng.uniform(0.2, 0.8, size=n)
    q = rng.uniform(1.0, 4.0, size=n)
    b = A @ rng.uniform(0.3, 0.6, size=n) + 0.05
    a0 = rng.uniform(0.5, 1.0, size=n)

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=w, nwinequality=w, rowp=rowp, cols=cols,
                             dense_column_rows=dense_column_rows)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = b - A @ x
            return 0, float(np.sum(q * (x - xt) ** 2)), np.array([0.45 * np.sum(a0) - a0 @ x])

        def evalSparseObjConGradient(self, x, g, Ac, d):
            g[:] = 2.0 * q * (x - xt)
            Ac[0][:] = -a0
            d[:] = -data
            return 0

    return _P()


IP_OPTS = {"qn_type": "bfgs", "qn_subspace_size": 5, "starting_point_strategy": "affine_step",
           "barrier_strategy": "monotone", "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0}


def _ip_run(ctx, dense_column_rows, **opts):
    import paropt_amd as pa

    prob = _ip_problem(ctx, dense_column_rows)
    assert prob.dense_columns == ([300, 301] if dense_column_rows > 0 else [])
    ip = pa.InteriorPoint(prob, dict(IP_OPTS, **opts))
    ip.optimize()
    x, z = ip.getOptimizedPoint()[:2]
    return ip, x.to_numpy(), z, ip.getOptimizedSparse()[0].to_numpy()


def test_interior_point_split_matches_unsplit(ctx):
    """gramSolve on a panel of c + 2k = 11 > 8 columns, correction and applyK0 inside the step: the same problem with
    the two columns split off (dense_column_rows = 100) and on the direct path (-1)."""
    # the direct path converges on this problem: it is the reference of everything below
    ref, xr, zr, zwr = _ip_run(ctx, -1, abs_res_tol=1e-6, max_major_iters=200)
    assert ref.getIterationCounters()[0] < 200
    got, xg, zg, zwg = _ip_run(ctx, 100, abs_res_tol=1e-6, max_major_iters=200)
    assert got.getIterationCounters()[0] < 200  # both stop converged
    fr, fg = ref.getObjective()[0], got.getObjective()[0]
    assert abs(fg - fr) <= 1e-6 * max(1.0, abs(fr))
    np.testing.assert_allclose(xg, xr, rtol=0, atol=1e-6)
    # after exactly eight iterations, the tolerance out of reach
    ref, xr, zr, zwr = _ip_run(ctx, -1, abs_res_tol=1e-30, max_major_iters=8)
    got, xg, zg, zwg = _ip_run(ctx, 100, abs_res_tol=1e-30, max_major_iters=8)
    assert ref.getIterationCounters() == got.getIterationCounters() and got.getIterationCounters()[0] == 8
    for a, r in ((xg, xr), (zg, zr), (zwg, zwr)):
        np.testing.assert_allclose(a, r, rtol=0, atol=1e-8 * max(1.0, np.abs(r).max()))


# ---- two ranks on one GPU: only rank 0's shard has dense columns --------------------------------------------------------
def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_problem(ctx, rank, world, reduce):
    """The global problem of 602 variables: rank 0's shard is chain2 on 300 variables plus two variables in every one
    of its rows, rank 1's the same chain on its own 300 variables without them.  rank = None: all of it on one rank.
    `reduce` sums an array over the ranks."""
    import paropt_amd as pa

    rng = np.random.default_rng(29)
    n0, rowp0, cols0 = add_dense_columns(300, *chain_pattern(300, 2, 1), 2)
    rowp1, cols1 = chain_pattern(300, 2, 1)
    data0 = rng.uniform(0.5, 1.5, size=int(rowp0[-1]))
    data1 = rng.uniform(0.5, 1.5, size=int(rowp1[-1]))
    ng = n0 + 300
    xt, q, a0 = rng.uniform(0.2, 0.8, size=ng), rng.uniform(1.0, 4.0, size=ng), rng.uniform(0.5, 1.0, size=ng)
    xf = rng.uniform(0.3, 0.6, size=ng)
    if rank is None:
        n, rowp = ng, np.concatenate([rowp0, rowp0[-1] + rowp1[1:]]).astype(np.intc)
        cols, data, lo = np.concatenate([cols0, cols1 + n0]).astype(np.intc), np.concatenate([data0, data1]), 0
    elif rank == 0:
        n, rowp, cols, data, lo = n0, rowp0, cols0, data0, 0
    else:
        n, rowp, cols, data, lo = 300, rowp1, cols1, data1, n0
    A = dense_jacobian(n, rowp, cols, data)
    xt, q, a0, xf = (v[lo:lo + n] for v in (xt, q, a0, xf))
    b = A @ xf + 0.05
    a0sum = 0.45 * float(reduce(np.array([np.sum(a0)]))[0])

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=len(rowp) - 1, nwinequality=len(rowp) - 1, rowp=rowp, cols=cols,
                             dense_column_rows=100)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = b - A @ x
            f, ax = reduce(np.array([np.sum(q * (x - xt) ** 2), a0 @ x]))
            return 0, float(f), np.array([a0sum - ax])

        def evalSparseObjConGradient(self, x, g, Ac, d):
            g[:] = 2.0 * q * (x - xt)
            Ac[0][:] = -a0
            d[:] = -data
            return 0

    return _P()


def _shard_run(ctx, prob):
    import paropt_amd as pa

    ip = pa.InteriorPoint(prob, dict(IP_OPTS, abs_res_tol=1e-8, max_major_iters=25, write_output_frequency=0))
    ip.optimize()
    return ip.getIterationCounters(), ip.getObjective()[0], ip.getOptimizedPoint()[0].to_numpy()


def _worker(rank, world, port, q):
    import os

    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()

    def reduce(v):
        t = torch.from_numpy(np.array(v, dtype=np.float64))
        dist.all_reduce(t)
        return t.numpy()

    prob = _shard_problem(ctx, rank, world, reduce)
    dense = prob.dense_columns
    counters, f, x = _shard_run(ctx, prob)
    got = [None] * world
    dist.all_gather_object(got, (rank, dense, counters, f, x))
    if rank == 0:
        q.put(sorted(got, key=lambda t: t[0]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_dense_columns_on_one_rank(ctx):
    """The dense columns are one rank's business: rank 0 solves its sparse constraints by low-rank update, rank 1 has
    nothing to split, no collective is issued by either on that account, and the run matches the same global problem
    on one rank as closely as the other two-rank runs of the suite match theirs (test_gpu_torch_problem)."""
    import torch.multiprocessing as mp

    one = _shard_problem(ctx, None, 1, lambda v: v)
    assert one.dense_columns == [300, 301]
    counters1, f1, x1 = _shard_run(ctx, one)
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    port = _free_port()
    procs = [mpctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    (_, da, ca, fa, xa), (_, db, cb, fb, xb) = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert da == [300, 301] and db == []
    assert ca == cb == counters1
    assert abs(fa - f1) <= 1e-7 * max(1.0, abs(f1)) and fa == fb
    np.testing.assert_allclose(np.concatenate([xa, xb]), x1, rtol=0, atol=1e-7)


def test_minmax_example_on_the_facade():
    """examples/minmax_amd.cpp: ParOptSparseProblem::setDenseColumnThreshold / getDenseColumns on an epigraph problem."""
    import json
    import os
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "examples", "minmax_amd")
    out = subprocess.run([exe, "nvars=120"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["rc"] == 0 and res["ndense"] == 1 and res["dense_column"] == 120
    assert res["factor_info"].endswith(" ndense 1")
    assert 0 < res["niter"] < 200 and abs(res["t"] - res["max_term"]) <= 1e-4 and res["max_term"] > 0.0


def test_column_sum_with_dense_columns(ctx):
    """The column sum (pattern only) is reached the way the suite reaches it: the Hessian of the built-in chain
    constraints, 2 zw_i on the diagonal entries of row i's variables.  r = 9 variables enter every row; the part of
    H px that zw adds is 2 (pattern^T zw) o px, against numpy and against the direct path."""
    import paropt_amd as pa

    n0, r, c = 300, 9, 2
    n, w = n0 + r, n0 - 1
    rng = np.random.default_rng(3)
    z = np.linspace(0.5, 1.5, c)
    zw_h, px_h = rng.uniform(0.1, 2.0, size=w), rng.standard_normal(n)
    got = {}
    for rule in (100, -1):
        prob = pa.SeparableProblem(ctx, "convex", n, c).setChain(2, 1, dense_vars=r, dense_column_rows=rule)
        assert prob.nwcon == w and prob.dense_columns == (list(range(n0, n)) if rule > 0 else [])
        ip = pa.InteriorPoint(prob, {"max_major_iters": 1, "write_output_frequency": 0})
        ip.optimize()
        zw, px = _vec(ctx, zw_h), _vec(ctx, px_h)
        with_zw = ip.evalHvec(z, zw, px, pa.PVec(ctx, n)).to_numpy()
        without = ip.evalHvec(z, _vec(ctx, np.zeros(w)), px, pa.PVec(ctx, n)).to_numpy()
        got[rule] = with_zw - without
    colsum = np.zeros(n)
    colsum[:w] += zw_h
    colsum[1:w + 1] += zw_h
    colsum[n0:] = zw_h.sum()
    ref = 2.0 * colsum * px_h
    scale = np.abs(ref).max()
    np.testing.assert_allclose(got[-1], ref, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(got[100], ref, rtol=0, atol=1e-12 * scale)
