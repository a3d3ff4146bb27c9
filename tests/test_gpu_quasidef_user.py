"""GPU: a problem that brings its own quasi-definite solver (createQuasiDefMat, po_problem_set_quasidef_callbacks).

  * the reference's own CSR trajectories (tests/golden/ipcsr_*.npz were recorded with a user-side DENSE solver handed
    to the reference through createQuasiDefMat) with the same kind of solver attached here, as a numpy object and as
    a torch object on the device, under the very assertions of test_gpu_ip.py::test_ip_trajectory_golden (that test
    function is called with its problem builder extended by the attachment -- nothing is restated);
  * the weighting goldens with a user-side diagonal solver, the nwblock = 3 golden with a user-side 3 x 3 block solver;
  * the same system under the user's and the library's solver; exact call accounting; the two-panel Gram kernel
    against numpy; subproblems (trust region, MMA), two ranks, failures, exceptions, leaks.
"""
import gc
import os
import socket

import numpy as np
import pytest

import test_gpu_csr as TC
import test_gpu_ip as TI
import test_gpu_mma as TM
import test_gpu_tr as TT
from conftest import ip_options_from_case, load_golden
from csr_helpers import dense_jacobian

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


# ---- user-side solvers: S = C + A D^-1 A^T, Cholesky, yw = S^-1 (bw - A D^-1 bx), yx = D^-1 (bx + A^T yw) ----------
class DenseSolver:
    """numpy; the entries come from problem.getSparseJacobianData() at every factor"""

    def __init__(self, problem, jacobian=None):
        self.problem, self.jacobian = problem, jacobian
        self.nfactor = self.napply3 = self.napply4 = 0
        self.cdiag_seen = []

    def _A(self):
        if self.jacobian is not None:
            return self.jacobian
        rowp, cols, data = self.problem.getSparseJacobianData()
        return dense_jacobian(self.problem.nvars, rowp, cols, data)

    def factor(self, x, dinv, cdiag):
        self.nfactor += 1
        self.A, self.d = self._A(), np.array(dinv)
        self.cdiag_seen.append(np.array(cdiag))
        self.L = np.linalg.cholesky(np.diag(np.array(cdiag)) + (self.A * self.d) @ self.A.T)
        return 0

    def apply(self, bx, bw, yx, yw):
        if bw is None:
            self.napply3 += 1
        else:
            self.napply4 += 1
        rhs = (0.0 if bw is None else bw) - self.A @ (self.d * bx)
        y = np.linalg.solve(self.L.T, np.linalg.solve(self.L, rhs))
        yw[:] = y
        yx[:] = self.d * (bx + self.A.T @ y)
        return 0

    def getFactorInfo(self):
        return "user dense %d" % self.A.shape[0]


class TorchDenseSolver:
    """the same on the device: zero-copy tensors, entries from getSparseJacobianData(device=True)"""

    def __init__(self, problem):
        self.problem = problem

    def factor(self, x, dinv, cdiag):
        import torch

        rowp, cols, data = self.problem.getSparseJacobianData(device=True)
        w, n = len(rowp) - 1, dinv.numel()
        rows = torch.as_tensor(np.repeat(np.arange(w), np.diff(rowp)), device=data.device, dtype=torch.long)
        A = torch.zeros((w, n), dtype=torch.float64, device=data.device)
        A[rows, torch.as_tensor(cols.astype(np.int64), device=data.device)] = data
        self.A, self.d = A, dinv
        self.L = torch.linalg.cholesky(torch.diag(cdiag) + (A * dinv) @ A.T)
        return 0

    def apply(self, bx, bw, yx, yw):
        import torch

        rhs = -(self.A @ (self.d * bx))
        if bw is not None:
            rhs = rhs + bw
        y = torch.cholesky_solve(rhs[:, None], self.L)[:, 0]
        yw.copy_(y)
        yx.copy_(self.d * (bx + self.A.T @ y))
        return 0


def weighting_jacobian(a):
    """cw_i = 1 - sum_{k < nw} x[nwstart + i (nw + nwskip) + k]: entries -1"""
    A = np.zeros((a["nwcon"], a["n"]))
    for i in range(a["nwcon"]):
        j0 = a.get("nwstart", 0) + i * (a["nw"] + a.get("nwskip", 0))
        A[i, j0:j0 + a["nw"]] = -1.0
    return A


class DiagonalSolver:
    """weighting constraints on disjoint groups: S is diagonal"""

    def __init__(self, A):
        self.A = A
        assert np.count_nonzero(A @ A.T - np.diag(np.diag(A @ A.T))) == 0

    def factor(self, x, dinv, cdiag):
        self.d = np.array(dinv)
        self.s = np.array(cdiag) + (self.A * self.A) @ self.d
        return 0

    def apply(self, bx, bw, yx, yw):
        y = ((0.0 if bw is None else bw) - self.A @ (self.d * bx)) / self.s
        yw[:] = y
        yx[:] = self.d * (bx + self.A.T @ y)
        return 0


class BlockSolver(DiagonalSolver):
    """blocks of B consecutive constraints share variables inside a block only"""

    def __init__(self, A, B):
        self.A, self.B = A, B

    def factor(self, x, dinv, cdiag):
        self.d = np.array(dinv)
        S = np.diag(np.array(cdiag)) + (self.A * self.d) @ self.A.T
        B = self.B
        self.blocks = [np.linalg.cholesky(S[i:i + B, i:i + B]) for i in range(0, S.shape[0], B)]
        return 0

    def apply(self, bx, bw, yx, yw):
        rhs = (0.0 if bw is None else bw) - self.A @ (self.d * bx)
        y = np.concatenate([np.linalg.solve(L.T, np.linalg.solve(L, rhs[i * self.B:(i + 1) * self.B]))
                            for i, L in enumerate(self.blocks)])
        yw[:] = y
        yx[:] = self.d * (bx + self.A.T @ y)
        return 0


def attaching(monkeypatch, cls_name, make_solver, device=False):
    """paropt_amd.<cls_name> (InteriorPoint / TrustRegion / MMA) attaches make_solver(problem) to its problem first: the
    existing runners (run_gpu, run_gpu_tr, run_gpu_mma) then build the problem exactly as they do and solve it with
    the user's solver."""
    import paropt_amd as pa

    base = getattr(pa, cls_name)
    made = []

    class Attaching(base):
        def __init__(self, problem, options=None):
            solver = make_solver(problem)
            made.append(solver)
            problem.setQuasiDefMat(solver, device=device)
            super().__init__(problem, options)

    monkeypatch.setattr(pa, cls_name, Attaching)
    return made


# ---- 1. the reference's own runs with the reference's kind of solver ------------------------------------------------
CSR_CASES = [n for n in TI.IP_CASES if n.startswith("ipcsr_")]
W_CASES = [n for n in TI.IP_CASES if n.startswith("ipw_")]


def test_case_lists_are_complete():
    assert len(CSR_CASES) >= 9 and len(W_CASES) >= 9


@pytest.mark.parametrize("name", CSR_CASES)
def test_csr_goldens_with_user_dense_solver_numpy(ctx, name, monkeypatch):
    made = attaching(monkeypatch, "InteriorPoint", DenseSolver)
    TI.test_ip_trajectory_golden(ctx, name)
    assert made and made[0].nfactor > 0 and made[0].napply4 > 0


@pytest.mark.parametrize("name", CSR_CASES)
def test_csr_goldens_with_user_dense_solver_torch(ctx, name, monkeypatch):
    made = attaching(monkeypatch, "InteriorPoint", TorchDenseSolver, device=True)
    TI.test_ip_trajectory_golden(ctx, name)
    assert made and hasattr(made[0], "L")


# ---- 2. block problems --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W_CASES)
def test_weighting_goldens_with_user_diagonal_solver(ctx, name, monkeypatch):
    _, case = load_golden(name)
    made = attaching(monkeypatch, "InteriorPoint", lambda p: DiagonalSolver(weighting_jacobian(case["args"])))
    TI.test_ip_trajectory_golden(ctx, name)
    assert made and hasattr(made[0], "s")


def test_nwblock_three_with_user_block_solver():
    """tests/test_gpu_compat.py::test_nwblock_three_matches_reference_golden with a user-side 3 x 3 block solver."""
    from oracle import paropt_oracle as po  # problem data only
    from paropt_amd import ParOpt

    name = "ipw_quadratic_n240_c2_w60_nwblock3"
    g, case = load_golden(name)
    a = case["args"]
    n, w, B, nw = a["n"], a["nwcon"], a["nwblock"], a["nw"]
    data = po.SepProblem(a["problem"], n, a.get("c", 2), nwcon=w, nw=nw, nwstart=a["nwstart"], nwskip=a["nwskip"],
                         nwblock=B)
    nc = data.c
    Aw = data.sparse_jacobian_dense()

    class Blocked(ParOpt.Problem):
        def __init__(self):
            super(Blocked, self).__init__(None, nvars=n, ncon=nc, nwcon=w, nwblock=B)
            self.solver = BlockSolver(Aw, B)  # set AFTER the base constructor: the solver is asked for later

        def createQuasiDefMat(self):
            return self.solver

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = data.vars_and_bounds()

        def evalObjCon(self, x):
            return data.eval_obj_con(np.array(x[:]))

        def evalObjConGradient(self, x, g_, A):
            fail, gg, AA = data.eval_obj_con_gradient(np.array(x[:]))
            g_[:] = gg
            for j in range(nc):
                A[j][:] = AA[j]
            return fail

        def evalSparseCon(self, x, con):
            con[:] = 1.0 + Aw @ np.array(x[:])

        def addSparseJacobian(self, alpha, x, px, con):
            con[:] = np.array(con[:]) + alpha * (Aw @ np.array(px[:]))

        def addSparseJacobianTranspose(self, alpha, x, pz, out):
            out[:] = np.array(out[:]) + alpha * (Aw.T @ np.array(pz[:]))

        def addSparseInnerProduct(self, alpha, x, c, A):
            raise AssertionError("the library's block factor must not run when the problem brings its own solver")

    opts = ip_options_from_case(case)
    opts.pop("write_output_frequency", None)
    blocked = Blocked()
    solver = blocked.solver
    opt = ParOpt.Optimizer(blocked, dict(opts, algorithm="ip", output_file=None))
    opt.optimize()
    x, z, zw, zl, zu = opt.getOptimizedPoint()
    np.testing.assert_array_equal(np.array(opt.ip.getIterationCounters()), g["final/counters"])
    assert abs(opt.ip.getObjective()[0] - g["final/fobj"][0]) <= 1e-6 * abs(g["final/fobj"][0])
    np.testing.assert_allclose(x[:], g["final/x"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(z, g["final/z"], rtol=1e-5, atol=1e-6)
    assert hasattr(solver, "blocks")


# ---- 3. same system, two solvers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.PATTERNS))
def test_quasidef_entry_points_route_to_the_user_solver(ctx, name):
    import paropt_amd as pa

    n, rowp, cols = TC.PATTERNS[name]()
    w = len(rowp) - 1
    rng = np.random.default_rng(5)
    data = rng.uniform(-1.5, 1.5, size=int(rowp[-1]))
    prob = TC.PatternProblem(ctx, n, rowp, cols, data)
    solver = DenseSolver(prob)
    prob.setQuasiDefMat(solver)
    x = TC._vec(ctx, np.full(n, 0.5))
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()  # one gradient evaluation uploads the entries
    A = dense_jacobian(n, rowp, cols, data)
    d = rng.uniform(0.2, 3.0, size=n)
    c = rng.uniform(0.05, 2.0, size=w)
    S = np.diag(c) + (A * d) @ A.T
    dv, cv = TC._vec(ctx, d), TC._vec(ctx, c)
    before = solver.nfactor
    pa.quasidef_factor(prob, x, dv, cv)
    assert solver.nfactor == before + 1
    np.testing.assert_array_equal(solver.cdiag_seen[-1], c)  # the user sees Cdiag itself ...
    np.testing.assert_array_equal(cv.to_numpy(), c)          # ... and it is left alone
    assert pa.quasidef_factor_info(prob) == "user dense %d" % w
    for with_bw in (True, False):
        bx = rng.standard_normal(n)
        bw = rng.standard_normal(w) if with_bw else None
        yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
        pa.quasidef_apply(prob, x, dv, cv, TC._vec(ctx, bx), TC._vec(ctx, bw) if with_bw else None, yx, yw)
        rhs = (bw if with_bw else 0.0) - A @ (d * bx)
        yw_ref = np.linalg.solve(S, rhs) if w else np.zeros(0)
        yx_ref = d * (bx + A.T @ yw_ref)
        scale = max(1.0, np.abs(yw_ref).max() if w else 1.0)
        np.testing.assert_allclose(yw.to_numpy(), yw_ref, rtol=0, atol=1e-10 * scale)
        np.testing.assert_allclose(yx.to_numpy(), yx_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yx_ref).max()))


def _grid_fronts_problem(ctx):
    n, rowp, cols = TC.PATTERNS["grid_fronts"]()
    data = np.random.default_rng(5).uniform(-1.5, 1.5, size=int(rowp[-1]))
    return TC.PatternProblem(ctx, n, rowp, cols, data)


def test_interior_point_same_run_under_both_solvers(ctx):
    import paropt_amd as pa

    runs = []
    for user in (False, True):
        prob = _grid_fronts_problem(ctx)
        if user:
            prob.setQuasiDefMat(DenseSolver(prob))
        ip = pa.InteriorPoint(prob, TC.OPTS)
        ip.optimize()
        x, z = ip.getOptimizedPoint()[:2]
        runs.append((ip.getIterationCounters(), x.to_numpy(), np.array(z), ip.getOptimizedSparse()[0].to_numpy(),
                     ip.getHistory()))
    lib, usr = runs
    assert usr[0] == lib[0]
    np.testing.assert_allclose(usr[1], lib[1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(usr[2], lib[2], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(usr[3], lib[3], rtol=0, atol=1e-8 * max(1.0, np.abs(lib[3]).max()))
    assert "MatInfo: user dense" in usr[4] and "MatInfo: n " in lib[4]


# ---- 4. call accounting ---------------------------------------------------------------------------------------------
def test_call_accounting(ctx):
    """Per major iteration of a monotone-barrier L-BFGS run with one refinement step (the cost model):
    exactly ONE factor, c + k three-argument applies (the solved panel of the Gram correction; k = quasi-Newton
    columns in the panel of that iteration) and TWO four-argument applies (the first bordered solve and its one
    refinement; the panel corrections of both are linear combinations of the solved panel, no user call).  The
    start-up before the first iteration (least-squares multipliers): one factor, c three-argument applies for its
    Gram correction and two more for its two block solves."""
    import paropt_amd as pa

    c = 3
    prob = pa.SeparableProblem(ctx, "convex", 300, c).setChain(3, 2)
    solver = DenseSolver(prob)
    prob.setQuasiDefMat(solver)
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": 5, "barrier_strategy": "monotone",
                                 "starting_point_strategy": "least_squares_multipliers",
                                 "iterative_refinement_steps": 1, "abs_res_tol": 1e-9, "max_major_iters": 14})
    marks = []

    def cb(k):
        marks.append((k, ip.snapshot().get("qn_size", 0), solver.nfactor, solver.napply3, solver.napply4))

    ip.setIterationCallback(cb)
    ip.optimize()
    assert len(marks) >= 10
    print("start-up:", marks[0])
    for a, b in zip(marks[:-1], marks[1:]):
        print("iteration %d: k = %d, factor %d, apply3 %d, apply4 %d" % (a[0], a[1], b[2] - a[2], b[3] - a[3],
                                                                        b[4] - a[4]))
    assert marks[0][2:] == (1, c + 2, 0)
    for a, b in zip(marks[:-1], marks[1:]):
        assert (b[2] - a[2], b[3] - a[3], b[4] - a[4]) == (1, c + a[1], 2), (a, b)


# ---- 5. xgram -------------------------------------------------------------------------------------------------------
XW = [0, 1, 5, 127, 128, 129, 1000, 70001]
XNV = [1, 5, 16, 17, 32, 43, 48, 49, 80, 97]


@pytest.mark.parametrize("w", XW)
def test_xgram_vs_numpy(ctx, w):
    import paropt_amd as pa
    from paropt_amd import lib

    rng = np.random.default_rng(w + 1)
    for nv in (XNV if w <= 1000 else [1, 17, 43, 49, 97]):
        Un, Zn = rng.standard_normal((nv, w)), rng.uniform(-1.0, 3.0, size=(nv, w))
        U = [pa.PVec(ctx, w).from_numpy(Un[j]) for j in range(nv)]
        Z = [pa.PVec(ctx, w).from_numpy(Zn[j]) for j in range(nv)]
        X = pa.xgram(U, Z)
        ref = Un @ Zn.T
        atol = 1e-13 * max(w, 64) * 10
        err = np.abs(X - ref).max() if nv else 0.0
        print("xgram w = %d nv = %d: max error %.3e (bound %.3e)" % (w, nv, err, atol))
        np.testing.assert_allclose(X, ref, rtol=0, atol=atol)
        if w > 0 and nv > 1:
            assert np.abs(X - X.T).max() > 0.0  # asymmetric data, asymmetric result
        np.testing.assert_array_equal(pa.xgram(U, Z), X)  # two calls, equal bits
        if w % 2 == 1:  # the pad element of an odd-length vector
            pad = np.zeros(1)
            for v in U + Z:
                lib.check(lib.lib.po_ctx_memcpy(ctx.handle, pad.ctypes.data, v.device_ptr() + 8 * w, 8, 0))
                assert pad[0] == 0.0
        if w > 0:
            ones = pa.PVec(ctx, w)
            ones.set(1.0)
            np.testing.assert_allclose(pa.xgram(U, U), pa.wgram(ones, U), rtol=0, atol=atol)


# ---- 6. subproblems, ranks, errors ----------------------------------------------------------------------------------
def _rows_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        if len(ra) == 2 and isinstance(ra[1], (list, tuple)):  # (printed columns, info tokens) of a trust-region row
            assert list(ra[1]) == list(rb[1]), (ra[1], rb[1])
            ra, rb = ra[0], rb[0]
        np.testing.assert_allclose(np.asarray(ra, dtype=float), np.asarray(rb, dtype=float), rtol=1e-6, atol=1e-9)


def test_trust_region_carries_the_solver(ctx, monkeypatch):
    _, case = load_golden("tr_csr_convex_n120_c2_chain3s2")
    _, rows_lib, _, final_lib = TT.run_gpu_tr(ctx, case)
    made = attaching(monkeypatch, "TrustRegion", DenseSolver)
    _, rows_usr, _, final_usr = TT.run_gpu_tr(ctx, case)
    assert made[0].nfactor > 0 and made[0].napply3 > 0 and made[0].napply4 > 0
    _rows_equal(rows_usr, rows_lib)
    assert final_usr["iter_count"] == final_lib["iter_count"]
    np.testing.assert_allclose(final_usr["x"], final_lib["x"], rtol=0, atol=1e-7)


def test_mma_carries_the_solver(ctx, monkeypatch):
    _, case = load_golden("mma_csr_convex_n150_c2_chain2s2")
    _, rows_lib, final_lib = TM.run_gpu_mma(ctx, case)
    made = attaching(monkeypatch, "MMA", DenseSolver)
    _, rows_usr, final_usr = TM.run_gpu_mma(ctx, case)
    assert made[0].nfactor > 0 and made[0].napply4 > 0
    assert final_usr["iters"] == final_lib["iters"]
    _rows_equal([r[1] for r in rows_usr], [r[1] for r in rows_lib])
    np.testing.assert_allclose(final_usr["x"], final_lib["x"], rtol=0, atol=1e-7)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, user, only_rank0):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    prob = pa.SeparableProblem(ctx, "convex", 400, 2).setChain(3, 2)  # rank-local chains
    solver = DenseSolver(prob)
    if user and (rank == 0 or not only_rank0):
        prob.setQuasiDefMat(solver)
    opts = {"qn_type": "bfgs", "qn_subspace_size": 5, "abs_res_tol": 1e-8, "barrier_strategy": "monotone",
            "max_major_iters": 25, "write_output_frequency": 0}
    try:
        ip = pa.InteriorPoint(prob, opts)
        ip.optimize()
        out = (tuple(ip.getIterationCounters()), ip.getObjective()[0], ip.getOptimizedPoint()[0].norm(),
               solver.nfactor)
    except ParOptAMDError as e:
        out = ("error", str(e))
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(user, only_rank0=False):
    import torch.multiprocessing as mp

    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    port = _free_port()
    procs = [mpctx.Process(target=_worker, args=(r, 2, port, q, user, only_rank0)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


def test_two_ranks_rank_local_solvers():
    lib = _two_ranks(False)
    usr = _two_ranks(True)
    assert usr[0] == lib[0] and usr[3] > 0 and lib[3] == 0
    assert abs(usr[1] - lib[1]) <= 1e-8 * max(1.0, abs(lib[1]))
    assert abs(usr[2] - lib[2]) <= 1e-8 * lib[2]


def test_two_ranks_must_agree_on_the_solver():
    out = _two_ranks(True, only_rank0=True)
    assert out[0] == "error" and "some ranks only" in out[1]


class FailingFactor(DenseSolver):
    def factor(self, x, dinv, cdiag):
        super().factor(x, dinv, cdiag)
        return 7


def test_failed_factor_is_counted_and_survived(ctx):
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    runs = []
    for cls in (DenseSolver, FailingFactor):
        prob = pa.SeparableProblem(ctx, "convex", 200, 2).setChain(3, 2)
        prob.setQuasiDefMat(cls(prob))
        ip = pa.InteriorPoint(prob, {"max_major_iters": 12, "barrier_strategy": "monotone"})
        ip.optimize()  # survived: the reference ignores the value
        runs.append((ip.getIterationCounters(), ip.getObjective()[0], prob))
    assert runs[0][:2] == runs[1][:2]
    prob = runs[1][2]
    x, d, c = pa.PVec(ctx, prob.nvars), pa.PVec(ctx, prob.nvars), pa.PVec(ctx, prob.nwcon)
    d.set(1.0)
    c.set(1.0)
    with pytest.raises(ParOptAMDError, match="failed factorization \\(7\\)"):  # counted: po_quasidef_factor reports it
        pa.quasidef_factor(prob, x, d, c)
    pa.quasidef_factor(runs[0][2], x, d, c)


class FailingApply(DenseSolver):
    def apply(self, bx, bw, yx, yw):
        super().apply(bx, bw, yx, yw)
        return 3 if self.napply4 >= 4 else 0


def test_failed_apply_ends_optimize_with_the_user_error(ctx):
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    prob = pa.SeparableProblem(ctx, "convex", 200, 2).setChain(3, 2)
    prob.setQuasiDefMat(FailingApply(prob))
    ip = pa.InteriorPoint(prob, {"max_major_iters": 12})
    with pytest.raises(ParOptAMDError) as e:
        ip.optimize()
    assert e.value.code == 6  # PO_ERR_USER, as for every other user callback


class FailingPanelApply(DenseSolver):
    def apply(self, bx, bw, yx, yw):
        super().apply(bx, bw, yx, yw)
        return 5 if (bw is None and self.nfactor >= 3) else 0


def test_failed_three_argument_apply_sets_the_message(ctx):
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    prob = pa.SeparableProblem(ctx, "convex", 200, 2).setChain(3, 2)
    prob.setQuasiDefMat(FailingPanelApply(prob))
    ip = pa.InteriorPoint(prob, {"max_major_iters": 12})
    with pytest.raises(ParOptAMDError, match="failed in apply \\(5\\)") as e:
        ip.optimize()
    assert e.value.code == 6


class Boom(RuntimeError):
    pass


class RaisingApply(DenseSolver):
    def apply(self, bx, bw, yx, yw):
        if self.napply4 >= 3:
            raise Boom("inside apply")
        return super().apply(bx, bw, yx, yw)


def test_python_exception_propagates(ctx):
    import paropt_amd as pa

    prob = pa.SeparableProblem(ctx, "convex", 200, 2).setChain(3, 2)
    prob.setQuasiDefMat(RaisingApply(prob))
    ip = pa.InteriorPoint(prob, {"max_major_iters": 12})
    with pytest.raises(Boom, match="inside apply"):
        ip.optimize()


def test_no_live_vectors_after_teardown(ctx):
    import paropt_amd as pa

    def scenario():
        prob = pa.SeparableProblem(ctx, "convex", 300, 2).setChain(3, 2)
        prob.setQuasiDefMat(DenseSolver(prob))
        ip = pa.InteriorPoint(prob, {"max_major_iters": 8})
        ip.optimize()
        ip.getOptimizedSparse()
        U = [pa.PVec(ctx, 500).fill_hash(0, j, 0, 1.0, 0.0) for j in range(7)]
        pa.xgram(U, U[::-1])

    scenario()  # (first use: lazily created context buffers)
    gc.collect()
    before, mirrors = pa.live_objects(), pa.live_host_mirrors()
    scenario()
    gc.collect()
    assert pa.live_objects() == before and pa.live_host_mirrors() == mirrors
