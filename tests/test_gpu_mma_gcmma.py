"""
GPU: the globally convergent MMA (mma_globalization = "conservative") on the dual sub-solver.

  1. the kernels of the rho form (po_mma_dual_eval_rho, po_mma_gcmma_point) against numpy sums in extended precision,
     and bit for bit against the plain form at rho = 0;
  2. whole iterations in lockstep with the numpy restatement (tests/mma_gcmma_helpers.py);
  3. the property the variant exists for: a monotone, feasible sequence that meets the stop test where plain MMA
     oscillates;
  4. conservativeness at acceptance, recomputed outside the library;
  5. the interfaces: refused combinations, the registry, the ParOpt.Optimizer facade, leaks, two ranks.
"""
import gc
import os

import numpy as np
import pytest

from conftest import load_golden
from mma_dual_helpers import Subproblem
from mma_gcmma_helpers import (GCMMA_DEFAULTS, dfun, dprime, fvals, oracle_gcmma, point_rho, primal_point_rho)
from mma_helpers import mma_options_from_case
from mma_test_util import accurate_sum, run_two_ranks
from test_gpu_mma_dual import draw_subproblem, make_problem

pytestmark = pytest.mark.gpu

M_F = 8
EPS = np.finfo(np.float64).eps
LOCKSTEP = "mma_rosenbrock_n60"
LOCKSTEP_ITERS = 8
LOCKSTEP_RAISES = [0, 0, 0, 0, 0, 0, 2, 2]


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


# ---- 1. kernels against numpy ---------------------------------------------------------------------------------------
def draw_rho_subproblem(n, m, seed):
    """The draw of test_gpu_mma_dual.py, and from a generator of its own xk in [alpha, beta] and rho in [0, 1]."""
    sp, lam = draw_subproblem(n, m, seed)
    rng = np.random.default_rng(seed + 7919)
    xk = sp.alpha + rng.random(n) * (sp.beta - sp.alpha)
    rho = rng.random(m + 1)
    return sp, lam, xk, rho


def reference(sp, lam, xk, rho, x_at=None):
    """Every sum of the rho form with its largest term: the terms in double precision, the sums in extended.

    x_at: the point the terms are taken at; None, the default and the reference of every shape with n >= 511: numpy's
    own primal point, independent of the library.  Only the shapes n = 1 and n = 2 pass the point the device reports:
    d(x) = sum (x - xk)^2 u l and the Delta_i are differences around xk, so one ulp of x moves a term by
    ulp(x) / |x - xk| of itself, 1e-14 to 1e-12 here (sigma = rho_0 + lambda . rho pulls x towards xk), and with one
    or two terms that is more than the whole bound 1e-13 n (largest term), which is a summation bound.  Measured
    against numpy's own point on the device: |dD| / bound = 3.2 (n = 1, m = 3), 2.3 (1, 8), 27 (2, 33), exactly where
    x differs from numpy's by one ulp (moving numpy's x by one ulp on the CPU gives 3.2, 2.3, 6.1); every n >= 511
    stays below 2e-2 of the bound.  At n = 1, 2 the point is held to its own 4-ulp bound against numpy and the sums
    are checked at that point, with the same bound."""
    m = sp.m
    P0, Q0, P, Q, xs, x, free = primal_point_rho(sp, xk, rho, lam)
    near = (np.abs(xs - sp.alpha) <= 4 * EPS * np.abs(sp.alpha)) | (np.abs(xs - sp.beta) <= 4 * EPS * np.abs(sp.beta))
    if x_at is not None:
        x = x_at
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    dterms = dfun(sp, xk, x)
    wterms = P0 * u + Q0 * l + sigma * dterms
    gterms = sp.p * u + sp.q * l + np.outer(rho[1:], dterms)
    G = (sp.p * u**2 - sp.q * l**2 + np.outer(rho[1:], dprime(sp, xk, x)))[:, free]
    h = (2.0 * (P * u**3 + Q * l**3))[free]
    ref = dict(near=int(near.sum()), W=float(accurate_sum(wterms)) + float(np.dot(lam, sp.b)),
               Wmax=float(np.abs(wterms).max()), g=accurate_sum(gterms) + sp.b, gmax=np.abs(gterms).max(axis=1),
               D=float(accurate_sum(dterms)), Dmax=float(dterms.max()))
    H, Hmax = np.zeros((m, m)), np.zeros((m, m))
    for k in range(m):
        t = G[: k + 1] * (G[k] / h)
        H[k, : k + 1] = H[: k + 1, k] = accurate_sum(t) if t.shape[1] else 0.0
        Hmax[k, : k + 1] = Hmax[: k + 1, k] = np.abs(t).max(axis=1) if t.shape[1] else 0.0
    ref["H"], ref["Hmax"] = H, Hmax
    uk, lk = 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
    du, dl = (x - xk) * u * uk, -(x - xk) * l * lk
    pterms = np.vstack([sp.p0 * du + sp.q0 * dl, sp.p * du + sp.q * dl, dterms])
    ref["sums"], ref["sumsmax"] = accurate_sum(pterms), np.abs(pterms).max(axis=1)
    ref["point"] = point_rho(sp, xk, rho, lam)[:3]
    return ref


def upload(ctx, sp, xk):
    import paropt_amd as pa

    up = lambda a: pa.PVec(ctx, sp.n).from_numpy(a)  # noqa: E731
    return dict(L=up(sp.L), U=up(sp.U), alpha=up(sp.alpha), beta=up(sp.beta), p0=up(sp.p0), q0=up(sp.q0),
                p=[up(sp.p[i]) for i in range(sp.m)], q=[up(sp.q[i]) for i in range(sp.m)], xk=up(xk))


def eval_rho(ctx, dev, sp, lam, rho, form):
    import paropt_amd as pa

    return pa.mma_dual_eval(ctx, dev["L"], dev["U"], dev["alpha"], dev["beta"], dev["p0"], dev["q0"], dev["p"],
                            dev["q"], sp.b, lam, form=form, xk=dev["xk"], rho=rho)


def eval_plain(ctx, dev, sp, lam, form):
    import paropt_amd as pa

    return pa.mma_dual_eval(ctx, dev["L"], dev["U"], dev["alpha"], dev["beta"], dev["p0"], dev["q0"], dev["p"],
                            dev["q"], sp.b, lam, form=form)


SHAPES = [(n, m) for m in (1, 3, M_F, M_F + 1, 33) for n in (1, 2, 511, 513, 4097)] + [(393217, 8)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_rho_kernels_against_numpy(ctx, n, m):
    import paropt_amd as pa

    sp, lam, xk, rho = draw_rho_subproblem(n, m, seed=1000 * m + n % 997)
    own = reference(sp, lam, xk, rho)  # at numpy's own point: the point itself, and figures to print
    assert own["near"] == 0, "the draw has an element within 4 ulp of a move limit"
    dev = upload(ctx, sp, xk)
    # the point pass: x, zl, zu against numpy
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    sums = pa.mma_gcmma_point(ctx, dev["L"], dev["U"], dev["alpha"], dev["beta"], dev["p0"], dev["q0"], dev["p"],
                              dev["q"], lam, dev["xk"], rho, pt)
    bound = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
    got_pt = [v.to_numpy() for v in pt]
    for name, got, want in zip(("x", "zl", "zu"), got_pt, own["point"]):
        err = np.abs(got - want)
        print("   %s: max err / (4 ulp of max(|L|, |U|)) = %.3f" % (name, (err / bound).max()))
        assert np.all(err <= bound), name
    assert np.all(sp.alpha <= got_pt[0]) and np.all(got_pt[0] <= sp.beta)
    # the reference of the sums: numpy's own point; at n = 1, 2 the point just checked (see reference())
    ref = own if n >= 511 else reference(sp, lam, xk, rho, x_at=got_pt[0])
    errs = np.abs(sums - ref["sums"])
    print("   point sums: max err / bound %.2e (at numpy's own point %.2e)" % (
        (errs / np.maximum(1e-13 * n * ref["sumsmax"], 1e-300)).max(),
        (np.abs(sums - own["sums"]) / np.maximum(1e-13 * n * own["sumsmax"], 1e-300)).max()))
    assert np.all(errs <= 1e-13 * n * ref["sumsmax"])
    forms = [1, 2] if m <= M_F else [2]
    res = {}
    for form in forms:
        W, g, H, D = eval_rho(ctx, dev, sp, lam, rho, form)
        res[form] = (W, g, H, D)
        errW, errg, errH, errD = abs(W - ref["W"]), np.abs(g - ref["g"]), np.abs(H - ref["H"]), abs(D - ref["D"])
        print("n=%d m=%d form %d: |dW| %.2e (bound %.2e)  |dD| %.2e (bound %.2e; at numpy's own point %.2e)  "
              "max|dg|/bound %.2e  max|dH|/bound %.2e" % (
                  n, m, form, errW, 1e-13 * n * ref["Wmax"], errD, 1e-13 * n * ref["Dmax"], abs(D - own["D"]),
                  (errg / np.maximum(1e-13 * n * ref["gmax"], 1e-300)).max(),
                  (errH / np.maximum(1e-13 * n * ref["Hmax"], 1e-300)).max()))
        assert errW <= 1e-13 * n * ref["Wmax"]
        assert errD <= 1e-13 * n * ref["Dmax"]
        assert np.all(errg <= 1e-13 * n * ref["gmax"])
        assert np.all(errH <= 1e-13 * n * ref["Hmax"])
        assert np.array_equal(H, H.T)
        assert D == sums[m + 1]  # the same terms in the same order as in the point pass
        # rho = 0: the bits of the plain form
        W0, g0, H0, _ = eval_rho(ctx, dev, sp, lam, np.zeros(m + 1), form)
        Wp, gp, Hp = eval_plain(ctx, dev, sp, lam, form)
        assert W0 == Wp and np.array_equal(g0, gp) and np.array_equal(H0, Hp)
    if len(forms) == 2:  # same pass, same order: the value and the gradient do not depend on the form
        assert res[1][0] == res[2][0] and np.array_equal(res[1][1], res[2][1]) and res[1][3] == res[2][3]


RHO_START_SHAPES = SHAPES + [(513, 20), (4097, 70)]  # (... and the capacities 32 and 96)


@pytest.mark.parametrize("n,m", RHO_START_SHAPES)
def test_rho_start_sums_against_numpy(ctx, n, m):
    """sum |g| (U - L) and sum |A_i| (U - L): odd tails, more than one workgroup, every column capacity."""
    import paropt_amd as pa

    rng = np.random.default_rng(31 * n + m)
    L = -1.0 - rng.random(n)
    U = 1.0 + 3.0 * rng.random(n)
    g = rng.standard_normal(n) * 10.0 ** (3.0 * rng.random(n))
    A = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.5)
    up = lambda a: pa.PVec(ctx, n).from_numpy(a)  # noqa: E731
    got = pa.mma_gcmma_rho_sums(ctx, up(L), up(U), up(g), [up(A[i]) for i in range(m)])
    terms = np.abs(np.vstack([g, A])) * (U - L)
    want, big = accurate_sum(terms), terms.max(axis=1)
    err = np.abs(got - want)
    print("n=%d m=%d: max err / bound %.2e" % (n, m, (err / np.maximum(1e-13 * n * big, 1e-300)).max()))
    assert got.shape == (m + 1,)
    assert np.all(err <= 1e-13 * n * big)


# ---- shared runs ----------------------------------------------------------------------------------------------------
def run_conservative(ctx, name, extra, keep=False):
    """One MMA run through the library: (mma, rows, per-callback records)."""
    import paropt_amd as pa

    _, case = load_golden(name)
    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), mma_subproblem_solver="dual", mma_dual_tol=1e-9,
                                               **extra))
    rows, recs = [], []

    def cb(k):
        rows.append(mma.getLastRow())
        st, gs = mma.getState(), mma.getGlobalizationStats()
        rec = dict(fobj=st["fobj"], cons=st["cons"].copy(), sub_iter=st["subproblem_iter"], inner_last=gs["inner_last"],
                   cap_hits=gs["cap_hits"], rho=gs["rho"].copy())
        if keep:
            # (inside callback k the subproblem, the asymptotes and rho are still those of iteration k - 1, whose
            # solution x is)
            s = mma.getSubproblem()
            lo, up = mma.getAsymptotes()
            rec["sp"] = Subproblem(lo.to_numpy(), up.to_numpy(), s["alpha"].to_numpy(), s["beta"].to_numpy(),
                                   s["p0"].to_numpy(), s["q0"].to_numpy(), [v.to_numpy() for v in s["p"]],
                                   [v.to_numpy() for v in s["q"]], s["b"])
            rec["x"] = mma.getOptimizedPoint()[0].to_numpy()
        recs.append(rec)

    mma.setIterationCallback(cb)
    mma.optimize()
    return mma, rows, recs


@pytest.fixture(scope="module")
def lockstep(ctx):
    """The library's run of the lockstep golden with everything the callbacks downloaded; released before the context
    closes."""
    run = run_conservative(ctx, LOCKSTEP, {"mma_globalization": "conservative", "mma_max_iterations": LOCKSTEP_ITERS},
                           keep=True)
    yield run
    del run
    gc.collect()


# ---- 2. lockstep with the restatement -------------------------------------------------------------------------------
def test_lockstep_with_the_restatement(ctx, lockstep):
    _, case = load_golden(LOCKSTEP)
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    its, omma = oracle_gcmma(case, mopts, {}, 1e-9, 200, LOCKSTEP_ITERS)
    assert [it["raises"] for it in its] == LOCKSTEP_RAISES
    margin = min(it["margin"] for it in its)
    print("smallest distance of a decision of the restatement from its threshold: %.3e" % margin)
    assert margin >= 1e-6
    mma, rows, recs = lockstep
    assert len(rows) == LOCKSTEP_ITERS + 1
    raises = [r["inner_last"] for r in recs[1:]]
    print("raises per iteration:", raises)
    assert raises == LOCKSTEP_RAISES
    for k, (row, t) in enumerate(zip(rows, omma.trace)):
        assert abs(row[0] - t["fobj"]) <= 1e-6 * max(1.0, abs(t["fobj"])), (k, row[0], t["fobj"])
    gs = mma.getGlobalizationStats()
    assert np.all(np.abs(gs["rho"] - its[-1]["rho"]) <= 1e-6 * its[-1]["rho"]), (gs["rho"], its[-1]["rho"])
    assert gs["inner_total"] == sum(LOCKSTEP_RAISES) and gs["inner_max"] == 2 and gs["cap_hits"] == 0


# ---- 3. the property GCMMA exists for -------------------------------------------------------------------------------
def test_monotone_feasible_and_convergent_where_plain_mma_oscillates(ctx):
    import paropt_amd as pa

    _, case = load_golden("mma_quadratic_n200_c2")
    base = {"mma_subproblem_solver": "dual", "mma_dual_tol": 1e-9, "mma_max_iterations": 150}
    out = {}
    for glob in ("conservative", "none"):
        mma = pa.MMA(make_problem(ctx, case), dict(base, mma_globalization=glob))
        rows = []
        mma.setIterationCallback(lambda k: rows.append(mma.getLastRow()))
        mma.optimize()
        out[glob] = (mma, rows)

    def stopped(row):  # the stop test of MMA::optimize (the driver's permuted names: l1, linfty, infeas)
        return row[1] < 1e-5 and (row[2] < 1e-6 or row[4] < 1e-6)

    mma, rows = out["conservative"]
    gs = mma.getGlobalizationStats()
    print("conservative: %d MMA iterations, %s" % (len(rows) - 1, gs))
    assert len(rows) - 1 <= 100 and stopped(rows[-1])
    first = next(k for k, r in enumerate(rows) if r[4] == 0.0)
    rises = [rows[k][0] - rows[k - 1][0] for k in range(first + 1, len(rows))]
    print("first feasible row %d, largest rise %.3e, largest infeas after %.3e" % (
        first, max(rises), max(r[4] for r in rows[first:])))
    for k in range(first + 1, len(rows)):
        assert rows[k][0] <= rows[k - 1][0] + 1e-7 * max(1.0, abs(rows[k][0])), (k, rows[k - 1][0], rows[k][0])
        assert rows[k][4] <= 1e-6, (k, rows[k][4])
    assert gs["cap_hits"] == 0 and gs["inner_max"] <= 8
    # control: plain MMA on the same sub-solver
    mma0, rows0 = out["none"]
    print("none: %d MMA iterations, last linfty-opt %.3e" % (len(rows0) - 1, rows0[-1][2]))
    assert len(rows0) - 1 == 150 and not stopped(rows0[-1])
    assert rows0[-1][2] > 1e-3
    assert mma0.getGlobalizationStats()["inner_total"] == 0


# ---- 4. conservative at acceptance ----------------------------------------------------------------------------------
def test_accepted_points_are_conservative_outside_the_library(ctx, lockstep):
    mma, rows, recs = lockstep
    tol = GCMMA_DEFAULTS["mma_gcmma_tol"]
    checked = 0
    for k in range(1, len(recs)):
        prev, cur = recs[k - 1], recs[k]
        assert cur["cap_hits"] == 0
        sp, xk, x, rho = cur["sp"], prev["x"], cur["x"], cur["rho"]
        assert np.all(sp.alpha <= x) and np.all(x <= sp.beta) and np.all(sp.alpha <= xk) and np.all(xk <= sp.beta)
        u, l, uk, lk = 1.0 / (sp.U - x), 1.0 / (x - sp.L), 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
        D = float(np.sum(dfun(sp, xk, x)))
        fk, fnew = fvals(prev["fobj"], prev["cons"]), fvals(cur["fobj"], cur["cons"])
        approx = np.empty(sp.m + 1)
        approx[0] = fk[0] + np.sum(sp.p0 * (u - uk) + sp.q0 * (l - lk)) + rho[0] * D
        for i in range(sp.m):
            # g~_i(x) = sum p_i u + q_i l + b_i, and b_i was set so that g~_i(xk) = g_i(xk)
            approx[1 + i] = np.sum(sp.p[i] * u + sp.q[i] * l) + sp.b[i] + rho[1 + i] * D
            assert abs(np.sum(sp.p[i] * uk + sp.q[i] * lk) + sp.b[i] - fk[1 + i]) <= 1e-9 * max(1.0, abs(fk[1 + i]))
        slack = 2.0 * tol * np.maximum(1.0, np.abs(fnew))
        print("iteration %d: f - f~ = %s (allowed %s), D = %.3e, rho = %s" % (k - 1, fnew - approx, slack, D, rho))
        assert np.all(fnew <= approx + slack), (k, fnew, approx)
        checked += 1
    assert checked == LOCKSTEP_ITERS


# ---- 5. interfaces --------------------------------------------------------------------------------------------------
def test_refused_combinations_and_registry(ctx):
    import paropt_amd as pa

    class Untouched(pa.Problem):  # nothing may run: every callback raises
        def getVarsAndBounds(self, x, lb, ub):
            raise AssertionError("the refused solver ran")

        evalObjCon = evalObjConGradient = getVarsAndBounds

    cons = {"mma_globalization": "conservative"}
    dual = dict(cons, mma_subproblem_solver="dual")
    sparse = pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)
    cases = [(pa.SeparableProblem(ctx, "convex", 100, 2), cons, "requires mma_subproblem_solver = dual"),
             (pa.SeparableProblem(ctx, "convex", 100, 2), dict(cons, mma_subproblem_solver="interior_point"),
              "requires mma_subproblem_solver = dual"),
             (sparse, dual, "sparse constraints"),
             (Untouched(ctx, 16, 2, ninequality=1), dual, "equality constraint"),
             (pa.SeparableProblem(ctx, "convex", 100, 2), dict(dual, mma_use_constraint_linearization=1),
              "linearised constraints")]
    for prob, opts, sentence in cases:
        gc.collect()
        before = pa.live_objects()[0]
        mma = pa.MMA(prob, opts)
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2 and sentence in str(e.value), str(e.value)
        assert mma.getState()["mma_iter"] == 0
        assert pa.live_objects()[0] == before, "a refused configuration allocated vectors"
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.MMA(pa.SeparableProblem(ctx, "convex", 100, 2), {"mma_globalization": "armijo"})
    assert e.value.code == 5 and "mma_globalization" in str(e.value)
    for bad in ({"mma_gcmma_rho_init": -0.1}, {"mma_gcmma_rho_min": 0.0}, {"mma_gcmma_tol": -1e-7},
                {"mma_gcmma_max_inner": -1}, {"mma_gcmma_max_inner": 1001}, {"mma_gcmma_raise": 1.1}):
        with pytest.raises(pa.ParOptAMDError) as e:
            pa.MMA(pa.SeparableProblem(ctx, "convex", 100, 2), bad)
        assert e.value.code == 5, bad


def test_facade_optimizer_reaches_the_same_last_row(ctx):
    import paropt_amd as pa
    from paropt_amd import ParOpt

    _, case = load_golden(LOCKSTEP)
    opts = {"mma_subproblem_solver": "dual", "mma_dual_tol": 1e-9, "mma_max_iterations": LOCKSTEP_ITERS,
            "mma_globalization": "conservative"}
    mma = pa.MMA(make_problem(ctx, case), opts)
    mma.optimize()
    opt = ParOpt.Optimizer(make_problem(ctx, case), dict(opts, algorithm="mma", output_file=None, mma_output_file=None))
    opt.optimize()
    assert opt.mma.getLastRow() == mma.getLastRow()
    assert np.array_equal(mma.getOptimizedPoint()[0].to_numpy(), np.array(opt.getOptimizedPoint()[0][:]))
    a, b = opt.mma.getGlobalizationStats(), mma.getGlobalizationStats()
    assert a["inner_total"] == b["inner_total"] == sum(LOCKSTEP_RAISES) and np.array_equal(a["rho"], b["rho"])


def test_no_vectors_leak_and_none_are_added(ctx):
    import paropt_amd as pa

    gc.collect()
    start = pa.live_objects()[0]
    n, c = 3000, 9  # (the panel form: m > M_F)
    prob = pa.SeparableProblem(ctx, "convex", n, c)
    base = pa.live_objects()[0]
    counts = {}
    for glob in ("none", "conservative"):
        mma = pa.MMA(prob, {"mma_subproblem_solver": "dual", "mma_globalization": glob, "mma_max_iterations": 3})
        mma.optimize()
        counts[glob] = pa.live_objects()[0] - base
        del mma
        gc.collect()
        assert pa.live_objects()[0] == base
    # the inner iteration works on the vectors the dual path has: the expansion point is x, the trial point the new x
    assert counts["conservative"] == counts["none"] == 17 + 4 * c, counts
    del prob
    gc.collect()
    assert pa.live_objects()[0] == start


def _counts(ctx):
    """Inner counts, cap hits and evaluation counters of the lockstep run, per row."""
    mma, rows, recs = run_conservative(ctx, LOCKSTEP, {"mma_globalization": "conservative",
                                                       "mma_max_iterations": LOCKSTEP_ITERS})
    gs, ds = mma.getGlobalizationStats(), mma.getDualStats()
    return dict(inner=[r["inner_last"] for r in recs], sub_iter=[r["sub_iter"] for r in recs],
                cap_hits=gs["cap_hits"], inner_total=gs["inner_total"], inner_max=gs["inner_max"],
                dual={k: ds[k] for k in ("solves", "iterations", "evaluations", "last_status")},
                fobj=[r[0] for r in rows])


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    got = _counts(ctx)
    both = [None] * world
    dist.all_gather_object(both, got)
    if rank == 0:
        q.put(both)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(ctx):
    one = _counts(ctx)
    both = run_two_ranks(_worker)
    assert both[0] == both[1], "the ranks took different decisions"
    two = both[0]
    print("one rank :", one)
    print("two ranks:", two)
    for key in ("inner", "cap_hits", "inner_total", "inner_max", "sub_iter", "dual"):
        assert two[key] == one[key], key
