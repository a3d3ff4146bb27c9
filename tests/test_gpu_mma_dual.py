"""
GPU: the dual sub-solver of the method of moving asymptotes (mma_subproblem_solver = "dual").

  1. the kernels (po_mma_dual_eval) against numpy sums in extended precision, both forms, every size class;
  2. optimality of the solved subproblems, checked in numpy on the downloaded data;
  3. whole runs against the unchanged interior-point path, measured by that path's own sensitivity to its tolerance;
  4. the interfaces: the ParOpt.Optimizer facade, the refused configurations, the registry, leaks, two ranks;
  5. launches and host syncs of six iterations on the four paths of the sub-solver, against the integers on record.
"""
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from mma_dual_helpers import (DUAL_GOLDENS, PENALTY_GAMMA, Subproblem, dual_eval, dual_point, primal_point,
                              projected_gradient)
from mma_helpers import mma_options_from_case
from mma_test_util import accurate_sum, run_two_ranks

pytestmark = pytest.mark.gpu

M_F = 8  # widest fused form
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


# ---- 1. kernels against numpy ---------------------------------------------------------------------------------------
def draw_subproblem(n, m, seed):
    """Data built like a real subproblem: L < alpha <= x0 <= beta < U, p, q >= 0 with about half the entries exactly
    0, lambda mixing 0, interior values and gamma (= 2 here).  The magnitudes are chosen so that the bound multipliers
    P u^2 - Q l^2 stay below max(|L|, |U|): the issue's element-wise bound is stated in ulps of that."""
    rng = np.random.default_rng(seed)
    x0 = 5.0 + rng.random(n)
    L = x0 - (2.0 + 2.0 * rng.random(n))
    U = x0 + (2.0 + 2.0 * rng.random(n))
    alpha = x0 - (0.2 + 0.4 * rng.random(n)) * (x0 - L)
    beta = x0 + (0.2 + 0.4 * rng.random(n)) * (U - x0)
    p0 = 0.2 * 10.0 ** (-2.0 * rng.random(n))  # (P / Q over four decades: the minimiser lands on either move limit
    q0 = 0.2 * 10.0 ** (-2.0 * rng.random(n))  # or in between)
    p = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    q = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    b = rng.standard_normal(m)
    gamma = 2.0
    lam = gamma * rng.random(m)
    lam[0::3] = 0.0
    lam[1::3] = gamma
    if m == 1:
        lam[0] = 0.7
    return Subproblem(L, U, alpha, beta, p0, q0, p, q, b), lam


_UPLOADS = {}


def uploaded(ctx, n, m, seed):
    """One draw and one upload per shape, shared by the forms and left unchanged."""
    import paropt_amd as pa

    key = (n, m, seed)
    if key not in _UPLOADS:
        _UPLOADS.clear()  # (one shape's vectors at a time)
        sp, lam = draw_subproblem(n, m, seed)
        up = lambda a: pa.PVec(ctx, n).from_numpy(a)  # noqa: E731
        dev = dict(L=up(sp.L), U=up(sp.U), alpha=up(sp.alpha), beta=up(sp.beta), p0=up(sp.p0), q0=up(sp.q0),
                   p=[up(sp.p[i]) for i in range(m)], q=[up(sp.q[i]) for i in range(m)])
        # the numpy side, computed once
        P, Q, xs, x, free = primal_point(sp, lam)
        near = (np.abs(xs - sp.alpha) <= 4 * EPS * np.abs(sp.alpha)) | (np.abs(xs - sp.beta) <= 4 * EPS * np.abs(sp.beta))
        u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
        wterms = P * u + Q * l
        gterms = sp.p * u + sp.q * l
        G = (sp.p * u**2 - sp.q * l**2)[:, free]
        h = (2.0 * (P * u**3 + Q * l**3))[free]
        ref = dict(near=int(near.sum()), nfree=int(free.sum()), nlow=int((x == sp.alpha).sum()),
                   nup=int((x == sp.beta).sum()),
                   W=float(accurate_sum(wterms)) + float(np.dot(lam, sp.b)), Wmax=float(np.abs(wterms).max()),
                   g=accurate_sum(gterms) + sp.b, gmax=np.abs(gterms).max(axis=1))
        H, Hmax = np.zeros((m, m)), np.zeros((m, m))
        for k in range(m):
            t = G[: k + 1] * (G[k] / h)
            H[k, : k + 1] = H[: k + 1, k] = accurate_sum(t) if t.shape[1] else 0.0
            Hmax[k, : k + 1] = Hmax[: k + 1, k] = np.abs(t).max(axis=1) if t.shape[1] else 0.0
        ref["H"], ref["Hmax"] = H, Hmax
        ref["point"] = dual_point(sp, lam)
        _UPLOADS[key] = (sp, lam, dev, ref)
    return _UPLOADS[key]


def run_eval(ctx, n, dev, sp, lam, form, point=False):
    import paropt_amd as pa

    pt = [pa.PVec(ctx, n) for _ in range(3)] if point else None
    W, g, H = pa.mma_dual_eval(ctx, dev["L"], dev["U"], dev["alpha"], dev["beta"], dev["p0"], dev["q0"], dev["p"],
                               dev["q"], sp.b, lam, form=form, point=pt)
    return W, g, H, ([v.to_numpy() for v in pt] if point else None)


@pytest.mark.parametrize("m", [1, 3, M_F, M_F + 1, 33])
@pytest.mark.parametrize("n", [1, 2, 511, 513, 4097, 393217])
def test_dual_kernels_against_numpy(ctx, n, m):
    sp, lam, dev, ref = uploaded(ctx, n, m, seed=1000 * m + n % 997)
    assert ref["near"] == 0, "the draw has an element within 4 ulp of a move limit"
    if n >= 511:  # every branch of the closed form is taken
        assert ref["nfree"] > n // 20 and ref["nlow"] > n // 20 and ref["nup"] > n // 20, ref
    forms = [1, 2] if m <= M_F else [2]
    res = {}
    for form in forms:
        W, g, H, pt = run_eval(ctx, n, dev, sp, lam, form, point=(form == forms[0]))
        res[form] = (W, g, H)
        errW = abs(W - ref["W"])
        errg = np.abs(g - ref["g"])
        errH = np.abs(H - ref["H"])
        print("n=%d m=%d form %d: |dW| %.2e (bound %.2e)  max|dg|/bound %.2e  max|dH|/bound %.2e" % (
            n, m, form, errW, 1e-13 * n * ref["Wmax"], (errg / np.maximum(1e-13 * n * ref["gmax"], 1e-300)).max(),
            (errH / np.maximum(1e-13 * n * ref["Hmax"], 1e-300)).max()))
        assert errW <= 1e-13 * n * ref["Wmax"]
        assert np.all(errg <= 1e-13 * n * ref["gmax"])
        assert np.all(errH <= 1e-13 * n * ref["Hmax"])
        assert np.array_equal(H, H.T)
        if pt is not None:
            bound = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
            for name, got, want in zip(("x", "zl", "zu"), pt, ref["point"]):
                err = np.abs(got - want)
                print("   %s: max err / (4 ulp of max(|L|, |U|)) = %.3f" % (name, (err / bound).max()))
                assert np.all(err <= bound), name
        # the same form again: identical bits
        W2, g2, H2, _ = run_eval(ctx, n, dev, sp, lam, form)
        assert W2 == W and np.array_equal(g2, g) and np.array_equal(H2, H)
    if len(forms) == 2:  # same pass, same order: the value and the gradient do not depend on the form
        assert res[1][0] == res[2][0] and np.array_equal(res[1][1], res[2][1])
        assert np.all(np.abs(res[1][2] - res[2][2]) <= 1e-13 * n * np.linalg.norm(ref["H"]))


def test_fused_form_is_refused_beyond_its_width(ctx):
    import paropt_amd as pa

    n, m = 64, M_F + 1
    sp, lam, dev, ref = uploaded(ctx, n, m, seed=5)
    with pytest.raises(pa.ParOptAMDError) as e:
        run_eval(ctx, n, dev, sp, lam, 1)
    assert e.value.code == 2


# ---- shared runs of the three goldens -------------------------------------------------------------------------------
def make_problem(ctx, case):
    import paropt_amd as pa

    a = case["args"]
    return pa.SeparableProblem(ctx, a["problem"], a["n"], a.get("c", 2), a.get("seed", 0))


def run_mma(ctx, case, extra, snapshots=()):
    """One MMA run: (mma, rows [(sub-iter, fobj)], {callback k: downloaded state})."""
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), **extra))
    rows, snaps = [], {}

    def cb(k):
        rows.append((mma.getState()["subproblem_iter"], mma.getLastRow()[0]))
        if k in snapshots:
            s = mma.getSubproblem()
            lo, up = mma.getAsymptotes()
            x, z, _, zl, zu = mma.getOptimizedPoint()
            snaps[k] = dict(sp=Subproblem(lo.to_numpy(), up.to_numpy(), s["alpha"].to_numpy(), s["beta"].to_numpy(),
                                          s["p0"].to_numpy(), s["q0"].to_numpy(), [v.to_numpy() for v in s["p"]],
                                          [v.to_numpy() for v in s["q"]], s["b"]),
                            x=x.to_numpy(), z=z.copy(), zl=zl.to_numpy(), zu=zu.to_numpy(), stats=mma.getDualStats(),
                            state=mma.getState())

    mma.setIterationCallback(cb)
    mma.optimize()
    return mma, rows, snaps


_RUNS = {}


def dual_run(ctx, name):
    if name not in _RUNS:
        _, case = load_golden(name)
        _RUNS[name] = run_mma(ctx, case, {"mma_subproblem_solver": "dual", "mma_dual_tol": 1e-9}, snapshots=(1, 2, 9))
    return _RUNS[name]


# ---- 2. optimality of the solved subproblems ------------------------------------------------------------------------
@pytest.mark.parametrize("name", DUAL_GOLDENS)
def test_subproblem_optimality_outside_the_library(ctx, name):
    tol = 1e-9
    mma, rows, snaps = dual_run(ctx, name)
    assert sorted(snaps) == [1, 2, 9]
    for k, s in sorted(snaps.items()):
        sp, x, z = s["sp"], s["x"], s["z"]
        assert np.all(sp.L < sp.alpha) and np.all(sp.beta < sp.U)
        assert np.all(sp.alpha <= x) and np.all(x <= sp.beta)
        assert np.all(z >= 0.0) and np.all(z <= PENALTY_GAMMA)
        W, g, H = dual_eval(sp, z)
        pg = np.abs(projected_gradient(z, g, np.full(sp.m, PENALTY_GAMMA))).max()
        P, Q, xs, xc, free = primal_point(sp, z)
        dx = np.abs(x - xc).max()
        u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
        stat = (np.abs(P * u**2 - Q * l**2) / (P * u**2 + Q * l**2))[free]
        print("%s @%d: max|pg| %.2e, |x - closed form| %.2e, %d free, stationarity %.2e, z = %s" % (
            name, k, pg, dx, free.sum(), stat.max() if stat.size else 0.0, z))
        assert pg <= 10 * tol
        assert dx <= 1e-12 * max(1.0, np.abs(xc).max())
        assert np.all(stat <= 1e-9)
        xk, zl, zu = dual_point(sp, z)  # the bound multipliers belong to the same point
        scale = max(1.0, np.abs(zl).max(), np.abs(zu).max())
        assert np.abs(s["zl"] - zl).max() <= 1e-12 * scale and np.abs(s["zu"] - zu).max() <= 1e-12 * scale
        st = s["stats"]
        assert st["evaluations"] == s["state"]["subproblem_iter"] and st["solves"] == k
        assert st["last_status"] == 0 and st["last_pg"] <= tol
        assert st["iterations"] <= st["evaluations"] - st["solves"]
    st = mma.getDualStats()
    assert st["evaluations"] == mma.getState()["subproblem_iter"] == rows[-1][0]


# ---- 3. whole runs against the interior-point path ------------------------------------------------------------------
@pytest.mark.parametrize("name", DUAL_GOLDENS)
def test_whole_runs_against_the_interior_point(ctx, name):
    _, case = load_golden(name)
    _, rows_a, _ = run_mma(ctx, case, {})
    _, rows_b, _ = run_mma(ctx, case, {"abs_res_tol": 1e-9})
    mma_d, rows_d, _ = dual_run(ctx, name)
    ncmp = min(len(rows_a), len(rows_b), len(rows_d))
    assert ncmp >= 15
    fa, fb, fd = (np.array([r[1] for r in rows[:ncmp]]) for rows in (rows_a, rows_b, rows_d))
    scale = np.maximum(1.0, np.abs(fb))
    d_ref = np.maximum.accumulate(np.abs(fa - fb) / scale)
    d_dual = np.abs(fd - fb) / scale
    per_iter_a = rows_a[-1][0] / (len(rows_a) - 1)
    per_iter_d = rows_d[-1][0] / (len(rows_d) - 1)
    record = dict(golden=name, rows=ncmp, d_ref=d_ref.tolist(), d_dual=d_dual.tolist(),
                  worst_ratio=float((d_dual / np.maximum(1e-12, d_ref)).max()),
                  ip_iterations_per_mma_iteration=per_iter_a, dual_evaluations_per_mma_iteration=per_iter_d,
                  dual_stats=mma_d.getDualStats())
    print(json.dumps({k: v for k, v in record.items() if k not in ("d_ref", "d_dual")}))
    out = os.environ.get("PAROPT_AMD_PROFILE_DIR")
    if out:  # the measurement of profiles/r09_mma_dual_parity.json
        path = os.path.join(out, "r09_mma_dual_parity.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[name] = record
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    for k in range(ncmp):
        assert d_dual[k] <= max(1e-12, d_ref[k]), (k, d_dual[k], d_ref[k])
    assert per_iter_d <= per_iter_a, (per_iter_d, per_iter_a)


# ---- 4. interfaces --------------------------------------------------------------------------------------------------
def test_facade_optimizer_reaches_the_same_point(ctx):
    import paropt_amd as pa
    from paropt_amd import ParOpt

    _, case = load_golden(DUAL_GOLDENS[0])
    opts = {"mma_subproblem_solver": "dual", "mma_dual_tol": 1e-9, "mma_max_iterations": 10}
    mma = pa.MMA(make_problem(ctx, case), opts)
    mma.optimize()
    x1 = mma.getOptimizedPoint()[0].to_numpy()
    opt = ParOpt.Optimizer(make_problem(ctx, case), dict(opts, algorithm="mma", output_file=None, mma_output_file=None))
    opt.optimize()
    x2 = np.array(opt.getOptimizedPoint()[0][:])
    assert np.array_equal(x1, x2)
    assert opt.mma.getDualStats()["evaluations"] == mma.getDualStats()["evaluations"] > 0


def test_refused_configurations_and_registry(ctx):
    import paropt_amd as pa

    class Untouched(pa.Problem):  # nothing may run: every callback raises
        def getVarsAndBounds(self, x, lb, ub):
            raise AssertionError("the refused solver ran")

        evalObjCon = evalObjConGradient = getVarsAndBounds

    dual = {"mma_subproblem_solver": "dual"}
    sparse = pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)
    cases = [(sparse, dual, "sparse constraints"),
             (Untouched(ctx, 16, 2, ninequality=1), dual, "equality constraint"),
             (pa.SeparableProblem(ctx, "convex", 100, 2), dict(dual, mma_use_constraint_linearization=1),
              "linearised constraints")]
    for prob, opts, sentence in cases:
        mma = pa.MMA(prob, opts)
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2 and sentence in str(e.value), str(e.value)
        assert mma.getState()["mma_iter"] == 0
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.MMA(pa.SeparableProblem(ctx, "convex", 100, 2), {"mma_subproblem_solver": "newton"})
    assert e.value.code == 5 and "mma_subproblem_solver" in str(e.value)
    for bad in ({"mma_dual_max_iterations": 0}, {"mma_dual_tol": -1.0}):
        with pytest.raises(pa.ParOptAMDError) as e:
            pa.MMA(pa.SeparableProblem(ctx, "convex", 100, 2), bad)
        assert e.value.code == 5


def test_no_vectors_leak_and_no_interior_point_is_allocated(ctx):
    import gc

    import paropt_amd as pa

    _UPLOADS.clear()
    _RUNS.clear()
    gc.collect()
    start = pa.live_objects()[0]
    n, c = 3000, 9  # (the panel form: m > M_F)
    prob = pa.SeparableProblem(ctx, "convex", n, c)
    base = pa.live_objects()[0]
    counts = {}
    for solver in ("interior_point", "dual"):
        mma = pa.MMA(prob, {"mma_subproblem_solver": solver, "mma_max_iterations": 3})
        mma.optimize()
        counts[solver] = pa.live_objects()[0] - base
        if solver == "dual":
            st = mma.getDualStats()
            assert st["solves"] == 3 and st["evaluations"] == mma.getState()["subproblem_iter"]
        del mma
        gc.collect()
        assert pa.live_objects()[0] == base
    # 17 + 3 c vectors of the MMA itself, + c columns of the panel form; the interior point adds its 15 + c and more
    assert counts["dual"] == 17 + 4 * c, counts
    assert counts["interior_point"] >= counts["dual"] - c + 15 + c, counts
    del prob
    gc.collect()
    assert pa.live_objects()[0] == start


def _dual_rows(ctx, case, lams):
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), mma_subproblem_solver="dual", mma_dual_tol=1e-9))
    rows = []

    def cb(k):
        rows.append((mma.getState()["subproblem_iter"], tuple(mma.getLastRow())))
        lams.append(mma.getOptimizedPoint()[1].tobytes())

    mma.setIterationCallback(cb)
    mma.optimize()
    return rows, mma.getDualStats()


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    _, case = load_golden("mma_quadratic_n200_c2")
    lams = []
    rows, stats = _dual_rows(ctx, case, lams)
    both = [None] * world
    dist.all_gather_object(both, lams)
    if rank == 0:
        q.put((rows, stats, both))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(ctx):
    _, case = load_golden("mma_quadratic_n200_c2")
    lams1 = []
    rows1, stats1 = _dual_rows(ctx, case, lams1)
    rows2, stats2, both = run_two_ranks(_worker)
    assert both[0] == both[1], "the multipliers differ between the ranks"
    assert len(rows2) == len(rows1)
    for (s2, r2), (s1, r1) in zip(rows2, rows1):
        assert s2 == s1  # dual-evaluation counts
        for a, b in zip(r2, r1):  # the table rows (another summation order over the shards: not the same bits)
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (r2, r1)
    assert {k: stats2[k] for k in ("solves", "iterations", "evaluations", "last_status")} == \
        {k: stats1[k] for k in ("solves", "iterations", "evaluations", "last_status")}


# ---- 5. launches and host syncs on record ---------------------------------------------------------------------------
# Six MMA iterations at n = 513 on the paths of the dual sub-solver: the plain dual at a fused and at a panel width,
# grouped sparse constraints (128 groups of nw = 4) and linearised constraints.  The integers are what the library
# printed before the host code of the dual passes was folded into one pass driver (profiles/README.md, round 25): a
# refactor of that code leaves them as they are.
_DUAL = {"mma_subproblem_solver": "dual"}
MMA_ON_RECORD = {
    "plain_c3": dict(c=3, opts=_DUAL, weighting=None, launches=297, syncs=109),
    "plain_c9": dict(c=9, opts=_DUAL, weighting=None, launches=507, syncs=214),
    "grouped_nw4": dict(c=3, opts=dict(_DUAL, mma_dual_sparse_constraints="groups"), weighting=(128, 4, 0, 0),
                        launches=623, syncs=204),
    "linearised_c9": dict(c=9, opts=dict(_DUAL, mma_use_constraint_linearization=1,
                                         mma_dual_linearized_constraints="newton"), weighting=None,
                          launches=403, syncs=165),
}


@pytest.mark.parametrize("name", sorted(MMA_ON_RECORD))
def test_launches_and_syncs_of_the_mma_dual_paths_on_record(ctx, name):
    import paropt_amd as pa

    rec = MMA_ON_RECORD[name]
    prob = pa.SeparableProblem(ctx, "convex", 513, rec["c"])
    if rec["weighting"]:
        prob.setWeighting(*rec["weighting"])
    mma = pa.MMA(prob, dict(rec["opts"], mma_max_iterations=6))
    syncs0, launches0 = ctx.counters()
    mma.optimize()
    syncs1, launches1 = ctx.counters()
    counts = (launches1 - launches0, syncs1 - syncs0)
    print(name, "launches, syncs:", counts)
    assert mma.getState()["mma_iter"] == 7 and mma.getDualStats()["solves"] == 6  # (the stop test never fires)
    assert counts == (rec["launches"], rec["syncs"])
