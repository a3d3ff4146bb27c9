"""
GPU: grouped ("weighting") sparse constraints kept in the dual sub-solver of the method of moving asymptotes
(mma_dual_sparse_constraints = "groups").

  1. the kernels (po_mma_dual_group_eval): residuals of the device's own point in extended precision, W / grad / H
     against extended-precision sums at that point, every class of group in every shape;
  2. optimality of the solved subproblems, checked in numpy on the downloaded data;
  3. a whole run against the unchanged interior-point path and the golden table;
  4. the interfaces: a user's CSR problem through ParOpt.Optimizer, refusals, the registry, leaks, two ranks.
"""
import gc
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from mma_dual_group_helpers import (WEIGHTING_GOLDEN, Groups, bound_multipliers, classes, dual_eval_groups, form_pq,
                                    group_solve)
from mma_dual_helpers import PENALTY_GAMMA, Subproblem, projected_gradient
from mma_helpers import mma_options_from_case, parse_mma_table
from mma_test_util import run_two_ranks

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
GROUPS_ON = {"mma_subproblem_solver": "dual", "mma_dual_sparse_constraints": "groups"}


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def _profile(key, record):
    out = os.environ.get("PAROPT_AMD_PROFILE_DIR")
    if out:  # the measurements of profiles/r12_mma_dual_groups_parity.json
        path = os.path.join(out, "r12_mma_dual_groups_parity.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[key] = record
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


# ---- 1. kernels -----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 0, 0), (2, 2, 0, 0), (37, 5, 0, 0), (513, 3, 2, 7), (1301, 20, 0, 0), (4097, 4, 1, 3)]
GAMMA = 2.0
# what a group is drawn to be.  Inequalities: inactive, strict with every element free, strict with elements on their
# move limits, at gamma; equalities in addition strict with a negative multiplier and at -gamma
INEQ_KINDS = ("inactive", "strict_free", "strict_clamped", "at_gamma")
EQ_KINDS = ("strict_free", "strict_clamped", "at_gamma", "strict_negative", "at_minus_gamma")


def draw(n, nw, skip, start, m, seed):
    """A subproblem as tests/test_gpu_mma_dual.py draws it, and groups (a = -1: psi = c - sum x) whose c is placed
    relative to sum alpha, the unconstrained sum and sum beta so that every kind above occurs."""
    rng = np.random.default_rng(seed)
    period = nw + skip
    nwcon = (n - start - nw) // period + 1
    nwineq = (nwcon + 1) // 2
    x0 = 5.0 + rng.random(n)
    half = 2.0 + 2.0 * rng.random(n)
    L, U = x0 - half, x0 + (2.0 + 2.0 * rng.random(n))
    p0 = 0.2 * 10.0 ** (-2.0 * rng.random(n))
    q0 = 0.2 * 10.0 ** (-2.0 * rng.random(n))
    p = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    q = (0.04 / m) * rng.random((m, n)) * (rng.random((m, n)) < 0.5)
    idx = start + np.arange(nwcon)[:, None] * period + np.arange(nw)[None, :]
    kinds = [INEQ_KINDS[i % 4] if i < nwineq else EQ_KINDS[(i - nwineq) % 5] for i in range(nwcon)]
    for i, k in enumerate(kinds):
        if k == "strict_free":  # symmetric asymptotes and P close to Q: the minimiser sits near x0, well inside
            j = idx[i]
            U[j] = x0[j] + half[j]
            q0[j] = p0[j] * (1.0 + 0.05 * rng.random(nw))
            p[:, j] = q[:, j]
    alpha = x0 - (0.2 + 0.4 * rng.random(n)) * (x0 - L)
    beta = x0 + (0.2 + 0.4 * rng.random(n)) * (U - x0)
    b = rng.standard_normal(m)
    lam = GAMMA * rng.random(m)
    lam[0::3] = 0.0
    lam[1::3] = GAMMA
    if m == 1:
        lam[0] = 0.7
    sp = Subproblem(L, U, alpha, beta, p0, q0, p, q, b)
    free = group_solve(sp, lam, Groups(0, 1, 0, 0, -1.0, [], 0))["x"]
    sa, s0, sb = alpha[idx].sum(axis=1), free[idx].sum(axis=1), beta[idx].sum(axis=1)
    c = np.zeros(nwcon)
    for i, k in enumerate(kinds):
        c[i] = {"inactive": s0[i] + 0.1 * nw, "strict_free": s0[i] - 0.02 * nw,
                "strict_clamped": sa[i] + 0.3 * (s0[i] - sa[i]), "at_gamma": sa[i] - 0.1 * nw,
                "strict_negative": s0[i] + 0.3 * (sb[i] - s0[i]), "at_minus_gamma": sb[i] + 0.1 * nw}[k]
    return sp, lam, Groups(nwcon, nw, start, skip, -1.0, c, nwineq, GAMMA)


def found_kinds(sp, gr, x, zw):
    """The kinds the groups of a point (x, zw) actually are."""
    out = set()
    cls = classes(gr, zw)
    for i in range(gr.nwcon):
        j = gr.idx[i]
        allfree = bool(np.all((x[j] > sp.alpha[j]) & (x[j] < sp.beta[j])))
        eq = i >= gr.nwineq
        if cls[i] == 2:
            out.add(("eq_" if eq else "") + "at_gamma")
        elif cls[i] == 0:
            out.add("at_minus_gamma" if eq else "inactive")
        elif zw[i] < 0.0:
            out.add("strict_negative")
        else:
            out.add(("eq_" if eq else "") + ("strict_free" if allfree else "strict_clamped"))
    return out


ALL_KINDS = {"inactive", "strict_free", "strict_clamped", "at_gamma", "eq_strict_free", "eq_strict_clamped",
             "eq_at_gamma", "strict_negative", "at_minus_gamma"}


def residual_ratios(sp, lam, gr, x, zw):
    """The issue's residual bounds at a device point, evaluated in extended precision: the largest ratio residual /
    bound over the free elements, the clamped elements (one-sided), the strict groups and the groups at an end of
    their interval (one-sided)."""
    m = sp.m
    P, Q = sp.p0.astype(LD), sp.q0.astype(LD)
    for i in range(m):
        P = P + LD(lam[i]) * sp.p[i].astype(LD)
        Q = Q + LD(lam[i]) * sp.q[i].astype(LD)
    xl = x.astype(LD)
    u, l = 1 / (sp.U.astype(LD) - xl), 1 / (xl - sp.L.astype(LD))
    t = np.zeros(sp.n, dtype=LD)
    if gr.nwcon:
        t[gr.idx] = (LD(gr.a) * zw.astype(LD))[:, None]
    res = P * u * u - Q * l * l - t
    h = 2 * (P * u**3 + Q * l**3)
    sp_lu = np.spacing(np.maximum(np.abs(sp.L), np.abs(sp.U))).astype(LD)
    bound = 4 * h * sp_lu + 16 * (m + 2) * LD(EPS) * (P * u * u + Q * l * l)
    free = (x > sp.alpha) & (x < sp.beta)
    lowc, upc = x == sp.alpha, x == sp.beta
    out = dict(free=float((np.abs(res) / bound)[free].max(initial=0.0)),
               clamped=float(max((-res / bound)[lowc].max(initial=0.0), (res / bound)[upc].max(initial=0.0))))
    if gr.nwcon:
        ix = gr.idx
        psi = LD(gr.a) * xl[ix].sum(axis=1) + gr.c.astype(LD)
        sg = np.where(free[ix], 1 / h[ix], 0).sum(axis=1)
        gb = (abs(gr.a) * (4 * sp_lu[ix]).sum(axis=1) + LD(gr.a) ** 2 * sg * 4 * np.spacing(np.abs(zw)).astype(LD)
              + gr.nw * LD(EPS) * (abs(gr.a) * np.abs(xl[ix]).sum(axis=1) + np.abs(gr.c)))
        cls = classes(gr, zw)
        out["strict"] = float((np.abs(psi) / gb)[cls == 1].max(initial=0.0))
        out["ends"] = float(max((-psi / gb)[cls == 0].max(initial=0.0), (psi / gb)[cls == 2].max(initial=0.0)))
    return out


def accurate_sum(terms):
    if np.finfo(LD).eps < 1e-18:
        return np.sum(np.asarray(terms, dtype=LD), axis=-1, dtype=LD).astype(np.float64)
    import math

    t = np.atleast_2d(terms)
    out = np.array([math.fsum(row) for row in t])
    return out if np.ndim(terms) > 1 else out[0]


def sums_at_point(sp, lam, gr, x, zw):
    """W, grad, H at the device's own point, classes from the device's values: (value, largest term) each."""
    P, Q = form_pq(sp, lam)
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    wterms = P * u + Q * l
    gterms = sp.p * u + sp.q * l
    free = (x > sp.alpha) & (x < sp.beta)
    d = np.where(free, 1.0 / (2.0 * (P * u**3 + Q * l**3)), 0.0)
    G = sp.p * u**2 - sp.q * l**2
    m = sp.m
    zterms = np.zeros(1)
    if gr.nwcon:
        psi = (LD(gr.a) * x[gr.idx].astype(LD).sum(axis=1) + gr.c.astype(LD)).astype(np.float64)
        zterms = zw * psi
    W = float(accurate_sum(wterms)) - float(accurate_sum(zterms)) + float(np.dot(lam, sp.b))
    Wmax = max(float(np.abs(wterms).max()), float(np.abs(zterms).max()))
    g, gmax = accurate_sum(gterms) + sp.b, np.abs(gterms).max(axis=1)
    H, Hmax = np.zeros((m, m)), np.zeros((m, m))
    if gr.nwcon:
        Gd = (G * d).astype(LD)
        ag = Gd[:, gr.idx].sum(axis=2)
        sg = d.astype(LD)[gr.idx].sum(axis=1)
        wgt = np.where((classes(gr, zw) == 1) & (sg > 0), 1 / np.where(sg > 0, sg, 1), 0)
    for k in range(m):
        t1 = G[: k + 1] * (G[k] * d)
        H[k, : k + 1] = accurate_sum(t1)
        Hmax[k, : k + 1] = np.abs(t1).max(axis=1)
        if gr.nwcon:
            t2 = (ag[: k + 1] * (ag[k] * wgt)).astype(np.float64)
            H[k, : k + 1] -= accurate_sum(t2)
            Hmax[k, : k + 1] = np.maximum(Hmax[k, : k + 1], np.abs(t2).max(axis=1))
        H[: k + 1, k], Hmax[: k + 1, k] = H[k, : k + 1], Hmax[k, : k + 1]
    return W, Wmax, g, gmax, H, Hmax


def device_eval(ctx, sp, lam, gr):
    import paropt_amd as pa

    n, m = sp.n, sp.m
    up = lambda a, k=n: pa.PVec(ctx, k).from_numpy(a)  # noqa: E731
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    zw = pa.PVec(ctx, gr.nwcon) if gr.nwcon else None
    W, g, H, st = pa.mma_dual_group_eval(
        ctx, up(sp.L), up(sp.U), up(sp.alpha), up(sp.beta), up(sp.p0), up(sp.q0), [up(sp.p[i]) for i in range(m)],
        [up(sp.q[i]) for i in range(m)], sp.b, lam, gr.nwcon, gr.nw, gr.start, gr.skip, gr.a,
        up(gr.c, gr.nwcon) if gr.nwcon else None, gr.nwineq, gr.gamma, pt, zw)
    x, zl, zu = (v.to_numpy() for v in pt)
    return W, g, H, st, x, zl, zu, (zw.to_numpy() if gr.nwcon else np.zeros(0))


@pytest.mark.parametrize("m", [1, 3, 8, 9, 33])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_nw%d_skip%d_start%d" % s)
def test_group_kernels(ctx, shape, m):
    n, nw, skip, start = shape
    sp, lam, gr = draw(n, nw, skip, start, m, seed=100 * m + n % 97)
    ref = group_solve(sp, lam, gr)  # the restatement alone: every kind of group is in the draw
    kinds = found_kinds(sp, gr, ref["x"], ref["zw"])
    assert ref["cap"] == 0
    if gr.nwcon >= 8:
        assert kinds == ALL_KINDS, sorted(ALL_KINDS - kinds)
    W, g, H, st, x, zl, zu, zw = device_eval(ctx, sp, lam, gr)
    # exact: the point lies inside its boxes
    assert np.all(x >= sp.alpha) and np.all(x <= sp.beta)
    assert np.all(zw >= gr.zlo) and np.all(zw <= gr.gamma)
    assert st["cap_hits"] == 0 and st["strict"] + st["at_lower"] + st["at_gamma"] == gr.nwcon
    cls = classes(gr, zw)
    assert (st["strict"], st["at_lower"], st["at_gamma"]) == tuple(int((cls == k).sum()) for k in (1, 0, 2))
    if gr.nwcon >= 8:
        assert found_kinds(sp, gr, x, zw) == ALL_KINDS
    ratios = residual_ratios(sp, lam, gr, x, zw)
    Wr, Wmax, gr_, gmax, Hr, Hmax = sums_at_point(sp, lam, gr, x, zw)
    rW = abs(W - Wr) / (1e-13 * n * Wmax)
    rg = float((np.abs(g - gr_) / np.maximum(1e-13 * n * gmax, 1e-300)).max())
    rH = float((np.abs(H - Hr) / np.maximum(1e-13 * n * Hmax, 1e-300)).max())
    zlr, zur = bound_multipliers(sp, gr, dict(P=form_pq(sp, lam)[0], Q=form_pq(sp, lam)[1], x=x, zw=zw))
    zb = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
    rz = float(max((np.abs(zl - zlr) / zb).max(), (np.abs(zu - zur) / zb).max()))
    record = dict(ratios, W=rW, grad=rg, hess=rH, zl_zu=rz, max_inner=st["max_inner"],
                  mean_inner=st["steps"] / max(1, gr.nwcon), groups=gr.nwcon)
    print("n=%d nw=%d skip=%d start=%d m=%d: %s" % (n, nw, skip, start, m, json.dumps(record)))
    _profile("kernels n%d_nw%d_skip%d_start%d m%d" % (n, nw, skip, start, m), record)
    for key in ("free", "clamped", "strict", "ends"):
        assert ratios.get(key, 0.0) <= 1.0, (key, ratios)
    assert rW <= 1.0 and rg <= 1.0 and rH <= 1.0, (rW, rg, rH)
    assert np.array_equal(H, H.T)
    assert rz <= 1.0
    assert abs(st["zw_psi"]) <= 1e300 and st["max_psi"] >= 0.0


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "n%d_nw%d_skip%d_start%d" % s)
def test_without_active_groups_it_is_the_plain_dual(ctx, shape):
    import paropt_amd as pa

    n, nw, skip, start = shape
    m = 3
    sp, lam, gr = draw(n, nw, skip, start, m, seed=7)
    up = lambda a: pa.PVec(ctx, n).from_numpy(a)  # noqa: E731
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    W0, g0, H0 = pa.mma_dual_eval(ctx, up(sp.L), up(sp.U), up(sp.alpha), up(sp.beta), up(sp.p0), up(sp.q0),
                                  [up(sp.p[i]) for i in range(m)], [up(sp.q[i]) for i in range(m)], sp.b, lam,
                                  form=2, point=pt)
    x0, zl0, zu0 = (v.to_numpy() for v in pt)
    Wr, Wmax, gr_, gmax, Hr, Hmax = sums_at_point(sp, lam, Groups(0, 1, 0, 0, -1.0, [], 0), x0, np.zeros(0))
    inactive = Groups(gr.nwcon, nw, start, skip, -1.0, sp.beta[gr.idx].sum(axis=1) + 1.0, gr.nwcon, GAMMA)
    for g_ in (Groups(0, 1, 0, 0, -1.0, [], 0, GAMMA), inactive):
        W, g, H, st, x, zl, zu, zw = device_eval(ctx, sp, lam, g_)
        assert np.all(zw == 0.0) and st["strict"] == st["at_gamma"] == 0 and st["at_lower"] == g_.nwcon
        assert abs(W - W0) <= 1e-13 * n * Wmax and np.all(np.abs(g - g0) <= 1e-13 * n * gmax)
        assert np.all(np.abs(H - H0) <= 1e-13 * n * Hmax)
        zb = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
        assert np.all(np.abs(x - x0) <= zb) and np.all(np.abs(zl - zl0) <= zb) and np.all(np.abs(zu - zu0) <= zb)


def test_group_eval_argument_checks(ctx):
    import paropt_amd as pa

    sp, lam, gr = draw(37, 5, 0, 0, 1, seed=1)
    for bad in (dict(nw=600), dict(start=10), dict(gamma=0.0)):
        g_ = Groups(gr.nwcon, bad.get("nw", gr.nw), bad.get("start", 0), 0, -1.0,
                    np.zeros(gr.nwcon), gr.nwineq, bad.get("gamma", GAMMA))
        g_.idx = gr.idx
        with pytest.raises(pa.ParOptAMDError) as e:
            device_eval(ctx, sp, lam, g_)
        assert e.value.code == 2, bad


# ---- shared runs of the weighting golden ----------------------------------------------------------------------------
def make_problem(ctx, case):
    import paropt_amd as pa

    a = case["args"]
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a.get("c", 2), a.get("seed", 0))
    return prob.setWeighting(a["nwcon"], a["nw"], a.get("nwstart", 0), a.get("nwskip", 0))


def golden_groups(case):
    a = case["args"]  # cw_i = 1 - sum x: linear, so psi is the constraint itself
    return Groups(a["nwcon"], a["nw"], a.get("nwstart", 0), a.get("nwskip", 0), -1.0, np.ones(a["nwcon"]), a["nwcon"])


def run_mma(ctx, case, extra, snapshots=()):
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), **extra))
    rows, snaps = [], {}

    def cb(k):
        rows.append((mma.getState()["subproblem_iter"], mma.getLastRow()[0]))
        if k in snapshots:
            s = mma.getSubproblem()
            lo, up = mma.getAsymptotes()
            x, z, zw, zl, zu = mma.getOptimizedPoint()
            snaps[k] = dict(sp=Subproblem(lo.to_numpy(), up.to_numpy(), s["alpha"].to_numpy(), s["beta"].to_numpy(),
                                          s["p0"].to_numpy(), s["q0"].to_numpy(), [v.to_numpy() for v in s["p"]],
                                          [v.to_numpy() for v in s["q"]], s["b"]),
                            x=x.to_numpy(), z=z.copy(), zw=zw.to_numpy(), zl=zl.to_numpy(), zu=zu.to_numpy(),
                            stats=mma.getDualStats(), gstats=mma.getDualGroupStats(), state=mma.getState())

    mma.setIterationCallback(cb)
    mma.optimize()
    return mma, rows, snaps


_RUNS = {}


def groups_run(ctx):
    if "d" not in _RUNS:
        _, case = load_golden(WEIGHTING_GOLDEN)
        _RUNS["d"] = run_mma(ctx, case, dict(GROUPS_ON, mma_dual_tol=1e-9), snapshots=(1, 2, 9))
    return _RUNS["d"]


# ---- 2. optimality of the solved subproblems ------------------------------------------------------------------------
def test_subproblem_optimality_outside_the_library(ctx):
    tol = 1e-9
    _, case = load_golden(WEIGHTING_GOLDEN)
    gr = golden_groups(case)
    mma, rows, snaps = groups_run(ctx)
    assert sorted(snaps) == [1, 2, 9]
    for k, s in sorted(snaps.items()):
        sp, x, z, zw = s["sp"], s["x"], s["z"], s["zw"]
        assert np.all(sp.alpha <= x) and np.all(x <= sp.beta)
        assert np.all(z >= 0.0) and np.all(z <= PENALTY_GAMMA)
        assert np.all(zw >= 0.0) and np.all(zw <= PENALTY_GAMMA)
        W, g, H, pt = dual_eval_groups(sp, z, gr)
        pg = np.abs(projected_gradient(z, g, np.full(sp.m, PENALTY_GAMMA))).max()
        ratios = residual_ratios(sp, z, gr, x, zw)
        print("@%d: max|pg| %.2e, ratios %s, group stats %s, z = %s" % (k, pg, ratios, s["gstats"], z))
        assert pg <= 10 * tol
        for key in ("free", "clamped", "strict", "ends"):
            assert ratios[key] <= 1.0, (k, key, ratios)
        assert s["gstats"]["cap_hits"] == 0
        assert s["gstats"]["strict"] + s["gstats"]["at_lower"] + s["gstats"]["at_gamma"] == gr.nwcon
        assert s["stats"]["last_status"] == 0 and s["stats"]["solves"] == k
    assert mma.getDualStats()["evaluations"] == mma.getState()["subproblem_iter"] == rows[-1][0]


# ---- 3. the whole run against the interior point --------------------------------------------------------------------
def test_whole_run_against_the_interior_point(ctx):
    g, case = load_golden(WEIGHTING_GOLDEN)
    _, rows_a, _ = run_mma(ctx, case, {})
    _, rows_b, _ = run_mma(ctx, case, {"abs_res_tol": 1e-9})
    mma_d, rows_d, _ = groups_run(ctx)
    ncmp = min(len(rows_a), len(rows_b), len(rows_d))
    assert ncmp >= 15
    fa, fb, fd = (np.array([r[1] for r in rows[:ncmp]]) for rows in (rows_a, rows_b, rows_d))
    scale = np.maximum(1.0, np.abs(fb))
    d_ref = np.maximum.accumulate(np.abs(fa - fb) / scale)
    d_dual = np.abs(fd - fb) / scale
    per_iter_a = rows_a[-1][0] / (len(rows_a) - 1)
    per_iter_d = rows_d[-1][0] / (len(rows_d) - 1)
    ref = parse_mma_table(g["paropt_mma"])
    d_gold = np.array([abs(fd[k] - ref[k][1][0]) / max(1.0, abs(ref[k][1][0])) for k in range(ncmp)])
    record = dict(golden=WEIGHTING_GOLDEN, rows=ncmp, d_ref=d_ref.tolist(), d_dual=d_dual.tolist(),
                  d_golden_table=d_gold.tolist(), worst_ratio=float((d_dual / np.maximum(1e-12, d_ref)).max()),
                  ip_iterations_per_mma_iteration=per_iter_a, dual_evaluations_per_mma_iteration=per_iter_d,
                  dual_stats=mma_d.getDualStats(), group_stats=mma_d.getDualGroupStats())
    print(json.dumps(record))
    _profile("whole_run", record)
    for k in range(ncmp):
        assert d_gold[k] <= 1e-4, (k, d_gold[k])
    for k in range(ncmp):
        assert d_dual[k] <= max(1e-12, d_ref[k]), (k, d_dual[k], d_ref[k])
    assert per_iter_d < per_iter_a, (per_iter_d, per_iter_a)


# ---- 4. interfaces --------------------------------------------------------------------------------------------------
def user_csr_problem(ctx, case):
    """The weighting golden as a user's problem in the CSR form (the form of examples/weighting_amd.cpp): the weighting
    constraints reach the library only as the pattern (rowp, cols) and the entries -1 its gradient callback writes.
    Objective, dense constraints and their gradients are the built-in problem's own evaluations (its kernels, through
    po_problem_eval_*), so that the twins can be compared to the last bit."""
    import ctypes as C

    import paropt_amd as pa
    from paropt_amd import lib as L

    a = case["args"]
    n, c, w, nw = a["n"], a.get("c", 2), a["nwcon"], a["nw"]
    gr = golden_groups(case)
    rowp = (np.arange(w + 1) * nw).astype(np.intc)
    cols = gr.idx.astype(np.intc).ravel()
    dense = pa.SeparableProblem(ctx, a["problem"], n, c, a.get("seed", 0))
    xv, lbv, ubv, gv = (pa.PVec(ctx, n) for _ in range(4))
    Av = [pa.PVec(ctx, n) for _ in range(c)]
    arr = (L.po_vec * c)(*[v.handle for v in Av])

    class P(pa.Problem):
        _keep = (dense, xv, lbv, ubv, gv, Av, arr)

        def getVarsAndBounds(self, x, lb, ub):
            pa.api.check(L.lib.po_problem_get_vars_and_bounds(dense.handle, xv.handle, lbv.handle, ubv.handle))
            x[:], lb[:], ub[:] = xv.to_numpy(), lbv.to_numpy(), ubv.to_numpy()

        def evalSparseObjCon(self, x, sparse):
            xn = np.array(x, dtype=np.float64)
            fail, f, con = dense.evalObjCon(xv.from_numpy(xn))
            acc = xn[gr.idx[:, 0]].copy()  # (the sum in index order, as the library's group sums take it)
            for k in range(1, nw):
                acc = acc + xn[gr.idx[:, k]]
            sparse[:] = 1.0 - acc
            return fail, f, con

        def evalSparseObjConGradient(self, x, g, A, data):
            xv.from_numpy(np.array(x, dtype=np.float64))
            pa.api.check(L.lib.po_problem_eval_obj_con_gradient(dense.handle, xv.handle, gv.handle, arr))
            g[:] = gv.to_numpy()
            for j in range(c):
                A[j][:] = Av[j].to_numpy()
            data[:] = -1.0
            return 0

    return P(ctx, n, c, c, nwcon=w, nwinequality=w, rowp=rowp, cols=cols)


def test_a_users_csr_problem_through_the_facade(ctx):
    """A user's problem in the CSR form: the pattern is recognised as groups, and the ParOpt.Optimizer facade reaches
    the last row of the built-in twin."""
    import paropt_amd as pa
    from paropt_amd import ParOpt

    _, case = load_golden(WEIGHTING_GOLDEN)
    opts = dict(GROUPS_ON, mma_dual_tol=1e-9, mma_max_iterations=10)
    mma = pa.MMA(make_problem(ctx, case), opts)
    mma.optimize()
    user = user_csr_problem(ctx, case)
    opt = ParOpt.Optimizer(user, dict(opts, algorithm="mma", output_file=None, mma_output_file=None))
    opt.optimize()
    print("built-in %r\nuser     %r" % (mma.getLastRow(), opt.mma.getLastRow()))
    assert opt.mma.getDualStats()["solves"] == 10 and opt.mma.getDualGroupStats()["cap_hits"] == 0
    assert opt.mma.getLastRow() == mma.getLastRow()


def test_refusals_and_registry(ctx):
    import paropt_amd as pa

    weighting = lambda: pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)  # noqa: E731
    mma = pa.MMA(weighting(), dict(GROUPS_ON, mma_max_iterations=2))
    mma.optimize()
    assert mma.getState()["mma_iter"] > 0 and mma.getDualStats()["solves"] == 2
    st = mma.getDualGroupStats()
    assert st["strict"] + st["at_lower"] + st["at_gamma"] == 40 and st["cap_hits"] == 0
    del mma
    gc.collect()

    class Untouched(pa.Problem):  # nothing may run: every callback raises
        def getVarsAndBounds(self, x, lb, ub):
            raise AssertionError("the refused solver ran")

        evalObjCon = evalObjConGradient = evalSparseCon = getVarsAndBounds
        addSparseJacobian = addSparseJacobianTranspose = addSparseInnerProduct = getVarsAndBounds

    blocks = Untouched(ctx, 240, 3, 3, nwcon=40, nwinequality=40, nwblock=2)
    wide = pa.SeparableProblem(ctx, "convex", 1200, 2).setWeighting(2, 600, 0, 0)  # a period beyond a tile
    # (the chain of examples/rosenbrock/sparse_rosenbrock.cpp: span 2, stride 1 -- overlapping rows, the CSR form proper)
    cases = [(pa.SeparableProblem(ctx, "convex", 150, 2).setChain(), GROUPS_ON),
             (blocks, GROUPS_ON),
             (wide, GROUPS_ON),
             (weighting(), dict(GROUPS_ON, mma_globalization="conservative")),
             (weighting(), dict(GROUPS_ON, mma_dual_sparse_constraints="refuse")),
             (weighting(), {"mma_subproblem_solver": "dual"})]
    for prob, opts in cases:
        before = pa.live_objects()[0]
        mma = pa.MMA(prob, opts)
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2 and "sparse constraints" in str(e.value), str(e.value)
        assert len(str(e.value)) > 60
        assert mma.getState()["mma_iter"] == 0
        assert pa.live_objects()[0] == before, "a refused solver allocated vectors"
        del mma
    # a CSR pattern that is recognised as groups (span 2, stride 2) and loses the form at the first gradient (entries
    # -2 x): accepted, then PO_ERR_ARG at that iteration
    mma = pa.MMA(pa.SeparableProblem(ctx, "convex", 150, 2).setChain(2, 2), GROUPS_ON)
    with pytest.raises(pa.ParOptAMDError) as e:
        mma.optimize()
    assert e.value.code == 2 and "lost their grouped form" in str(e.value), str(e.value)
    assert mma.getDualStats()["solves"] == 0
    del mma
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.MMA(weighting(), {"mma_dual_sparse_constraints": "csr"})
    assert e.value.code == 5 and "mma_dual_sparse_constraints" in str(e.value)


def test_no_vectors_leak_and_no_interior_point_is_allocated(ctx):
    import paropt_amd as pa

    _RUNS.clear()
    gc.collect()
    start = pa.live_objects()[0]
    n, c, w = 3000, 3, 500
    prob = pa.SeparableProblem(ctx, "convex", n, c).setWeighting(w, 5, 0, 1)
    base = pa.live_objects()[0]
    counts = {}
    for solver in ("interior_point", "dual"):
        mma = pa.MMA(prob, dict(GROUPS_ON, mma_subproblem_solver=solver, mma_max_iterations=3))
        mma.optimize()
        counts[solver] = pa.live_objects()[0] - base
        del mma
        gc.collect()
        assert pa.live_objects()[0] == base
    # 17 + 3 c vectors of the MMA itself and cw, zw; the groups add the c panel columns (n), c_i, the group weights
    # and c group columns (nwcon): 21 + 5 c in all
    assert counts["dual"] == 17 + 3 * c + 2 + c + 2 + c, counts
    assert counts["interior_point"] >= 17 + 3 * c + 2 + 15 + c, counts
    del prob
    gc.collect()
    assert pa.live_objects()[0] == start


def _group_rows(ctx, case, lams):
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), mma_dual_tol=1e-9, **GROUPS_ON))
    rows = []

    def cb(k):
        rows.append((mma.getState()["subproblem_iter"], tuple(mma.getLastRow())))
        lams.append(mma.getOptimizedPoint()[1].tobytes())

    mma.setIterationCallback(cb)
    mma.optimize()
    return rows, mma.getDualStats(), mma.getDualGroupStats()


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    _, case = load_golden(WEIGHTING_GOLDEN)
    lams = []
    rows, stats, gstats = _group_rows(ctx, case, lams)
    both = [None] * world
    dist.all_gather_object(both, lams)
    if rank == 0:
        q.put((rows, stats, gstats, both))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(ctx):
    _, case = load_golden(WEIGHTING_GOLDEN)
    lams1 = []
    rows1, stats1, gstats1 = _group_rows(ctx, case, lams1)
    rows2, stats2, gstats2, both = run_two_ranks(_worker)
    assert both[0] == both[1], "the multipliers differ between the ranks"
    assert len(rows2) == len(rows1)
    for (s2, r2), (s1, r1) in zip(rows2, rows1):
        assert s2 == s1  # dual-evaluation counts
        for a, b in zip(r2, r1):
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (r2, r1)
    assert {k: stats2[k] for k in ("solves", "iterations", "evaluations", "last_status")} == \
        {k: stats1[k] for k in ("solves", "iterations", "evaluations", "last_status")}
    assert {k: gstats2[k] for k in ("strict", "at_lower", "at_gamma", "cap_hits")} == \
        {k: gstats1[k] for k in ("strict", "at_lower", "at_gamma", "cap_hits")}
