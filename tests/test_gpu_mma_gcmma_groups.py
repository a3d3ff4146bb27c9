"""
GPU: the conservative variant (mma_globalization = "conservative") with the grouped sparse constraints kept in the dual
(mma_gcmma_sparse_constraints = "groups" on top of mma_dual_sparse_constraints = "groups").

  1. the kernels (po_mma_dual_group_eval_rho, po_mma_gcmma_group_point) at the device's own point, in extended precision;
  2. rho = 0 is the plain form, bit for bit;  3. without active groups it is the rho form of the ungrouped dual;
  4. lock step with the numpy restatement;  5. whole runs;  6.-9. refusals, leaks, two ranks, the facade.

Shapes, draw and bounds are those of tests/test_gpu_mma_dual_groups.py; the factor 16 (m + 2) eps of its residual bound
is 16 (m + 7) eps here: one more fma, and the five roundings of w_U, w_L (two differences, a square, a reciprocal, a
product).
"""
import gc
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from mma_dual_group_helpers import WEIGHTING_GOLDEN, Groups, bound_multipliers, classes
from mma_dual_helpers import Subproblem
from mma_gcmma_group_helpers import form_pq_rho, group_solve_rho, oracle_gcmma_groups, quadratic_case
from mma_gcmma_helpers import GCMMA_DEFAULTS, dfun, dprime, fvals
from mma_helpers import mma_options_from_case
from mma_test_util import run_two_ranks
from test_gpu_mma_dual_groups import (ALL_KINDS, EQ_KINDS, GAMMA, GROUPS_ON, INEQ_KINDS, SHAPES, accurate_sum, draw,
                                      found_kinds, golden_groups, make_problem)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
CONSERVATIVE_GROUPS = dict(GROUPS_ON, mma_globalization="conservative", mma_gcmma_sparse_constraints="groups")
# raises per MMA iteration of the restatement's conservative run on `quadratic` 200 x 2, 40 groups of 5
# (tests/test_mma_gcmma_groups_host.py prints the whole list)
LOCKSTEP_RAISES = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 3]


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def _profile(key, record):
    out = os.environ.get("PAROPT_AMD_PROFILE_DIR")
    if out:  # the measurements of profiles/r14_mma_gcmma_groups_parity.json
        path = os.path.join(out, "r14_mma_gcmma_groups_parity.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[key] = record
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


# ---- 1. kernels -----------------------------------------------------------------------------------------------------
def draw_rho(n, nw, skip, start, m, seed):
    """draw() of tests/test_gpu_mma_dual_groups.py with an expansion point strictly inside (alpha, beta) and rho over
    3.5 decades; c is placed as there, relative to the sums of the rho form's unconstrained point.  rho_1..m carry the
    1 / m of the columns p_i, q_i, so that P u^2 stays of order one: the bound on zl, zu is absolute (4 ulp of
    max(|L|, |U|)), as it is there.  In the groups drawn to be strictly free xk sits at the middle of the asymptotes,
    where draw() put their minimisers."""
    sp, lam, gr = draw(n, nw, skip, start, m, seed)
    rng = np.random.default_rng(seed + 12345)
    xk = sp.alpha + (0.1 + 0.8 * rng.random(n)) * (sp.beta - sp.alpha)
    rho = 10.0 ** (-3.0 + 3.5 * rng.random(m + 1))
    rho[1:] /= m
    kinds = [INEQ_KINDS[i % 4] if i < gr.nwineq else EQ_KINDS[(i - gr.nwineq) % 5] for i in range(gr.nwcon)]
    for i, k in enumerate(kinds):
        if k == "strict_free":
            j = gr.idx[i]
            xk[j] = 0.5 * (sp.L[j] + sp.U[j]) + 0.02 * (rng.random(nw) - 0.5)
    assert np.all(xk > sp.alpha) and np.all(xk < sp.beta)
    free = group_solve_rho(sp, xk, rho, lam, Groups(0, 1, 0, 0, -1.0, [], 0))["x"]
    idx = gr.idx
    sa, s0, sb = sp.alpha[idx].sum(axis=1), free[idx].sum(axis=1), sp.beta[idx].sum(axis=1)
    c = np.zeros(gr.nwcon)
    for i, k in enumerate(kinds):
        c[i] = {"inactive": s0[i] + 0.1 * nw, "strict_free": s0[i] - 0.02 * nw,
                "strict_clamped": sa[i] + 0.3 * (s0[i] - sa[i]), "at_gamma": sa[i] - 0.1 * nw,
                "strict_negative": s0[i] + 0.3 * (sb[i] - s0[i]), "at_minus_gamma": sb[i] + 0.1 * nw}[k]
    return sp, lam, Groups(gr.nwcon, nw, start, skip, -1.0, c, gr.nwineq, GAMMA), xk, rho


def pq_extended(sp, xk, rho, lam):
    """The rho form's P, Q in extended precision."""
    P, Q = sp.p0.astype(LD), sp.q0.astype(LD)
    for i in range(sp.m):
        P = P + LD(lam[i]) * sp.p[i].astype(LD)
        Q = Q + LD(lam[i]) * sp.q[i].astype(LD)
    sigma = LD(rho[0]) + np.dot(lam.astype(LD), rho[1:].astype(LD))
    Ll, Ul, xl = sp.L.astype(LD), sp.U.astype(LD), xk.astype(LD)
    return P + sigma * (Ul - xl) ** 2 / (Ul - Ll), Q + sigma * (xl - Ll) ** 2 / (Ul - Ll)


def residual_ratios_rho(sp, xk, rho, lam, gr, x, zw):
    """residual_ratios of tests/test_gpu_mma_dual_groups.py with the rho form's P, Q and the factor 16 (m + 7) eps; also
    psi, its bound and the class of every group."""
    m = sp.m
    P, Q = pq_extended(sp, xk, rho, lam)
    xl = x.astype(LD)
    u, l = 1 / (sp.U.astype(LD) - xl), 1 / (xl - sp.L.astype(LD))
    t = np.zeros(sp.n, dtype=LD)
    if gr.nwcon:
        t[gr.idx] = (LD(gr.a) * zw.astype(LD))[:, None]
    res = P * u * u - Q * l * l - t
    h = 2 * (P * u**3 + Q * l**3)
    sp_lu = np.spacing(np.maximum(np.abs(sp.L), np.abs(sp.U))).astype(LD)
    bound = 4 * h * sp_lu + 16 * (m + 7) * LD(EPS) * (P * u * u + Q * l * l)
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
        out["groups"] = (psi, gb, cls)
    return out


def sums_at_point_rho(sp, xk, rho, lam, gr, x, zw):
    """W, grad, H, the Delta_i and D at the device's own point, classes from the device's values: (value, largest term)
    each, the sums taken accurately."""
    m = sp.m
    P0, Q0, P, Q = form_pq_rho(sp, xk, rho, lam)
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    dterms = dfun(sp, xk, x)
    D, Dmax = float(accurate_sum(dterms)), float(dterms.max())
    wterms = P0 * u + Q0 * l + sigma * dterms
    gterms = sp.p * u + sp.q * l + rho[1:, None] * dterms
    free = (x > sp.alpha) & (x < sp.beta)
    d = np.where(free, 1.0 / (2.0 * (P * u**3 + Q * l**3)), 0.0)
    G = sp.p * u**2 - sp.q * l**2 + np.outer(rho[1:], dprime(sp, xk, x))
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
    uk, lk = 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
    du, dl = (x - xk) * u * uk, -(x - xk) * l * lk
    pterms = np.vstack([sp.p0 * du + sp.q0 * dl] + [sp.p[i] * du + sp.q[i] * dl for i in range(m)] + [dterms])
    S, Smax = accurate_sum(pterms), np.abs(pterms).max(axis=1)
    return W, Wmax, g, gmax, H, Hmax, D, Dmax, S, Smax


def upload(ctx, sp, gr, xk=None):
    import paropt_amd as pa

    n = sp.n
    up = lambda a, k=n: pa.PVec(ctx, k).from_numpy(a)  # noqa: E731
    dev = dict(head=(up(sp.L), up(sp.U), up(sp.alpha), up(sp.beta), up(sp.p0), up(sp.q0),
                     [up(sp.p[i]) for i in range(sp.m)], [up(sp.q[i]) for i in range(sp.m)]),
               c=up(gr.c, gr.nwcon) if gr.nwcon else None, xk=up(xk) if xk is not None else None)
    dev["groups"] = (gr.nwcon, gr.nw, gr.start, gr.skip, gr.a, dev["c"], gr.nwineq, gr.gamma)
    return dev


def new_point(ctx, sp, gr):
    import paropt_amd as pa

    return [pa.PVec(ctx, sp.n) for _ in range(3)], (pa.PVec(ctx, gr.nwcon) if gr.nwcon else None)


def download(pt, zw):
    return [v.to_numpy() for v in pt] + [zw.to_numpy() if zw is not None else np.zeros(0)]


def device_eval_rho(ctx, sp, lam, gr, xk, rho):
    """(W, g, H, stats, D, x, zl, zu, zw) of po_mma_dual_group_eval_rho and (sums, stats, x, zl, zu, zw) of
    po_mma_gcmma_group_point."""
    import paropt_amd as pa

    dev = upload(ctx, sp, gr, xk)
    pt, zw = new_point(ctx, sp, gr)
    W, g, H, st, D = pa.mma_dual_group_eval(ctx, *dev["head"], sp.b, lam, *dev["groups"], pt, zw, xk=dev["xk"], rho=rho)
    ev = (W, g, H, st, D, *download(pt, zw))
    pt, zw = new_point(ctx, sp, gr)
    sums, st2 = pa.mma_gcmma_group_point(ctx, *dev["head"], lam, *dev["groups"], dev["xk"], rho, pt, zw)
    return ev, (sums, st2, *download(pt, zw))


@pytest.mark.parametrize("m", [1, 3, 8, 9, 33])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_nw%d_skip%d_start%d" % s)
def test_group_kernels_rho(ctx, shape, m):
    n, nw, skip, start = shape
    sp, lam, gr, xk, rho = draw_rho(n, nw, skip, start, m, seed=100 * m + n % 97)
    ref = group_solve_rho(sp, xk, rho, lam, gr)  # the restatement alone: every kind of group is in the draw
    assert ref["cap"] == 0
    if gr.nwcon >= 8:
        kinds = found_kinds(sp, gr, ref["x"], ref["zw"])
        assert kinds == ALL_KINDS, sorted(ALL_KINDS - kinds)
    (W, g, H, st, D, x, zl, zu, zw), (sums, st2, x2, zl2, zu2, zw2) = device_eval_rho(ctx, sp, lam, gr, xk, rho)
    # the point entry is the same group solve
    assert np.array_equal(x, x2) and np.array_equal(zw, zw2)
    assert st == st2
    # exact: the point lies inside its boxes
    assert np.all(x >= sp.alpha) and np.all(x <= sp.beta)
    assert np.all(zw >= gr.zlo) and np.all(zw <= gr.gamma)
    assert st["cap_hits"] == 0 and st["strict"] + st["at_lower"] + st["at_gamma"] == gr.nwcon
    cls = classes(gr, zw)
    assert (st["strict"], st["at_lower"], st["at_gamma"]) == tuple(int((cls == k).sum()) for k in (1, 0, 2))
    if gr.nwcon >= 8:
        assert found_kinds(sp, gr, x, zw) == ALL_KINDS
    ratios = residual_ratios_rho(sp, xk, rho, lam, gr, x, zw)
    ratios.pop("groups", None)
    Wr, Wmax, gr_, gmax, Hr, Hmax, Dr, Dmax, Sr, Smax = sums_at_point_rho(sp, xk, rho, lam, gr, x, zw)
    tiny = 1e-300
    rW = abs(W - Wr) / (1e-13 * n * Wmax)
    rg = float((np.abs(g - gr_) / np.maximum(1e-13 * n * gmax, tiny)).max())
    rH = float((np.abs(H - Hr) / np.maximum(1e-13 * n * Hmax, tiny)).max())
    rD = abs(D - Dr) / max(1e-13 * n * Dmax, tiny)
    rS = float((np.abs(sums - Sr) / np.maximum(1e-13 * n * Smax, tiny)).max())
    _, _, P, Q = form_pq_rho(sp, xk, rho, lam)
    zlr, zur = bound_multipliers(sp, gr, dict(P=P, Q=Q, x=x, zw=zw))
    zb = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
    rz = float(max((np.abs(zl2 - zlr) / zb).max(), (np.abs(zu2 - zur) / zb).max()))
    record = dict(ratios, W=rW, grad=rg, hess=rH, D=rD, point_sums=rS, zl_zu=rz, max_inner=st["max_inner"],
                  mean_inner=st["steps"] / max(1, gr.nwcon), groups=gr.nwcon, rho_min=float(rho.min()),
                  rho_max=float(rho.max()))
    print("n=%d nw=%d skip=%d start=%d m=%d: %s" % (n, nw, skip, start, m, json.dumps(record)))
    _profile("kernels n%d_nw%d_skip%d_start%d m%d" % (n, nw, skip, start, m), record)
    for key in ("free", "clamped", "strict", "ends"):
        assert ratios.get(key, 0.0) <= 1.0, (key, ratios)
    assert rW <= 1.0 and rg <= 1.0 and rH <= 1.0 and rD <= 1.0 and rS <= 1.0, (rW, rg, rH, rD, rS)
    assert np.array_equal(H, H.T)
    assert rz <= 1.0
    assert np.array_equal(zl, zl2) and np.array_equal(zu, zu2)
    assert sums.shape == (m + 2,) and sums[m + 1] == D


# ---- 2. rho = 0 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 9])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "n%d_nw%d_skip%d_start%d" % s)
def test_rho_zero_is_the_plain_form_bitwise(ctx, shape, m):
    import paropt_amd as pa

    n, nw, skip, start = shape
    sp, lam, gr, xk, _ = draw_rho(n, nw, skip, start, m, seed=11 + m)
    dev = upload(ctx, sp, gr, xk)
    pt, zw = new_point(ctx, sp, gr)
    W0, g0, H0, st0 = pa.mma_dual_group_eval(ctx, *dev["head"], sp.b, lam, *dev["groups"], pt, zw)
    plain = download(pt, zw)
    assert st0["strict"] > 0
    (W, g, H, st, D, *point), (sums, st2, *point2) = device_eval_rho(ctx, sp, lam, gr, xk, np.zeros(m + 1))
    for a, b, c in zip(plain, point, point2):  # x, zl, zu, zw
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert W == W0 and np.array_equal(g, g0) and np.array_equal(H, H0)
    assert st == st0 and st2 == st0
    assert D >= 0.0


# ---- 3. without active groups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "n%d_nw%d_skip%d_start%d" % s)
def test_without_active_groups_it_is_the_rho_form_of_the_ungrouped_dual(ctx, shape):
    import paropt_amd as pa

    n, nw, skip, start = shape
    m = 3
    sp, lam, gr, xk, rho = draw_rho(n, nw, skip, start, m, seed=7)
    none = Groups(0, 1, 0, 0, -1.0, [], 0, GAMMA)
    dev = upload(ctx, sp, none, xk)
    W0, g0, H0, D0 = pa.mma_dual_eval(ctx, *dev["head"], sp.b, lam, form=2, xk=dev["xk"], rho=rho)
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    sums0 = pa.mma_gcmma_point(ctx, *dev["head"], lam, dev["xk"], rho, pt)
    x0, zl0, zu0 = (v.to_numpy() for v in pt)
    Wr, Wmax, gr_, gmax, Hr, Hmax, Dr, Dmax, Sr, Smax = sums_at_point_rho(sp, xk, rho, lam, none, x0, np.zeros(0))
    inactive = Groups(gr.nwcon, nw, start, skip, -1.0, sp.beta[gr.idx].sum(axis=1) + 1.0, gr.nwcon, GAMMA)
    for g_ in (none, inactive):
        (W, g, H, st, D, x, zl, zu, zw), (sums, _, x2, zl2, zu2, _) = device_eval_rho(ctx, sp, lam, g_, xk, rho)
        assert np.all(zw == 0.0) and st["strict"] == st["at_gamma"] == 0 and st["at_lower"] == g_.nwcon
        assert abs(W - W0) <= 1e-13 * n * Wmax and np.all(np.abs(g - g0) <= 1e-13 * n * gmax)
        assert np.all(np.abs(H - H0) <= 1e-13 * n * Hmax)
        assert abs(D - D0) <= 1e-13 * n * Dmax and np.all(np.abs(sums - sums0) <= 1e-13 * n * Smax)
        zb = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
        assert np.all(np.abs(x - x0) <= zb) and np.all(np.abs(zl2 - zl0) <= zb) and np.all(np.abs(zu2 - zu0) <= zb)


# ---- shared runs ----------------------------------------------------------------------------------------------------
def run_mma(ctx, case, extra, keep=False):
    """One MMA run through the library: (mma, rows, per-callback records)."""
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(opts, **mopts), mma_dual_tol=1e-9, **extra))
    rows, recs = [], []

    def cb(k):
        rows.append(mma.getLastRow())
        st, gs = mma.getState(), mma.getGlobalizationStats()
        rec = dict(fobj=st["fobj"], cons=st["cons"].copy(), sub_iter=st["subproblem_iter"], inner_last=gs["inner_last"],
                   cap_hits=gs["cap_hits"], rho=gs["rho"].copy(), z=mma.getOptimizedPoint()[1].copy(),
                   gstats=mma.getDualGroupStats(), status=mma.getDualStats()["last_status"])
        if keep:
            # (inside callback k the subproblem, the asymptotes and rho are still those of iteration k - 1, whose
            # solution x is)
            s = mma.getSubproblem()
            lo, up = mma.getAsymptotes()
            rec["sp"] = Subproblem(lo.to_numpy(), up.to_numpy(), s["alpha"].to_numpy(), s["beta"].to_numpy(),
                                   s["p0"].to_numpy(), s["q0"].to_numpy(), [v.to_numpy() for v in s["p"]],
                                   [v.to_numpy() for v in s["q"]], s["b"])
            x, _, zw, _, _ = mma.getOptimizedPoint()
            rec["x"], rec["zw"] = x.to_numpy(), zw.to_numpy()
        recs.append(rec)

    mma.setIterationCallback(cb)
    mma.optimize()
    return mma, rows, recs


def weighting_case(kind):
    _, case = load_golden(WEIGHTING_GOLDEN)
    return case if kind == "convex" else quadratic_case(case)


def stopped(row):  # the stop test of MMA::optimize (the driver's permuted names: l1, linfty, infeas)
    return row[1] < 1e-5 and (row[2] < 1e-6 or row[4] < 1e-6)


@pytest.fixture(scope="module")
def quadratic_run(ctx):
    """The library's conservative grouped run on `quadratic` to its stop, with everything the callbacks downloaded."""
    run = run_mma(ctx, weighting_case("quadratic"), dict(CONSERVATIVE_GROUPS, mma_max_iterations=80), keep=True)
    yield run
    del run
    gc.collect()


# ---- 4. lock step ---------------------------------------------------------------------------------------------------
def test_lockstep_with_the_restatement(ctx, quadratic_run):
    case = weighting_case("quadratic")
    _, mopts = mma_options_from_case(case)
    window = len(LOCKSTEP_RAISES)
    its, omma, _ = oracle_gcmma_groups(case, dict(mopts, mma_max_iterations=80), {}, 1e-9, 200, window, stop=False)
    assert [it["raises"] for it in its] == LOCKSTEP_RAISES and sum(LOCKSTEP_RAISES) > 0
    margin = min(it["margin"] for it in its)
    print("smallest distance of a decision of the restatement from its threshold: %.3e" % margin)
    assert margin > 1e-6
    mma, rows, recs = quadratic_run
    assert len(rows) > window
    raises = [r["inner_last"] for r in recs[1:window + 1]]
    print("raises per iteration:", raises)
    assert raises == LOCKSTEP_RAISES
    for k in range(window):
        it, rec = its[k], recs[k + 1]
        assert np.all(np.abs(rec["rho"] - it["rho"]) <= 1e-6 * it["rho"]), (k, rec["rho"], it["rho"])
        assert np.all(np.abs(rec["z"] - it["lam"]) <= 1e-6 * np.maximum(1.0, np.abs(it["lam"]))), (k, rec["z"], it["lam"])
    for k in range(window + 1):
        t = omma.trace[k]
        assert abs(rows[k][0] - t["fobj"]) <= 1e-6 * max(1.0, abs(t["fobj"])), (k, rows[k][0], t["fobj"])


# ---- 5. whole runs --------------------------------------------------------------------------------------------------
def test_quadratic_run_is_conservative_feasible_and_monotone(ctx, quadratic_run):
    mma, rows, recs = quadratic_run
    gr = golden_groups(weighting_case("quadratic"))
    tol = GCMMA_DEFAULTS["mma_gcmma_tol"]
    gs = mma.getGlobalizationStats()
    print("conservative: %d MMA iterations, %s, last row %s" % (len(rows) - 1, gs, rows[-1]))
    assert len(rows) - 1 <= 80 and stopped(rows[-1])
    assert gs["cap_hits"] == 0
    root_caps = 0
    for k in range(1, len(recs)):
        prev, cur = recs[k - 1], recs[k]
        assert cur["status"] == 0
        root_caps += cur["gstats"]["cap_hits"]
        sp, xk, x, rho, zw = cur["sp"], prev["x"], cur["x"], cur["rho"], cur["zw"]
        assert np.all(sp.alpha <= x) and np.all(x <= sp.beta) and np.all(sp.alpha <= xk) and np.all(xk <= sp.beta)
        # conservative at acceptance, recomputed from the downloaded subproblem
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
        assert np.all(fnew <= approx + slack), (k, fnew, approx)
        # the groups: psi within the group bound of the plain grouped dual, or the group sits at gamma
        psi, gb, cls = residual_ratios_rho(sp, xk, rho, cur["z"], gr, x, zw)["groups"]
        assert np.all(np.abs(psi)[cls == 1] <= gb[cls == 1]) and np.all(psi[cls == 0] >= -gb[cls == 0]), (k, psi, gb)
    print("cap hits of the root searches over the run: %d" % root_caps)
    assert root_caps == 0  # (the restatement has none on this run)
    feasible = [r[4] <= 1e-6 for r in rows]
    rises = [rows[k][0] - rows[k - 1][0] for k in range(1, len(rows)) if feasible[k] and feasible[k - 1]]
    print("largest rise of fobj between consecutive feasible iterates: %.3e" % max(rises))
    for k in range(1, len(rows)):
        if feasible[k] and feasible[k - 1]:
            assert rows[k][0] <= rows[k - 1][0] + tol * max(1.0, abs(rows[k][0])), (k, rows[k - 1][0], rows[k][0])
    # the contrast: plain MMA with the same options has not stopped at 80 (the parent's library shows the same rows)
    _, rows0, _ = run_mma(ctx, weighting_case("quadratic"), dict(GROUPS_ON, mma_max_iterations=80))
    print("none: %d MMA iterations, last row %s" % (len(rows0) - 1, rows0[-1]))
    assert len(rows0) - 1 == 80 and not any(stopped(r) for r in rows0[1:])
    _profile("quadratic_run", dict(iterations=len(rows) - 1, stats=dict(gs, rho=gs["rho"].tolist()),
                                   last_row=list(rows[-1]), root_cap_hits=root_caps, largest_rise=max(rises),
                                   raises=[r["inner_last"] for r in recs[1:]], plain_last_row=list(rows0[-1]),
                                   plain_fobj_8_13=[r[0] for r in rows0[8:13]]))


def test_convex_run_reaches_the_objective_of_the_plain_grouped_run(ctx):
    case = weighting_case("convex")
    out = {}
    for name, extra in (("conservative", CONSERVATIVE_GROUPS), ("none", GROUPS_ON)):
        mma, rows, recs = run_mma(ctx, case, dict(extra, mma_max_iterations=200))
        assert stopped(rows[-1]), (name, rows[-1])
        out[name] = dict(iterations=len(rows) - 1, fobj=rows[-1][0], stats=mma.getGlobalizationStats(),
                         root_cap_hits=sum(r["gstats"]["cap_hits"] for r in recs[1:]),
                         raises=[r["inner_last"] for r in recs[1:]])
        out[name]["stats"]["rho"] = out[name]["stats"]["rho"].tolist()
        del mma
    print(json.dumps(out))
    _profile("convex_runs", out)
    # the two restatement runs end at 265.0618094070654 and 265.0618094070653 (relative 4.3e-16): ten times that, and
    # not below 1e-8
    fa, fb = out["conservative"]["fobj"], out["none"]["fobj"]
    assert abs(fa - fb) <= max(10 * 4.3e-16, 1e-8) * abs(fb), (fa, fb)
    assert out["conservative"]["stats"]["inner_total"] > 0 and out["none"]["stats"]["inner_total"] == 0
    # (the restatement's element searches, with the rho form's second stop, meet no cap on this run)
    assert out["conservative"]["root_cap_hits"] == 0 and out["conservative"]["stats"]["cap_hits"] == 0


# ---- 6. refusals and registry ---------------------------------------------------------------------------------------
def test_refusals_and_registry(ctx):
    import paropt_amd as pa

    weighting = lambda: pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)  # noqa: E731

    class Untouched(pa.Problem):  # nothing may run: every callback raises
        def getVarsAndBounds(self, x, lb, ub):
            raise AssertionError("the refused solver ran")

        evalObjCon = evalObjConGradient = evalSparseCon = getVarsAndBounds
        addSparseJacobian = addSparseJacobianTranspose = addSparseInnerProduct = getVarsAndBounds

    on = CONSERVATIVE_GROUPS
    blocks = Untouched(ctx, 240, 3, 3, nwcon=40, nwinequality=40, nwblock=2)
    wide = pa.SeparableProblem(ctx, "convex", 1200, 2).setWeighting(2, 600, 0, 0)  # a period beyond a tile
    # a dense equality on top of a pattern that is recognised as groups (40 rows of 6 consecutive columns)
    rowp, cols = (np.arange(41) * 6).astype(np.intc), np.arange(240).astype(np.intc)
    cases = [(weighting(), dict(on, mma_gcmma_sparse_constraints="refuse"), "mma_gcmma_sparse_constraints"),
             (weighting(), dict(GROUPS_ON, mma_globalization="conservative"), "mma_gcmma_sparse_constraints"),
             (pa.SeparableProblem(ctx, "convex", 150, 2).setChain(), on, "sparse constraints"),
             (blocks, on, "sparse constraints"),
             (wide, on, "sparse constraints"),
             (weighting(), dict(on, mma_dual_sparse_constraints="refuse"), "sparse constraints"),
             (Untouched(ctx, 240, 3, 2, nwcon=40, nwinequality=40, rowp=rowp, cols=cols), on, "equality constraint")]
    for prob, opts, sentence in cases:
        gc.collect()
        before = pa.live_objects()[0]
        mma = pa.MMA(prob, opts)
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2 and sentence in str(e.value), str(e.value)
        assert mma.getState()["mma_iter"] == 0
        assert pa.live_objects()[0] == before, "a refused solver allocated vectors"
        del mma
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.MMA(weighting(), {"mma_gcmma_sparse_constraints": "csr"})
    assert e.value.code == 5 and "mma_gcmma_sparse_constraints" in str(e.value)
    # the option alone changes nothing: plain grouped MMA runs as before
    mma = pa.MMA(weighting(), dict(GROUPS_ON, mma_gcmma_sparse_constraints="groups", mma_max_iterations=2))
    mma.optimize()
    assert mma.getDualStats()["solves"] == 2 and mma.getGlobalizationStats()["inner_total"] == 0
    mma = pa.MMA(weighting(), dict(on, mma_max_iterations=2))
    mma.optimize()
    assert mma.getState()["mma_iter"] > 0 and mma.getDualStats()["solves"] >= 2


# ---- 7. no leak -----------------------------------------------------------------------------------------------------
def test_no_vectors_leak_and_none_are_added(ctx):
    import paropt_amd as pa

    gc.collect()
    start = pa.live_objects()[0]
    n, c, w = 3000, 3, 500
    prob = pa.SeparableProblem(ctx, "convex", n, c).setWeighting(w, 5, 0, 1)
    base = pa.live_objects()[0]
    counts = {}
    for name, extra in (("none", GROUPS_ON), ("conservative", CONSERVATIVE_GROUPS)):
        mma = pa.MMA(prob, dict(extra, mma_max_iterations=3))
        seen = []
        mma.setIterationCallback(lambda k: seen.append(pa.live_objects()[0] - base))
        mma.optimize()
        counts[name] = (pa.live_objects()[0] - base, max(seen))
        del mma
        gc.collect()
        assert pa.live_objects()[0] == base
    # the inner iteration works on the vectors the grouped dual has: 21 + 5 c
    assert counts["conservative"] == counts["none"] == (21 + 5 * c, 21 + 5 * c), counts
    del prob
    gc.collect()
    assert pa.live_objects()[0] == start


# ---- 8. two ranks ---------------------------------------------------------------------------------------------------
def _counts(ctx):
    """Raises, evaluation counts and multipliers of the first iterations of the conservative run on `quadratic`."""
    mma, rows, recs = run_mma(ctx, weighting_case("quadratic"),
                              dict(CONSERVATIVE_GROUPS, mma_max_iterations=len(LOCKSTEP_RAISES)))
    gs, ds = mma.getGlobalizationStats(), mma.getDualStats()
    return dict(inner=[r["inner_last"] for r in recs], sub_iter=[r["sub_iter"] for r in recs],
                cap_hits=gs["cap_hits"], inner_total=gs["inner_total"],
                dual={k: ds[k] for k in ("solves", "iterations", "evaluations", "last_status")},
                z=[r["z"].tolist() for r in recs], fobj=[r[0] for r in rows])


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
    assert one["inner"][1:] == LOCKSTEP_RAISES
    for key in ("inner", "cap_hits", "inner_total", "sub_iter", "dual"):
        assert two[key] == one[key], (key, two[key], one[key])
    for a, b in zip(two["z"], one["z"]):
        assert np.all(np.abs(np.array(a) - np.array(b)) <= 1e-9 * np.maximum(1.0, np.abs(b))), (a, b)
    for a, b in zip(two["fobj"], one["fobj"]):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (a, b)


# ---- 9. the facade --------------------------------------------------------------------------------------------------
def test_facade_optimizer_reaches_the_same_last_row(ctx):
    import paropt_amd as pa
    from paropt_amd import ParOpt

    case = weighting_case("quadratic")
    opts = dict(CONSERVATIVE_GROUPS, mma_dual_tol=1e-9, mma_max_iterations=len(LOCKSTEP_RAISES))
    mma = pa.MMA(make_problem(ctx, case), opts)
    mma.optimize()
    opt = ParOpt.Optimizer(make_problem(ctx, case), dict(opts, algorithm="mma", output_file=None, mma_output_file=None))
    opt.optimize()
    assert opt.mma.getLastRow() == mma.getLastRow()
    a, b = opt.mma.getGlobalizationStats(), mma.getGlobalizationStats()
    assert a["inner_total"] == b["inner_total"] == sum(LOCKSTEP_RAISES) and np.array_equal(a["rho"], b["rho"])
    assert opt.mma.getDualGroupStats() == mma.getDualGroupStats()
