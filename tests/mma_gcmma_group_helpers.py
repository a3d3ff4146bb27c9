"""numpy restatement of the conservative variant (mma_globalization = "conservative") with the grouped sparse
constraints kept in the dual (mma_gcmma_sparse_constraints = "groups"; paropt_amd/csrc/mma.hip, the rho form of the
group solve), on top of tests/mma_dual_group_helpers.py and tests/mma_gcmma_helpers.py.  Independent of the library.

In the grouped form the sparse constraints are affine, psi_i(x) = a sum x + c_i: their approximation is exact, so they
carry no rho and take no part in the acceptance test.  The rho terms only change the separable part,
    P = P0 + sigma w_U,  Q = Q0 + sigma w_L,  sigma = rho_0 + lam . rho[1:]   (P0, Q0 as form_pq accumulates them),
and column i of the Hessian gains rho_i d'(x)."""
import numpy as np

from mma_dual_group_helpers import (NEWTON_CAP, bound_multipliers, classes, closed_form, form_pq, groups_of_oracle,
                                    oracle_weighting_problem, phi1)
from mma_dual_helpers import Subproblem, projected_gradient
from mma_gcmma_helpers import GCMMA_DEFAULTS, acceptance, dfun, dprime, fvals, raise_rho, rho_start, weights


def form_pq_rho(sp, xk, rho, lam):
    """(P0, Q0, P, Q): the sigma term is added last, as one fma per element on the device."""
    P0, Q0 = form_pq(sp, lam)
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    wU, wL = weights(sp, xk)
    return P0, Q0, P0 + sigma * wU, Q0 + sigma * wL


def element_roots_rho(P, Q, L, U, alpha, beta, t, x0):
    """element_roots of mma_dual_group_helpers with the rho form's second stop: the search of an element also ends when
    its step changes neither U - x nor x - L.  (Where |x| << |L|, |U| a step of one ulp of x is below the resolution
    of both differences: phi' keeps its rounding residue, which a large sigma makes large, the step keeps its size and
    x creeps one ulp at a time into the cap.)  Until that stop acts, the two are the same iteration."""
    ga, gb = phi1(P, Q, L, U, alpha), phi1(P, Q, L, U, beta)
    x = np.where(t <= ga, alpha, np.where(t >= gb, beta, x0))
    zero = t == 0.0
    x = np.where(zero, closed_form(P, Q, L, U, alpha, beta), x)
    act = (t > ga) & (t < gb) & ~zero
    lo, hi = alpha.copy(), beta.copy()
    outside = act & ~((x > lo) & (x < hi))
    x = np.where(outside, 0.5 * (lo + hi), x)
    for _ in range(NEWTON_CAP):
        if not act.any():
            return x, 0
        u, l = 1.0 / (U - x), 1.0 / (x - L)
        f = P * u * u - Q * l * l - t
        h = 2.0 * (P * u**3 + Q * l**3)
        lo = np.where(act & (f < 0.0), x, lo)
        hi = np.where(act & (f > 0.0), x, hi)
        act = act & (f != 0.0)
        with np.errstate(all="ignore"):
            xn = x - f / h
        xn = np.where((xn > lo) & (xn < hi), xn, 0.5 * (lo + hi))
        stop = ~((xn > lo) & (xn < hi)) | (xn == x) | ((U - xn == U - x) & (xn - L == x - L))
        x = np.where(act & ~stop, xn, x)
        act = act & ~stop
    return x, int(act.sum())


def group_solve_rho(sp, xk, rho, lam, gr, roots=element_roots_rho):
    """group_solve of mma_dual_group_helpers on the full P, Q, its element searches through `roots`: the point dict
    with P, Q, P0, Q0, x (n), zw, psi, s, steps per group, cap."""
    P0, Q0, P, Q = form_pq_rho(sp, xk, rho, lam)
    x = closed_form(P, Q, sp.L, sp.U, sp.alpha, sp.beta)
    w = gr.nwcon
    out = dict(P=P, Q=Q, P0=P0, Q0=Q0, x=x, zw=np.zeros(w), psi=np.zeros(w), s=np.zeros(w),
               steps=np.zeros(w, dtype=int), cap=0)
    if w == 0:
        return out
    ix = gr.idx
    e = [a[ix] for a in (P, Q, sp.L, sp.U, sp.alpha, sp.beta)]
    xg = x[ix].copy()
    zw, lo, hi = gr.zlo.copy(), gr.zlo.copy(), np.full(w, gr.gamma)
    hik = np.zeros(w, dtype=bool)
    act = np.ones(w, dtype=bool)
    psi, sd = np.zeros(w), np.zeros(w)
    steps = np.zeros(w, dtype=int)
    cap = 0
    while act.any():
        t = np.broadcast_to((gr.a * zw)[:, None], xg.shape)
        xa, c1 = roots(*[a[act] for a in e], t[act], xg[act])
        cap += c1
        xg[act] = xa
        Pe, Qe, Le, Ue, ae, be = [a[act] for a in e]
        u, l = 1.0 / (Ue - xa), 1.0 / (xa - Le)
        d = np.where((xa > ae) & (xa < be), 1.0 / (2.0 * (Pe * u**3 + Qe * l**3)), 0.0)
        psi[act] = gr.a * xa.sum(axis=1) + gr.c[act]
        sd[act] = d.sum(axis=1)
        steps[act] += 1
        done = act & (((zw == gr.zlo) & (psi >= 0.0)) | ((zw == gr.gamma) & (psi <= 0.0)) | (psi == 0.0))
        go = act & ~done
        lo = np.where(go & (psi < 0.0), zw, lo)
        up = go & (psi > 0.0)
        hi = np.where(up, zw, hi)
        hik = hik | up
        with np.errstate(all="ignore"):
            zn = np.where(sd > 0.0, zw - psi / (gr.a * gr.a * sd), hi)
        inside = (zn > lo) & (zn < hi)
        zn = np.where(inside, zn, np.where(hik, 0.5 * (lo + hi), gr.gamma))
        inside = (zn > lo) & (zn < hi)
        stop = go & ((hik & ~inside) | (zn == zw))
        capped = go & ~stop & (steps >= NEWTON_CAP)
        cap += int(capped.sum())
        move = go & ~stop & ~capped
        zw = np.where(move, zn, zw)
        act = move
    x[ix] = xg
    out.update(x=x, zw=zw, psi=psi, s=sd, steps=steps, cap=cap)
    return out


def dual_eval_groups_rho(sp, xk, rho, lam, gr, pt=None):
    """W, grad W, -hess W, D and the point dict of the rho form."""
    pt = pt or group_solve_rho(sp, xk, rho, lam, gr)
    P, Q, x = pt["P"], pt["Q"], pt["x"]
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    D = float(np.sum(dfun(sp, xk, x)))
    W = float(np.sum(pt["P0"] * u + pt["Q0"] * l) + sigma * D - np.dot(pt["zw"], pt["psi"]) + np.dot(lam, sp.b))
    g = np.array([np.sum(sp.p[i] * u + sp.q[i] * l) for i in range(sp.m)]) + rho[1:] * D + sp.b
    free = (x > sp.alpha) & (x < sp.beta)
    d = np.where(free, 1.0 / (2.0 * (P * u**3 + Q * l**3)), 0.0)
    G = sp.p * u**2 - sp.q * l**2 + np.outer(rho[1:], dprime(sp, xk, x))
    H = (G * d) @ G.T
    if gr.nwcon:
        ag = (G * d)[:, gr.idx].sum(axis=2)
        sg = d[gr.idx].sum(axis=1)
        wgt = np.where((classes(gr, pt["zw"]) == 1) & (sg > 0.0), 1.0 / np.where(sg > 0.0, sg, 1.0), 0.0)
        H = H - (ag * wgt) @ ag.T
    return W, g, H, D, pt


def point_sums(sp, xk, x):
    """The m + 2 sums [Delta_0, Delta_1..m, D] at a stored point; Delta_i = f~_i(x) - f~_i(xk) without the rho term."""
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    uk, lk = 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
    du, dl = (x - xk) * u * uk, -(x - xk) * l * lk  # u - uk, l - lk
    sums = np.zeros(sp.m + 2)
    sums[0] = np.sum(sp.p0 * du + sp.q0 * dl)
    for i in range(sp.m):
        sums[1 + i] = np.sum(sp.p[i] * du + sp.q[i] * dl)
    sums[sp.m + 1] = np.sum(dfun(sp, xk, x))
    return sums


def shifted_subproblem(sp, xk, rho):
    """The plain subproblem whose grouped dual is the rho form on (sp, xk, rho): p_i + rho_i w_U, q_i + rho_i w_L
    (i = 0..m) and b_i - rho_i n, since sum w_U u + w_L l = d + n.  (W of the two differs by the constant rho_0 n.)"""
    wU, wL = weights(sp, xk)
    return Subproblem(sp.L, sp.U, sp.alpha, sp.beta, sp.p0 + rho[0] * wU, sp.q0 + rho[0] * wL,
                      sp.p + np.outer(rho[1:], wU), sp.q + np.outer(rho[1:], wL), sp.b - rho[1:] * sp.n)


def dual_solve_groups_rho(sp, xk, rho, lam0, gr, tol, max_evals):
    """The iteration of mma_dual_solve on the rho form of the grouped dual: (lam, status, evaluations, max|pg|,
    point, most steps of a group, cap hits)."""
    gamma = np.full(sp.m, gr.gamma)
    lam = np.clip(np.asarray(lam0, dtype=np.float64), 0.0, gamma)
    W, g, H, _, pt = dual_eval_groups_rho(sp, xk, rho, lam, gr)
    evals, most, cap = 1, int(pt["steps"].max(initial=0)), pt["cap"]
    tau = 1e-8 * max(1.0, float(np.trace(H)))
    while True:
        pg = projected_gradient(lam, g, gamma)
        pgmax = float(np.max(np.abs(pg))) if sp.m else 0.0
        if pgmax <= tol:
            return lam, 0, evals, pgmax, pt, most, cap
        if evals >= max_evals or not tau <= 1e30:
            return lam, 1, evals, pgmax, pt, most, cap
        F = np.nonzero(pg != 0.0)[0]
        d = np.zeros(sp.m)
        d[F] = np.linalg.solve(H[np.ix_(F, F)] + tau * np.eye(F.size), g[F])
        cand = np.clip(lam + d, 0.0, gamma)
        cand[pg == 0.0] = lam[pg == 0.0]
        Wc, gc, Hc, _, ptc = dual_eval_groups_rho(sp, xk, rho, cand, gr)
        evals += 1
        most, cap = max(most, int(ptc["steps"].max(initial=0))), cap + ptc["cap"]
        slope = float(np.dot(g, cand - lam))
        accept = Wc >= W + 1e-4 * slope
        if not accept and Wc >= W + 1e-4 * slope - 1e-13 * max(1.0, abs(W)):  # within the rounding error of W
            accept = float(np.max(np.abs(projected_gradient(cand, gc, gamma)))) < pgmax
        if accept:
            lam, W, g, H, pt = cand, Wc, gc, Hc, ptc
            tau = max(tau / 8.0, 1e-14)
        else:
            tau *= 8.0


def gcmma_group_iteration(mma, opts, dual_tol, max_evals):
    """One conservative MMA iteration on the oracle's MMA object with groups (gcmma_iteration of mma_gcmma_helpers with
    the grouped dual): dict(sp, gr, xk, fk, rho0, rho, lam0, lam, x, zw, zl, zu, sums, fnew, raises, capped, margin,
    evals, trials, cap, most, accepted) -- accepted: (rho, sums, fnew) of the trial that ended the loop."""
    o = dict(GCMMA_DEFAULTS, **opts)
    sp, gr = Subproblem.of_oracle(mma), groups_of_oracle(mma)
    xk = mma.x.copy()
    fk = fvals(mma.fobj, mma.cons)
    rho = rho_start(sp, [mma.g] + list(mma.A), mma.prob.nlocal, o["mma_gcmma_rho_init"], o["mma_gcmma_rho_min"])
    out = dict(sp=sp, gr=gr, xk=xk, fk=fk, rho0=rho.copy(), lam0=mma.z.copy(), raises=0, capped=False, margin=np.inf,
               evals=0, trials=0, cap=0, most=0)
    lam = mma.z.copy()
    while True:
        lam, status, evals, _, pt, most, cap = dual_solve_groups_rho(sp, xk, rho, lam, gr, dual_tol, max_evals)
        x = pt["x"]
        sums = point_sums(sp, xk, x)
        _, f, c = mma.prob.eval_obj_con(x)
        fnew = fvals(f, c)
        out["evals"] += evals
        out["trials"] += 1
        out["cap"] += cap
        out["most"] = max(out["most"], most)
        ok, viol, margin = acceptance(fnew, fk, sums, rho, o["mma_gcmma_tol"])
        out["margin"] = min(out["margin"], margin)
        if ok:
            break
        if out["raises"] == o["mma_gcmma_max_inner"]:
            out["capped"] = True
            break
        rho = raise_rho(rho, viol, sums[sp.m + 1])
        out["raises"] += 1
    zl, zu = bound_multipliers(sp, gr, pt)
    out.update(rho=rho, lam=lam, x=x, zw=pt["zw"].copy(), zl=zl, zu=zu, sums=sums, fnew=fnew, status=status)
    return out


def stop_test(mma):
    infeas, l1, linfty = mma.compute_kkt_error()  # (the driver's permuted names)
    o = mma.opt
    return infeas < o["mma_infeas_tol"] and (l1 < o["mma_l1_tol"] or linfty < o["mma_linfty_tol"])


def oracle_gcmma_groups(case, mma_options, opts, dual_tol, max_evals, niter, stop=True):
    """The oracle's MMA driven by the conservative inner loop on the grouped dual: (iterations, the oracle MMA,
    stopped)."""
    from oracle import mma_oracle as mo

    mma = mo.MMA(oracle_weighting_problem(case), mma_options)
    mma.initialize_subproblem(None)
    out, stopped = [], False
    for _ in range(niter):
        it = gcmma_group_iteration(mma, opts, dual_tol, max_evals)
        out.append(it)
        mma.zl, mma.zu, mma.z, mma.zw = it["zl"], it["zu"], it["lam"].copy(), it["zw"].copy()
        mma.subproblem_iter += it["evals"]
        mma.initialize_subproblem(it["x"])
        if stop and stop_test(mma):
            stopped = True
            break
    return out, mma, stopped


def quadratic_case(case):
    """The weighting golden's arguments with the problem kind swapped to `quadratic`."""
    return dict(case, args=dict(case["args"], problem="quadratic"))
