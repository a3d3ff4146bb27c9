"""numpy restatement of the MMA dual with grouped ("weighting") sparse constraints kept in it
(mma_dual_sparse_constraints = "groups"; paropt_amd/csrc/mma.hip, the group solve), on top of mma_dual_helpers.  Shared
by tests/test_mma_dual_groups_host.py and tests/test_gpu_mma_dual_groups.py.  Independent of the library.

Group i owns the variables start + i (nw + skip) + [0, nw); psi_i(x) = a sum x_j + c_i >= 0 (= 0 from group nwineq on)
with multiplier zw_i in [zlo_i, gamma], zlo_i = 0 (inequality) or -gamma (equality).  For a given lambda every group
is a root search in zw on top of root searches in x; both are safeguarded Newton iterations, vectorised over the
groups and over the elements."""
import numpy as np

from mma_dual_helpers import PENALTY_GAMMA, Subproblem, projected_gradient

NEWTON_CAP = 100
WEIGHTING_GOLDEN = "mma_convex_n200_c2_w40"


class Groups:
    def __init__(self, nwcon, nw, start, skip, a, c, nwineq, gamma=PENALTY_GAMMA):
        self.nwcon, self.nw, self.start, self.skip = int(nwcon), int(nw), int(start), int(skip)
        self.a, self.gamma, self.nwineq = float(a), float(gamma), int(nwineq)
        self.c = np.array(c, dtype=np.float64).reshape(self.nwcon)
        self.idx = (self.start + np.arange(self.nwcon)[:, None] * (self.nw + self.skip)
                    + np.arange(self.nw)[None, :]).astype(np.int64).reshape(self.nwcon, self.nw)
        self.zlo = np.where(np.arange(self.nwcon) < self.nwineq, 0.0, -self.gamma)


def form_pq(sp, lam):
    P, Q = sp.p0.copy(), sp.q0.copy()
    for i in range(sp.m):
        P = P + lam[i] * sp.p[i]
        Q = Q + lam[i] * sp.q[i]
    return P, Q


def closed_form(P, Q, L, U, alpha, beta):
    sP, sQ = np.sqrt(P), np.sqrt(Q)
    xs = (sP * L + sQ * U) / (sP + sQ)
    return np.minimum(np.maximum(xs, alpha), beta)


def phi1(P, Q, L, U, x):
    return P / (U - x) ** 2 - Q / (x - L) ** 2


def element_roots(P, Q, L, U, alpha, beta, t, x0):
    """clamp(root of phi'(x) = t, alpha, beta) for arrays of one shape: Newton inside the bracket, its midpoint when
    the step leaves it, until the iterate or the bracket stops moving.  t == 0: the closed form.  -> (x, cap hits)."""
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
        mid = 0.5 * (lo + hi)
        xn = np.where((xn > lo) & (xn < hi), xn, mid)
        stop = ~((xn > lo) & (xn < hi)) | (xn == x)
        x = np.where(act & ~stop, xn, x)
        act = act & ~stop
    return x, int(act.sum())


def group_solve(sp, lam, gr):
    """The point of lambda: dict with P, Q, x (n), zw, psi, s (sum of [free] / h per group), steps per group, cap."""
    P, Q = form_pq(sp, lam)
    x = closed_form(P, Q, sp.L, sp.U, sp.alpha, sp.beta)
    w = gr.nwcon
    out = dict(P=P, Q=Q, x=x, zw=np.zeros(w), psi=np.zeros(w), s=np.zeros(w), steps=np.zeros(w, dtype=int), cap=0)
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
        xa, c1 = element_roots(*[a[act] for a in e], t[act], xg[act])
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


def classes(gr, zw):
    """0: at the lower end, 1: strictly inside, 2: at gamma."""
    return np.where((zw > gr.zlo) & (zw < gr.gamma), 1, np.where(zw >= gr.gamma, 2, 0))


def dual_eval_groups(sp, lam, gr, pt=None):
    """W, grad W, -hess W and the point dict."""
    pt = pt or group_solve(sp, lam, gr)
    P, Q, x = pt["P"], pt["Q"], pt["x"]
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    W = float(np.sum(P * u + Q * l) - np.dot(pt["zw"], pt["psi"]) + np.dot(lam, sp.b))
    g = np.array([np.sum(sp.p[i] * u + sp.q[i] * l) for i in range(sp.m)]) + sp.b
    free = (x > sp.alpha) & (x < sp.beta)
    d = np.where(free, 1.0 / (2.0 * (P * u**3 + Q * l**3)), 0.0)
    G = sp.p * u**2 - sp.q * l**2
    H = (G * d) @ G.T
    if gr.nwcon:
        ag = (G * d)[:, gr.idx].sum(axis=2)  # (m, w)
        sg = d[gr.idx].sum(axis=1)
        wgt = np.where((classes(gr, pt["zw"]) == 1) & (sg > 0.0), 1.0 / np.where(sg > 0.0, sg, 1.0), 0.0)
        H = H - (ag * wgt) @ ag.T
    return W, g, H, pt


def bound_multipliers(sp, gr, pt):
    x = pt["x"]
    t = np.zeros(sp.n)
    if gr.nwcon:
        t[gr.idx] = (gr.a * pt["zw"])[:, None]
    r = phi1(pt["P"], pt["Q"], sp.L, sp.U, x) - t
    return np.where(x == sp.alpha, np.maximum(r, 0.0), 0.0), np.where(x == sp.beta, np.maximum(-r, 0.0), 0.0)


def dual_solve_groups(sp, lam0, gr, tol, max_evals):
    """The iteration of mma_dual_solve on the grouped dual: (lam, status, evaluations, max|pg|, point, most steps)."""
    gamma = np.full(sp.m, gr.gamma)
    lam = np.clip(np.asarray(lam0, dtype=np.float64), 0.0, gamma)
    W, g, H, pt = dual_eval_groups(sp, lam, gr)
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
        Wc, gc, Hc, ptc = dual_eval_groups(sp, cand, gr)
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


def oracle_weighting_problem(case):
    from oracle import paropt_oracle as po

    a = case["args"]
    return po.SepProblem(a["problem"], a["n"], a.get("c", 2), seed=a.get("seed", 0), nwcon=a["nwcon"], nw=a["nw"],
                         nwstart=a.get("nwstart", 0), nwskip=a.get("nwskip", 0), nwineq=a.get("nwineq", -1))


def groups_of_oracle(mma):
    """The linearised weighting constraints of the oracle's current subproblem (Jacobian entries -1)."""
    p = mma.prob
    g = Groups(p.nwcon, p.nw, p.nwstart, p.nwskip, -1.0, np.zeros(p.nwcon), p.nwineq)
    g.c = mma.cw - g.a * mma.x[g.idx].sum(axis=1)
    return g


def oracle_group_mma(case, mma_options, tol, max_evals, niter):
    """The oracle's MMA driven by dual_solve_groups: (rows [trace dicts], solves [(status, evals, most steps, cap)])."""
    from oracle import mma_oracle as mo

    mma = mo.MMA(oracle_weighting_problem(case), mma_options)
    mma.initialize_subproblem(None)
    solves = []
    for _ in range(niter):
        sp = Subproblem.of_oracle(mma)
        gr = groups_of_oracle(mma)
        lam, status, evals, pgmax, pt, most, cap = dual_solve_groups(sp, mma.z.copy(), gr, tol, max_evals)
        solves.append((status, evals, most, cap))
        mma.zl, mma.zu = bound_multipliers(sp, gr, pt)
        mma.z, mma.zw = lam.copy(), pt["zw"].copy()
        mma.subproblem_iter += evals
        mma.initialize_subproblem(pt["x"])
    return mma.trace, solves
