"""numpy restatement of the globally convergent MMA (mma_globalization = "conservative": Svanberg 2002 / 2007 in the
coefficient form of paropt_amd/csrc/mma.cpp, mma_gcmma.cpp), on top of tests/mma_dual_helpers.py and
oracle/mma_oracle.py.  Independent of the library: plain arrays only.

With w_U = (U - xk)^2 / (U - L), w_L = (xk - L)^2 / (U - L), u = 1 / (U - x), l = 1 / (x - L):
    d(x) = sum (x - xk)^2 u l  (= sum w_U u + w_L l - 1),   f~_i^rho = f~_i + rho_i d,  i = 0..m
and the dual of the subproblem in these functions is the dual of mma_dual_helpers with
    P = p0 + sum lam_i p_i + sigma w_U,  Q likewise,  sigma = rho_0 + lam . rho[1:]."""
import numpy as np

from mma_dual_helpers import PENALTY_GAMMA, Subproblem, oracle_problem, projected_gradient

GCMMA_GOLDENS = ("mma_quadratic_n200_c2", "mma_rosenbrock_n60")
GCMMA_DEFAULTS = dict(mma_gcmma_rho_init=0.1, mma_gcmma_rho_min=1e-6, mma_gcmma_tol=1e-7, mma_gcmma_max_inner=15)


def weights(sp, xk):
    r = 1.0 / (sp.U - sp.L)
    return (sp.U - xk) ** 2 * r, (xk - sp.L) ** 2 * r


def primal_point_rho(sp, xk, rho, lam):
    """(P0, Q0, P, Q, unclamped x, x, free): P0, Q0 without the sigma term, which is added last."""
    P0, Q0 = sp.p0.copy(), sp.q0.copy()
    for i in range(sp.m):
        P0 = P0 + lam[i] * sp.p[i]
        Q0 = Q0 + lam[i] * sp.q[i]
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    wU, wL = weights(sp, xk)
    P, Q = P0 + sigma * wU, Q0 + sigma * wL
    sP, sQ = np.sqrt(P), np.sqrt(Q)
    xs = (sP * sp.L + sQ * sp.U) / (sP + sQ)
    free = (xs > sp.alpha) & (xs < sp.beta)
    return P0, Q0, P, Q, xs, np.minimum(np.maximum(xs, sp.alpha), sp.beta), free


def dfun(sp, xk, x):
    """The terms of d(x): non-negative, no cancellation."""
    return (x - xk) ** 2 / ((sp.U - x) * (x - sp.L))


def dprime(sp, xk, x):
    """The derivative of d, w_U u^2 - w_L l^2, in the form that does not cancel near xk (where it vanishes): with
    a = (U - xk) u = 1 + (x - xk) u and b = (xk - L) l = 1 - (x - xk) l it is (a - b)(a + b) / (U - L)."""
    u, l, dx = 1.0 / (sp.U - x), 1.0 / (x - sp.L), x - xk
    return dx * (u + l) * (2.0 + dx * (u - l)) / (sp.U - sp.L)


def dual_eval_rho(sp, xk, rho, lam):
    """W, grad W, -hess W, D of the rho form."""
    P0, Q0, P, Q, _, x, free = primal_point_rho(sp, xk, rho, lam)
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    D = float(np.sum(dfun(sp, xk, x)))
    sigma = rho[0] + float(np.dot(lam, rho[1:]))
    W = float(np.sum(P0 * u + Q0 * l)) + sigma * D + float(np.dot(lam, sp.b))
    g = np.array([np.sum(sp.p[i] * u + sp.q[i] * l) for i in range(sp.m)]) + rho[1:] * D + sp.b
    h = 2.0 * (P * u**3 + Q * l**3)
    G = sp.p * u**2 - sp.q * l**2 + np.outer(rho[1:], dprime(sp, xk, x))
    H = (G[:, free] / h[free]) @ G[:, free].T
    return W, g, H, D


def point_rho(sp, xk, rho, lam):
    """The point pass: x, zl, zu and the m + 2 sums [Delta_0, Delta_1..m, D]; Delta_i = f~_i(x) - f~_i(xk)."""
    _, _, P, Q, _, x, _ = primal_point_rho(sp, xk, rho, lam)
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    uk, lk = 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
    du, dl = (x - xk) * u * uk, -(x - xk) * l * lk  # u - uk, l - lk
    r = P * u**2 - Q * l**2
    zl = np.where(x == sp.alpha, np.maximum(r, 0.0), 0.0)
    zu = np.where(x == sp.beta, np.maximum(-r, 0.0), 0.0)
    sums = np.zeros(sp.m + 2)
    sums[0] = np.sum(sp.p0 * du + sp.q0 * dl)
    for i in range(sp.m):
        sums[1 + i] = np.sum(sp.p[i] * du + sp.q[i] * dl)
    sums[sp.m + 1] = np.sum(dfun(sp, xk, x))
    return x, zl, zu, sums


def dual_solve_rho(sp, xk, rho, lam0, gamma, tol, max_evals):
    """The iteration of mma_dual_helpers.dual_solve on the rho form: (lam, status, evaluations, max|pg|)."""
    gamma = np.full(sp.m, gamma, dtype=np.float64)
    lam = np.clip(np.asarray(lam0, dtype=np.float64), 0.0, gamma)
    W, g, H, _ = dual_eval_rho(sp, xk, rho, lam)
    evals = 1
    tau = 1e-8 * max(1.0, float(np.trace(H)))
    while True:
        pg = projected_gradient(lam, g, gamma)
        pgmax = float(np.max(np.abs(pg))) if sp.m else 0.0
        if pgmax <= tol:
            return lam, 0, evals, pgmax
        if evals >= max_evals or not tau <= 1e30:
            return lam, 1, evals, pgmax
        F = np.nonzero(pg != 0.0)[0]
        d = np.zeros(sp.m)
        d[F] = np.linalg.solve(H[np.ix_(F, F)] + tau * np.eye(F.size), g[F])
        cand = np.clip(lam + d, 0.0, gamma)
        cand[pg == 0.0] = lam[pg == 0.0]
        Wc, gc, Hc, _ = dual_eval_rho(sp, xk, rho, cand)
        evals += 1
        slope = float(np.dot(g, cand - lam))
        accept = Wc >= W + 1e-4 * slope
        if not accept and Wc >= W + 1e-4 * slope - 1e-13 * max(1.0, abs(W)):
            accept = float(np.max(np.abs(projected_gradient(cand, gc, gamma)))) < pgmax
        if accept:
            lam, W, g, H = cand, Wc, gc, Hc
            tau = max(tau / 8.0, 1e-14)
        else:
            tau *= 8.0


def rho_start(sp, grads, n_global, rho_init, rho_min):
    """rho_i = max(rho_init / n * sum |df_i/dx_j| (U_j - L_j), rho_min); grads: the objective gradient and the m
    Jacobian columns."""
    w = sp.U - sp.L
    return np.array([max(rho_init / n_global * float(np.sum(np.abs(g) * w)), rho_min) for g in grads])


def acceptance(fnew, fk, sums, rho, tol):
    """(accepted, violations without the tolerance, smallest relative distance of a decision from its threshold).
    fnew, fk: [f_0, g_1..g_m] with g_i = -c_i at the candidate and at the expansion point."""
    m = len(fk) - 1
    D = sums[m + 1]
    bound = fk + sums[: m + 1] + rho * D
    viol = fnew - bound
    slack = tol * np.maximum(1.0, np.abs(fnew))
    margin = float(np.min(np.abs(viol - slack) / np.maximum(1.0, np.abs(fnew))))
    return bool(np.all(viol <= slack)) or D == 0.0, viol, margin


def raise_rho(rho, viol, D):
    delta = viol / D
    return np.where(delta > 0.0, np.minimum(1.1 * (rho + delta), 10.0 * rho), rho)


def fvals(fobj, cons):
    return np.concatenate(([fobj], -np.asarray(cons, dtype=np.float64)))


def gcmma_iteration(mma, opts, dual_tol, max_evals, evaluate=None):
    """One MMA iteration of the conservative variant on the oracle's MMA object `mma` (its current subproblem):
    returns dict(sp, xk, fk, rho0, rho, lam0, lam, x, zl, zu, raises, capped, margin, evals, trials).  evaluate(x) ->
    (fobj, cons) defaults to the oracle problem's own functions."""
    o = dict(GCMMA_DEFAULTS, **opts)
    sp = Subproblem.of_oracle(mma)
    xk = mma.x.copy()
    fk = fvals(mma.fobj, mma.cons)
    if evaluate is None:
        def evaluate(x):
            _, f, c = mma.prob.eval_obj_con(x)
            return f, c
    rho = rho_start(sp, [mma.g] + list(mma.A), mma.prob.nlocal, o["mma_gcmma_rho_init"], o["mma_gcmma_rho_min"])
    out = dict(sp=sp, xk=xk, fk=fk, rho0=rho.copy(), lam0=mma.z.copy(), raises=0, capped=False, margin=np.inf,
               evals=0, trials=0)
    lam = mma.z.copy()
    while True:
        lam, status, evals, _ = dual_solve_rho(sp, xk, rho, lam, PENALTY_GAMMA, dual_tol, max_evals)
        x, zl, zu, sums = point_rho(sp, xk, rho, lam)
        f, c = evaluate(x)
        fnew = fvals(f, c)
        out["evals"] += evals
        out["trials"] += 1
        ok, viol, margin = acceptance(fnew, fk, sums, rho, o["mma_gcmma_tol"])
        out["margin"] = min(out["margin"], margin)
        if ok:
            break
        if out["raises"] == o["mma_gcmma_max_inner"]:
            out["capped"] = True
            break
        rho = raise_rho(rho, viol, sums[sp.m + 1])
        out["raises"] += 1
    out.update(rho=rho, lam=lam, x=x, zl=zl, zu=zu, sums=sums, fnew=fnew)
    return out


def oracle_gcmma(case, mma_options, opts, dual_tol, max_evals, niter, stop=False):
    """The oracle's MMA driven by the conservative inner loop: (list of gcmma_iteration results, the oracle MMA)."""
    from oracle import mma_oracle as mo

    mma = mo.MMA(oracle_problem(case), mma_options)
    mma.initialize_subproblem(None)
    out = []
    for _ in range(niter):
        it = gcmma_iteration(mma, opts, dual_tol, max_evals)
        out.append(it)
        mma.zl, mma.zu, mma.z = it["zl"], it["zu"], it["lam"].copy()
        mma.initialize_subproblem(it["x"])
        if stop:
            infeas, l1, linfty = mma.compute_kkt_error()  # (the driver's permuted names)
            o = mma.opt
            if infeas < o["mma_infeas_tol"] and (l1 < o["mma_l1_tol"] or linfty < o["mma_linfty_tol"]):
                break
    return out, mma
