"""numpy restatement of the dual of the MMA subproblem with linearised constraints and of the box solver on top of it
(paropt_amd/csrc/mma_dual.cpp, mma.hip), shared by tests/test_mma_dual_linear_host.py and
tests/test_gpu_mma_dual_linear.py.  Independent of the library: it works on plain arrays.

  minimise sum p0 / (U - x) + q0 / (x - L) over alpha <= x <= beta
  subject to c_i(x) = cons_i + sum_j A_ij (x_j - xk_j) >= 0 (the first m - neq rows), = 0 (the last neq rows)

With t = sum_i lambda_i A_i the element-wise minimiser of the Lagrangian is the root of the increasing function
p0 u^2 - q0 l^2 = t (u = 1 / (U - x), l = 1 / (x - L)) clamped into [alpha, beta]; it is found here by bisection down
to a bracket that no longer moves.  W = sum (p0 u + q0 l) - lambda . c(x), dW/dlambda = -c(x), -hess W = sum over the
free elements (root strictly inside (alpha, beta)) of A_i A_k / h, h = 2 (p0 u^3 + q0 l^3)."""
import numpy as np

LINEAR_GOLDENS = ("mma_convex_n200_c2_linearized", "mma_quadratic_n200_c2", "mma_convex_n300_c3")
PENALTY_GAMMA = 1000.0  # the registry's default of penalty_gamma


class LinearSubproblem:
    """L, U, alpha, beta, p0, q0, xk: arrays of n; A: (m, n); cons: m; neq: the last neq rows are equalities."""

    def __init__(self, L, U, alpha, beta, p0, q0, A, cons, xk, neq=0):
        as_f = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
        self.L, self.U, self.alpha, self.beta, self.p0, self.q0, self.xk = (
            as_f(a) for a in (L, U, alpha, beta, p0, q0, xk))
        self.n = self.L.size
        self.cons = as_f(cons).reshape(-1)
        self.m = self.cons.size
        self.A = as_f(A).reshape(self.m, self.n)
        self.neq = int(neq)

    @classmethod
    def of_oracle(cls, mma, neq=0):
        return cls(mma.L, mma.U, mma.alpha, mma.beta, mma.p0, mma.q0, mma.A, mma.cons, mma.x, neq)

    def box(self, gamma):
        lower = np.zeros(self.m)
        if self.neq:
            lower[self.m - self.neq:] = -gamma
        return lower, np.full(self.m, float(gamma))


def multiplier_term(sp, lam):
    """t = sum_i lambda_i A_i, accumulated in constraint order as the kernels do."""
    t = np.zeros(sp.n)
    for i in range(sp.m):
        t = t + lam[i] * sp.A[i]
    return t


def phi1(sp, x):
    """p0 u^2 - q0 l^2, the derivative of the objective's approximation."""
    return sp.p0 / (sp.U - x) ** 2 - sp.q0 / (x - sp.L) ** 2


def element_roots(sp, t):
    """(x, free): clamp(root of phi1(x) = t, alpha, beta) by bisection to a stationary bracket."""
    fa, fb = phi1(sp, sp.alpha) - t, phi1(sp, sp.beta) - t
    free = (fa < 0.0) & (fb > 0.0)
    lo, hi = sp.alpha.copy(), sp.beta.copy()
    for _ in range(2200):  # (a bracket of doubles halves at most about 2100 times)
        mid = 0.5 * (lo + hi)
        move = free & (mid > lo) & (mid < hi)
        if not move.any():
            break
        fm = phi1(sp, mid) - t
        lo = np.where(move & (fm < 0.0), mid, lo)
        hi = np.where(move & ~(fm < 0.0), mid, hi)
    else:
        raise AssertionError("the bisection did not end")
    # of the two ends of the last bracket, the one with the smaller residual
    pick_hi = np.abs(phi1(sp, hi) - t) < np.abs(phi1(sp, lo) - t)
    x = np.where(pick_hi, hi, lo)
    x = np.where(free, x, np.where(fa >= 0.0, sp.alpha, sp.beta))
    free = free & (x > sp.alpha) & (x < sp.beta)
    return x, free


def sums_at(sp, lam, x, free):
    """W, grad W, -hess W with the primal point given."""
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    c = sp.cons + np.array([np.sum(sp.A[i] * (x - sp.xk)) for i in range(sp.m)])
    W = float(np.sum(sp.p0 * u + sp.q0 * l) - np.dot(lam, c))
    h = 2.0 * (sp.p0 * u**3 + sp.q0 * l**3)
    Af = sp.A[:, free]
    H = (Af / h[free]) @ Af.T
    return W, -c, H


def linear_eval(sp, lam):
    """W, grad W, -hess W at lam."""
    x, free = element_roots(sp, multiplier_term(sp, lam))
    return sums_at(sp, lam, x, free)


def bound_multipliers(sp, lam, x):
    """zl, zu at the point x: r = p0 u^2 - q0 l^2 - t, zl = max(r, 0) where x = alpha, zu = max(-r, 0) where x = beta."""
    r = phi1(sp, x) - multiplier_term(sp, lam)
    zl = np.where(x == sp.alpha, np.maximum(r, 0.0), 0.0)
    zu = np.where(x == sp.beta, np.maximum(-r, 0.0), 0.0)
    return zl, zu


def linear_point(sp, lam):
    """x, zl, zu at lam."""
    x, _ = element_roots(sp, multiplier_term(sp, lam))
    zl, zu = bound_multipliers(sp, lam, x)
    return x, zl, zu


def projected_gradient(lam, g, lower, upper):
    blocked = ((lam <= lower) & (g < 0.0)) | ((lam >= upper) & (g > 0.0))
    return np.where(blocked, 0.0, g)


def linear_dual_solve(sp, lam0, gamma, tol, max_evals):
    """The iteration of mma_dual_solve over the box of sp: (lam, status, evaluations, max|pg|)."""
    lower, upper = sp.box(gamma)
    lam = np.clip(np.asarray(lam0, dtype=np.float64), lower, upper)
    W, g, H = linear_eval(sp, lam)
    evals = 1
    tau = 1e-8 * max(1.0, float(np.trace(H)))
    while True:
        pg = projected_gradient(lam, g, lower, upper)
        pgmax = float(np.max(np.abs(pg))) if sp.m else 0.0
        if pgmax <= tol:
            return lam, 0, evals, pgmax
        if evals >= max_evals or not tau <= 1e30:
            return lam, 1, evals, pgmax
        F = np.nonzero(pg != 0.0)[0]
        d = np.zeros(sp.m)
        d[F] = np.linalg.solve(H[np.ix_(F, F)] + tau * np.eye(F.size), g[F])
        cand = np.clip(lam + d, lower, upper)
        cand[pg == 0.0] = lam[pg == 0.0]
        Wc, gc, Hc = linear_eval(sp, cand)
        evals += 1
        slope = float(np.dot(g, cand - lam))
        accept = Wc >= W + 1e-4 * slope
        if not accept and Wc >= W + 1e-4 * slope - 1e-13 * max(1.0, abs(W)):  # within the rounding error of W
            accept = float(np.max(np.abs(projected_gradient(cand, gc, lower, upper)))) < pgmax
        if accept:
            lam, W, g, H = cand, Wc, gc, Hc
            tau = max(tau / 8.0, 1e-14)
        else:
            tau *= 8.0


def oracle_linear_dual_mma(case, mma_options, tol, max_evals, niter, neq=0):
    """The oracle's MMA with linearised constraints (use_true_mma = 0) driven by linear_dual_solve, the last neq
    constraints taken as equalities: the list of (LinearSubproblem k, start multipliers, solution, status,
    evaluations) for k < niter."""
    from mma_dual_helpers import oracle_problem
    from oracle import mma_oracle as mo

    opts = dict(mma_options, mma_use_constraint_linearization=1)
    mma = mo.MMA(oracle_problem(case), opts)
    mma.use_true_mma = 0
    mma.initialize_subproblem(None)
    out = []
    for _ in range(niter):
        sp = LinearSubproblem.of_oracle(mma, neq)
        lam0 = mma.z.copy()
        lam, status, evals, pgmax = linear_dual_solve(sp, lam0, PENALTY_GAMMA, tol, max_evals)
        out.append((sp, lam0, lam, status, evals))
        x, mma.zl, mma.zu = linear_point(sp, lam)
        mma.z = lam.copy()
        mma.initialize_subproblem(x)
    return out


def residual_bound(sp, lam, x):
    """The bound of the element residual |p0 u^2 - q0 l^2 - t| at a computed root: four spacings of the variable's
    scale through the slope h, and the rounding of the m + 2 terms of the residual itself."""
    eps = np.finfo(np.float64).eps
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    h = 2.0 * (sp.p0 * u**3 + sp.q0 * l**3)
    mag = sp.p0 * u**2 + sp.q0 * l**2 + np.sum(np.abs(np.asarray(lam)[:, None] * sp.A), axis=0)
    return 4.0 * h * np.spacing(np.maximum(np.abs(sp.L), np.abs(sp.U))) + 16.0 * (sp.m + 2) * eps * mag


def residual_longdouble(sp, lam, x):
    """r = p0 u^2 - q0 l^2 - t at x, evaluated in longdouble."""
    ld = np.longdouble
    xl = x.astype(ld)
    t = np.zeros(sp.n, dtype=ld)
    for i in range(sp.m):
        t = t + ld(lam[i]) * sp.A[i].astype(ld)
    r = sp.p0.astype(ld) / (sp.U.astype(ld) - xl) ** 2 - sp.q0.astype(ld) / (xl - sp.L.astype(ld)) ** 2 - t
    return r.astype(np.float64)
