"""numpy restatement of the MMA subproblem's dual and of the solver on top of it (paropt_amd/csrc/mma_dual.cpp,
mma.hip), shared by tests/test_mma_dual_host.py and tests/test_gpu_mma_dual.py.  Independent of the library: it works
on plain arrays, e.g. those of oracle/mma_oracle.MMA.initialize_subproblem."""
import numpy as np

DUAL_GOLDENS = ("mma_quadratic_n200_c2", "mma_convex_n300_c3", "mma_rosenbrock_n60")
PENALTY_GAMMA = 1000.0  # the registry's default of penalty_gamma


class Subproblem:
    """L, U, alpha, beta, p0, q0: arrays of n; p, q: (m, n); b: m."""

    def __init__(self, L, U, alpha, beta, p0, q0, p, q, b):
        as_f = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
        self.L, self.U, self.alpha, self.beta, self.p0, self.q0 = (as_f(a) for a in (L, U, alpha, beta, p0, q0))
        self.n = self.L.size
        self.b = as_f(b)
        self.m = self.b.size
        self.p = as_f(p).reshape(self.m, self.n)
        self.q = as_f(q).reshape(self.m, self.n)

    @classmethod
    def of_oracle(cls, mma):
        return cls(mma.L, mma.U, mma.alpha, mma.beta, mma.p0, mma.q0, mma.pi, mma.qi, mma.b)


def primal_point(sp, lam):
    """(P, Q, unclamped x, x, free) at lam; P and Q accumulate in constraint order as the kernels do."""
    P, Q = sp.p0.copy(), sp.q0.copy()
    for i in range(sp.m):
        P = P + lam[i] * sp.p[i]
        Q = Q + lam[i] * sp.q[i]
    sP, sQ = np.sqrt(P), np.sqrt(Q)
    xs = (sP * sp.L + sQ * sp.U) / (sP + sQ)
    free = (xs > sp.alpha) & (xs < sp.beta)
    return P, Q, xs, np.minimum(np.maximum(xs, sp.alpha), sp.beta), free


def dual_eval(sp, lam):
    """W, grad W, -hess W."""
    P, Q, _, x, free = primal_point(sp, lam)
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    W = float(np.sum(P * u + Q * l) + np.dot(lam, sp.b))
    g = np.array([np.sum(sp.p[i] * u + sp.q[i] * l) for i in range(sp.m)]) + sp.b
    h = 2.0 * (P * u**3 + Q * l**3)
    G = sp.p * u**2 - sp.q * l**2
    H = (G[:, free] / h[free]) @ G[:, free].T
    return W, g, H


def dual_point(sp, lam):
    """x, zl, zu at lam."""
    P, Q, _, x, _ = primal_point(sp, lam)
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    r = P * u**2 - Q * l**2
    zl = np.where(x == sp.alpha, np.maximum(r, 0.0), 0.0)
    zu = np.where(x == sp.beta, np.maximum(-r, 0.0), 0.0)
    return x, zl, zu


def projected_gradient(lam, g, gamma):
    blocked = ((lam <= 0.0) & (g < 0.0)) | ((lam >= gamma) & (g > 0.0))
    return np.where(blocked, 0.0, g)


def dual_solve(sp, lam0, gamma, tol, max_evals):
    """The iteration of mma_dual_solve: (lam, status, evaluations, max|pg|)."""
    gamma = np.full(sp.m, gamma, dtype=np.float64) if np.isscalar(gamma) else np.asarray(gamma, dtype=np.float64)
    lam = np.clip(np.asarray(lam0, dtype=np.float64), 0.0, gamma)
    W, g, H = dual_eval(sp, lam)
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
        Wc, gc, Hc = dual_eval(sp, cand)
        evals += 1
        slope = float(np.dot(g, cand - lam))
        accept = Wc >= W + 1e-4 * slope
        if not accept and Wc >= W + 1e-4 * slope - 1e-13 * max(1.0, abs(W)):  # within the rounding error of W
            accept = float(np.max(np.abs(projected_gradient(cand, gc, gamma)))) < pgmax
        if accept:
            lam, W, g, H = cand, Wc, gc, Hc
            tau = max(tau / 8.0, 1e-14)
        else:
            tau *= 8.0


def oracle_problem(case):
    from oracle import paropt_oracle as po

    a = case["args"]
    return po.SepProblem(a["problem"], a["n"], a.get("c", 2), seed=a.get("seed", 0))


def oracle_dual_mma(case, mma_options, tol, max_evals, niter):
    """The oracle's MMA driven by dual_solve: the list of (Subproblem k, start multipliers, solution) for k < niter."""
    from oracle import mma_oracle as mo

    mma = mo.MMA(oracle_problem(case), mma_options)
    mma.initialize_subproblem(None)
    out = []
    for _ in range(niter):
        sp = Subproblem.of_oracle(mma)
        lam0 = mma.z.copy()
        lam, status, evals, pgmax = dual_solve(sp, lam0, PENALTY_GAMMA, tol, max_evals)
        out.append((sp, lam0, lam, status, evals))
        x, mma.zl, mma.zu = dual_point(sp, lam)
        mma.z = lam.copy()
        mma.initialize_subproblem(x)
    return out
