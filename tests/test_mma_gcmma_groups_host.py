"""CPU: the conservative variant with the grouped sparse constraints kept in the dual (mma_gcmma_sparse_constraints =
"groups"), as the numpy restatement of tests/mma_gcmma_group_helpers.py on oracle/mma_oracle.MMA.

  1. the rho form on (sp, xk, rho) is the plain grouped dual on the shifted subproblem p_i + rho_i w_U, q_i + rho_i w_L,
     b_i - rho_i n;
  2. with rho = 0 it is dual_eval_groups bit for bit;
  3. one conservative run on `quadratic` 200 x 2 with 40 groups of 5: every accepted trial is conservative when
     recomputed from plain arrays, and the run meets the stop test where plain MMA does not."""
import numpy as np

from conftest import load_golden
from mma_dual_group_helpers import WEIGHTING_GOLDEN, Groups, dual_eval_groups, element_roots, oracle_group_mma
from mma_dual_helpers import Subproblem
from mma_gcmma_group_helpers import (dual_eval_groups_rho, group_solve_rho, oracle_gcmma_groups, quadratic_case,
                                     shifted_subproblem)
from mma_gcmma_helpers import GCMMA_DEFAULTS, dfun
from mma_helpers import mma_options_from_case

EPS = np.finfo(np.float64).eps
# raises per MMA iteration of the conservative run on `quadratic` (printed by the run below; the first twelve are the
# constant of the lock-step test in tests/test_gpu_mma_gcmma_groups.py)
QUADRATIC_RAISES_12 = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 3]


def small_draw(seed, n=60, m=3):
    rng = np.random.default_rng(seed)
    x0 = 5.0 + rng.random(n)
    L, U = x0 - 3.0, x0 + 3.0
    sp = Subproblem(L, U, x0 - 0.8, x0 + 0.9, 0.2 * rng.random(n) + 0.01, 0.2 * rng.random(n) + 0.01,
                    0.01 * rng.random((m, n)), 0.01 * rng.random((m, n)), rng.standard_normal(m))
    xk = sp.alpha + (0.1 + 0.8 * rng.random(n)) * (sp.beta - sp.alpha)
    lam = np.array([0.0, 0.7, 2.0])
    free = group_solve_rho(sp, xk, np.zeros(m + 1), lam, Groups(0, 1, 0, 0, -1.0, [], 0))["x"]
    idx = 3 + np.arange(8)[:, None] * 6 + np.arange(4)[None, :]
    s0 = free[idx].sum(axis=1)
    # inactive, active, active, far beyond (at gamma), then equalities on both sides
    c = s0 + np.array([0.5, -0.3, -0.1, -4.0, 0.2, -0.2, 0.05, -0.05])
    return sp, xk, lam, Groups(8, 4, 3, 2, -1.0, c, 4, 2.0)


def test_the_rho_form_is_the_plain_grouped_dual_of_the_shifted_subproblem():
    for seed, rho in ((1, [1e-2, 1.0, 1e2, 1e3]), (2, [3e1, 1e-3, 1e-1, 5.0])):
        rho = np.array(rho)
        sp, xk, lam, gr = small_draw(seed)
        W, g, H, D, pt = dual_eval_groups_rho(sp, xk, rho, lam, gr)
        sh = shifted_subproblem(sp, xk, rho)
        Ws, gs, Hs, pts = dual_eval_groups(sh, lam, gr)
        assert pt["cap"] == 0 and pts["cap"] == 0
        assert set(np.sign(pt["zw"])) == {-1.0, 0.0, 1.0} and np.any(pt["zw"] == gr.gamma)
        # The shifted route carries sum rho_i (w_U u + w_L l) = rho_i (D + n) in its sums and takes rho_i n off again
        # through b: a cancellation of size rho_i n, so the two agree to rho_i n eps times a small integer (8) -- W with
        # sigma in place of rho_i -- on top of the rounding of the sums themselves, n eps times their largest term.
        sigma = rho[0] + float(np.dot(lam, rho[1:]))
        u, l = 1.0 / (sp.U - pt["x"]), 1.0 / (pt["x"] - sp.L)
        wterm = float(np.max(pt["P"] * u + pt["Q"] * l))
        tolW = 8 * sp.n * EPS * (sigma + wterm)
        tolg = 8 * sp.n * EPS * (rho[1:] + np.max(sp.p * u + sp.q * l, axis=1))
        errW, errg = abs((Ws - rho[0] * sp.n) - W), np.abs(gs - g)
        print("seed %d: W err %.2e (tol %.2e), grad err %s (tol %s), D %.3e" % (seed, errW, tolW, errg, tolg, D))
        assert errW <= tolW and np.all(errg <= tolg)
        # the points agree to the resolution of the root searches, the Hessians to what the cancelling form of the
        # shifted columns (rho_i w_U u^2 - rho_i w_L l^2 near xk) leaves: rho eps / |column| per element, far below 1e-9
        assert np.allclose(pt["x"], pts["x"], rtol=1e-12, atol=0) and np.allclose(pt["zw"], pts["zw"], rtol=1e-9)
        assert np.allclose(H, Hs, rtol=1e-9, atol=1e-9 * np.abs(H).max())


def test_with_rho_zero_it_is_the_plain_restatement_bit_for_bit():
    for seed in (1, 2):
        sp, xk, lam, gr = small_draw(seed)
        W0, g0, H0, pt0 = dual_eval_groups(sp, lam, gr)
        for roots in (None, element_roots):  # (the rho form's second stop does not act on this data)
            pt = group_solve_rho(sp, xk, np.zeros(sp.m + 1), lam, gr, **({"roots": roots} if roots else {}))
            W, g, H, D, _ = dual_eval_groups_rho(sp, xk, np.zeros(sp.m + 1), lam, gr, pt)
            assert np.array_equal(pt["x"], pt0["x"]) and np.array_equal(pt["zw"], pt0["zw"])
            assert np.array_equal(pt["steps"], pt0["steps"])
            assert W == W0 and np.array_equal(g, g0) and np.array_equal(H, H0)
            assert D == float(np.sum(dfun(sp, xk, pt0["x"])))


def stopped(t, o):
    """The stop test of the driver on a trace row (the driver's permuted names: infeas, l1, linfty <- l1, linfty, infeas)."""
    return t["l1"] < o["mma_infeas_tol"] and (t["linfty"] < o["mma_l1_tol"] or t["infeas"] < o["mma_linfty_tol"])


def test_conservative_run_on_quadratic_stops_where_plain_mma_does_not():
    from oracle.mma_oracle import MMA_DEFAULTS

    _, case = load_golden(WEIGHTING_GOLDEN)
    case = quadratic_case(case)
    _, mopts = mma_options_from_case(case)
    mopts = dict(mopts, mma_max_iterations=80)
    its, mma, met = oracle_gcmma_groups(case, mopts, {}, 1e-9, 200, 80)
    raises = [it["raises"] for it in its]
    print("conservative: %d iterations, stop test met %s, fobj %.8f" % (len(its), met, mma.fobj))
    print("raises per iteration:", raises)
    print("cap hits of the root searches:", sum(it["cap"] for it in its), "most steps of a group:",
          max(it["most"] for it in its))
    assert met and len(its) <= 80
    assert raises[:12] == QUADRATIC_RAISES_12
    assert all(it["status"] == 0 for it in its) and not any(it["capped"] for it in its)
    tol = GCMMA_DEFAULTS["mma_gcmma_tol"]
    for k, it in enumerate(its):  # gcmma_accept's inequality from plain arrays
        sp, xk, x, rho = it["sp"], it["xk"], it["x"], it["rho"]
        u, l, uk, lk = 1.0 / (sp.U - x), 1.0 / (x - sp.L), 1.0 / (sp.U - xk), 1.0 / (xk - sp.L)
        D = float(np.sum((x - xk) ** 2 * u * l))
        coef = [(sp.p0, sp.q0)] + [(sp.p[i], sp.q[i]) for i in range(sp.m)]
        for i, (p, q) in enumerate(coef):
            approx = it["fk"][i] + float(np.sum(p * u + q * l) - np.sum(p * uk + q * lk)) + rho[i] * D
            # (the differences above cancel against the sums: n eps times their size on top of the tolerance)
            slack = tol * max(1.0, abs(it["fnew"][i])) + 4 * sp.n * EPS * float(np.sum(p * uk + q * lk))
            assert it["fnew"][i] <= approx + slack or D == 0.0, (k, i, it["fnew"][i], approx)
        # the groups: exact, so feasible to the resolution of the searches without any rho
        psi = it["gr"].a * x[it["gr"].idx].sum(axis=1) + it["gr"].c
        assert np.all(psi >= -1e-12)
    o = dict(MMA_DEFAULTS, **mopts)
    trace, solves = oracle_group_mma(case, mopts, 1e-9, 200, 80)
    assert len(trace) == 81 and not any(stopped(t, o) for t in trace[1:])
    f = [t["fobj"] for t in trace]
    print("plain: not stopped after 80 iterations; fobj around iteration 10: %s" % f[8:13])
    assert max(f[k + 1] - f[k] for k in range(5, 15)) > 1.0  # it oscillates where the conservative run descends
    fc = [it["fnew"][0] for it in its]
    assert all(fc[k + 1] <= fc[k] + tol * max(1.0, abs(fc[k])) for k in range(len(fc) - 1))
