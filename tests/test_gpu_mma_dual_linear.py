"""
GPU: the dual sub-solver of the method of moving asymptotes on linearised constraints
(mma_subproblem_solver = "dual", mma_use_constraint_linearization = 1, mma_dual_linearized_constraints = "newton").

  1. the kernels (po_mma_dual_linear_eval) against numpy at the device's stored point, both forms, every size class;
  2. optimality of the solved subproblems, checked in numpy on the downloaded data (a dense equality included);
  3. whole runs against the unchanged interior-point path, measured by that path's own sensitivity to its tolerance;
  4. the interfaces: refusals, the registry, the vector count, the ParOpt.Optimizer facade;
  5. two ranks on one GPU.
"""
import gc
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from mma_dual_linear_helpers import (PENALTY_GAMMA, LinearSubproblem, bound_multipliers, projected_gradient,
                                     residual_bound, residual_longdouble)
from mma_helpers import mma_options_from_case, parse_mma_table
from mma_test_util import accurate_sum, run_two_ranks
from test_gpu_mma_dual import draw_subproblem, make_problem

pytestmark = pytest.mark.gpu

M_F = 8  # widest fused form
EPS = np.finfo(np.float64).eps
GOLDEN = "mma_convex_n200_c2_linearized"
LINEAR = {"mma_subproblem_solver": "dual", "mma_use_constraint_linearization": 1,
          "mma_dual_linearized_constraints": "newton"}


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


# ---- 1. kernels against numpy ---------------------------------------------------------------------------------------
def draw_linear(n, m, seed):
    """L, U, alpha, beta, p0, q0 and x0 of draw_subproblem (test_gpu_mma_dual.py); A = (0.08 / sqrt m) N(0, 1) with half
    the entries exactly 0; lambda = 2 rand with every third entry 0 and every third 2; the last m // 2 rows are
    equalities and their multipliers get a random sign."""
    rat, _ = draw_subproblem(n, m, seed)
    x0 = 5.0 + np.random.default_rng(seed).random(n)  # (the first draw of draw_subproblem)
    rng = np.random.default_rng([seed, 1])
    A = (0.08 / np.sqrt(m)) * rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.5)
    lam = 2.0 * rng.random(m)
    lam[0::3] = 0.0
    lam[1::3] = 2.0
    neq = m // 2
    if neq:
        lam[m - neq:] *= np.where(rng.random(neq) < 0.5, -1.0, 1.0)
    cons = rng.standard_normal(m)
    assert np.all(rat.alpha < x0) and np.all(x0 < rat.beta)
    return LinearSubproblem(rat.L, rat.U, rat.alpha, rat.beta, rat.p0, rat.q0, A, cons, x0, neq), lam


_UPLOADS = {}


def uploaded(ctx, n, m, seed):
    """One draw and one upload per shape, shared by the forms and left unchanged."""
    import paropt_amd as pa

    key = (n, m, seed)
    if key not in _UPLOADS:
        _UPLOADS.clear()  # (one shape's vectors at a time)
        sp, lam = draw_linear(n, m, seed)
        up = lambda a: pa.PVec(ctx, n).from_numpy(a)  # noqa: E731
        dev = dict(L=up(sp.L), U=up(sp.U), alpha=up(sp.alpha), beta=up(sp.beta), p0=up(sp.p0), q0=up(sp.q0),
                   xk=up(sp.xk), A=[up(sp.A[i]) for i in range(m)])
        _UPLOADS[key] = (sp, lam, dev)
    return _UPLOADS[key]


def run_eval(ctx, dev, sp, lam, form, start, point=False):
    """One evaluation from the start values `start`: (W, g, H, stats, x of the evaluation, point or None)."""
    import paropt_amd as pa

    xs = pa.PVec(ctx, sp.n).from_numpy(start)
    pt = [pa.PVec(ctx, sp.n) for _ in range(3)] if point else None
    W, g, H, st = pa.mma_dual_linear_eval(ctx, dev["L"], dev["U"], dev["alpha"], dev["beta"], dev["p0"], dev["q0"],
                                          dev["A"], sp.cons, dev["xk"], lam, xs, form=form, point=pt)
    return W, g, H, st, xs.to_numpy(), ([v.to_numpy() for v in pt] if point else None)


def check_point(sp, lam, x, what):
    """x in [alpha, beta]; the element residual under its bound on the free elements, one-sided on the clamped ones."""
    assert np.all(x >= sp.alpha) and np.all(x <= sp.beta), what
    r, bound = residual_longdouble(sp, lam, x), residual_bound(sp, lam, x)
    low, upp = x == sp.alpha, x == sp.beta
    free = ~low & ~upp
    worst = max(float((np.abs(r) / bound)[free].max()) if free.any() else 0.0,
                float((-r / bound)[low].max()) if low.any() else 0.0,
                float((r / bound)[upp].max()) if upp.any() else 0.0)
    print("   %s: %d free, %d at alpha, %d at beta, worst residual / bound = %.3f" % (
        what, free.sum(), low.sum(), upp.sum(), worst))
    assert np.all(np.abs(r[free]) <= bound[free]), what
    assert np.all(r[low] >= -bound[low]) and np.all(r[upp] <= bound[upp]), what
    return free, low, upp


def reference_sums(sp, lam, x, free):
    """W, g, H by accurate sums over the point x, and the largest term of each."""
    u, l = 1.0 / (sp.U - x), 1.0 / (x - sp.L)
    wterms = sp.p0 * u + sp.q0 * l
    cterms = sp.A * (x - sp.xk)
    c = sp.cons + accurate_sum(cterms)
    cmax = np.abs(cterms).max(axis=1)
    ref = dict(W=float(accurate_sum(wterms)) - float(np.dot(lam, c)),
               Wmax=float(np.abs(wterms).max() + np.dot(np.abs(lam), cmax)), g=-c, gmax=cmax)
    m = sp.m
    Af, h = sp.A[:, free], (2.0 * (sp.p0 * u**3 + sp.q0 * l**3))[free]
    H, Hmax = np.zeros((m, m)), np.zeros((m, m))
    for k in range(m):
        t = Af[: k + 1] * (Af[k] / h)
        H[k, : k + 1] = H[: k + 1, k] = accurate_sum(t) if t.shape[1] else 0.0
        Hmax[k, : k + 1] = Hmax[: k + 1, k] = np.abs(t).max(axis=1) if t.shape[1] else 0.0
    ref["H"], ref["Hmax"] = H, Hmax
    return ref


@pytest.mark.parametrize("m", [1, 3, M_F, M_F + 1, 33])
@pytest.mark.parametrize("n", [1, 2, 511, 513, 4097, 393217])
def test_linear_dual_kernels_against_numpy(ctx, n, m):
    sp, lam, dev = uploaded(ctx, n, m, seed=1000 * m + n % 997)
    forms = [1, 2] if m <= M_F else [2]
    res = {}
    for form in forms:
        first = form == forms[0]
        W, g, H, st, x, pt = run_eval(ctx, dev, sp, lam, form, sp.xk, point=first)
        res[form] = (W, g, H, x)
        assert st["cap_hits"] == 0, st
        free, low, upp = check_point(sp, lam, x, "n=%d m=%d form %d" % (n, m, form))
        if n >= 511:  # every branch of the element search is taken
            assert free.sum() > n // 20 and low.sum() > n // 20 and upp.sum() > n // 20
        ref = reference_sums(sp, lam, x, free)
        errW, errg, errH = abs(W - ref["W"]), np.abs(g - ref["g"]), np.abs(H - ref["H"])
        print("n=%d m=%d form %d: |dW| %.2e (bound %.2e)  max|dg|/bound %.2e  max|dH|/bound %.2e  steps %d" % (
            n, m, form, errW, 1e-13 * n * ref["Wmax"], (errg / np.maximum(1e-13 * n * ref["gmax"], 1e-300)).max(),
            (errH / np.maximum(1e-13 * n * ref["Hmax"], 1e-300)).max(), st["max_steps"]))
        assert errW <= 1e-13 * n * ref["Wmax"]
        assert np.all(errg <= 1e-13 * n * ref["gmax"])
        assert np.all(errH <= 1e-13 * n * ref["Hmax"])
        assert np.array_equal(H, H.T)
        if pt is not None:  # the point pass, started from the evaluation's x: its own x, and zl, zu at that x
            xp, zl, zu = pt
            check_point(sp, lam, xp, "point pass")
            wl, wu = bound_multipliers(sp, lam, xp)
            bound = 4 * EPS * np.maximum(np.abs(sp.L), np.abs(sp.U))
            for name, got, want in (("zl", zl, wl), ("zu", zu, wu)):
                err = np.abs(got - want)
                print("   %s: max err / (4 ulp of max(|L|, |U|)) = %.3f" % (name, (err / bound).max()))
                assert np.all(err <= bound), name
        # the same form again from the same start: identical bits
        W2, g2, H2, st2, x2, _ = run_eval(ctx, dev, sp, lam, form, sp.xk)
        assert W2 == W and np.array_equal(g2, g) and np.array_equal(H2, H) and np.array_equal(x2, x)
    if len(forms) == 2:  # same pass, same order: the value, the gradient and the point do not depend on the form
        assert res[1][0] == res[2][0] and np.array_equal(res[1][1], res[2][1]) and np.array_equal(res[1][3], res[2][3])
        assert np.all(np.abs(res[1][2] - res[2][2]) <= 1e-13 * n * np.linalg.norm(res[1][2]))
    # starts outside (alpha, beta) and an all-zero start: the search restarts from the midpoint and ends at the same
    # root within the residual bound (two roots under the bound lie within 2 bound / h of each other)
    x_ref = res[forms[0]][3]
    u, l = 1.0 / (sp.U - x_ref), 1.0 / (x_ref - sp.L)
    dx_bound = 2.0 * residual_bound(sp, lam, x_ref) / (2.0 * (sp.p0 * u**3 + sp.q0 * l**3))
    for what, start in (("start outside", sp.U + 1.0), ("zero start", np.zeros(n))):
        _, _, _, st, x, _ = run_eval(ctx, dev, sp, lam, 0, start)
        assert st["cap_hits"] == 0, (what, st)
        check_point(sp, lam, x, what)
        clamped = (x_ref == sp.alpha) | (x_ref == sp.beta)
        assert np.array_equal(x[clamped], x_ref[clamped]), what
        assert np.all(np.abs(x - x_ref) <= 1.01 * dx_bound + 2.0 * np.spacing(np.abs(x_ref))), what


def test_roots_far_below_the_asymptotes_end_without_the_cap(ctx):
    """Variables around zero between asymptotes of order one: a Newton step of an ulp of x is below the resolution of
    U - x and x - L, the residual keeps its rounding residue and a search that only watches x creeps into its step cap.
    The search also ends when a step changes neither difference: no cap hit, the same residual bound."""
    import paropt_amd as pa

    n, m = 4097, 3
    sp, lam = draw_linear(n, m, seed=77)
    shift = sp.xk * (1.0 - 1e-3 * np.random.default_rng(78).random(n))  # x^k lands in (0, 1e-3 x^k)
    sp = LinearSubproblem(sp.L - shift, sp.U - shift, sp.alpha - shift, sp.beta - shift, sp.p0, sp.q0, sp.A, sp.cons,
                          sp.xk - shift, sp.neq)
    up = lambda a: pa.PVec(ctx, n).from_numpy(a)  # noqa: E731
    dev = dict(L=up(sp.L), U=up(sp.U), alpha=up(sp.alpha), beta=up(sp.beta), p0=up(sp.p0), q0=up(sp.q0), xk=up(sp.xk),
               A=[up(sp.A[i]) for i in range(m)])
    for what, start in (("from x^k", sp.xk), ("zero start", np.zeros(n))):
        W, g, H, st, x, _ = run_eval(ctx, dev, sp, lam, 1, start)
        print("   %s: most evaluations of one search %d" % (what, st["max_steps"]))
        assert st["cap_hits"] == 0, (what, st)
        free, low, upp = check_point(sp, lam, x, what)
        assert free.sum() > n // 20 and low.sum() > n // 20 and upp.sum() > n // 20


def test_fused_form_is_refused_beyond_its_width(ctx):
    import paropt_amd as pa

    sp, lam, dev = uploaded(ctx, 64, M_F + 1, seed=5)
    with pytest.raises(pa.ParOptAMDError) as e:
        run_eval(ctx, dev, sp, lam, 1, sp.xk)
    assert e.value.code == 2


# ---- the two problems of the whole runs -----------------------------------------------------------------------------
EQ_N, EQ_TOTAL = 64, 24.0


def equality_problem(ctx):
    """n = 64, two dense constraints, the first an inequality: minimise the convex separable sum w (x - a)^2 + 0.1 x^4
    subject to 14 - sum x^2 >= 0 and sum x - 24 = 0, -1 <= x <= 2."""
    import paropt_amd as pa

    j = np.arange(EQ_N)
    w, a = 1.0 + 2.0 * ((7 * j) % 11) / 10.0, ((5 * j) % 13) / 12.0

    class Equality(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, -1.0, 2.0

        def evalObjCon(self, x):
            f = float(np.sum(w * (x - a) ** 2 + 0.1 * x**4))
            return 0, f, np.array([14.0 - np.sum(x * x), np.sum(x) - EQ_TOTAL])

        def evalObjConGradient(self, x, g, A):
            g[:] = 2.0 * w * (x - a) + 0.4 * x**3
            A[0][:] = -2.0 * x
            A[1][:] = 1.0
            return 0

    return Equality(ctx, EQ_N, 2, ninequality=1)


def case_problem(ctx, name):
    """(problem, options of the run, equality rows)."""
    if name == "equality":
        return equality_problem(ctx), {"mma_max_iterations": 25, "mma_use_constraint_linearization": 1}, 1
    _, case = load_golden(name)
    opts, mopts = mma_options_from_case(case)
    return make_problem(ctx, case), dict(opts, **mopts), 0


def run_mma(ctx, name, extra, snapshots=()):
    """One MMA run: (mma, rows [(sub-iter, fobj)], {callback k: subproblem k - 1 and its solution})."""
    import paropt_amd as pa

    prob, opts, neq = case_problem(ctx, name)
    mma = pa.MMA(prob, dict(opts, **extra))
    rows, snaps, lin = [], {}, {}

    def cb(k):
        rows.append((mma.getState()["subproblem_iter"], mma.getLastRow()[0]))
        if not snapshots:
            return
        s = mma.getLinearSubproblem()
        # A, cons and xk are already those of subproblem k; the rest still describes subproblem k - 1
        lin[k] = dict(A=[v.to_numpy() for v in s["A"]], cons=s["cons"].copy(), xk=s["xk"].to_numpy())
        if k in snapshots:
            lo, up = mma.getAsymptotes()
            x, z, _, zl, zu = mma.getOptimizedPoint()
            old = lin[k - 1]
            snaps[k] = dict(sp=LinearSubproblem(lo.to_numpy(), up.to_numpy(), s["alpha"].to_numpy(),
                                                s["beta"].to_numpy(), s["p0"].to_numpy(), s["q0"].to_numpy(), old["A"],
                                                old["cons"], old["xk"], neq),
                            x=x.to_numpy(), z=z.copy(), zl=zl.to_numpy(), zu=zu.to_numpy(), stats=mma.getDualStats(),
                            state=mma.getState())
        lin.pop(k - 1, None)

    mma.setIterationCallback(cb)
    mma.optimize()
    return mma, rows, snaps


_RUNS = {}


def dual_run(ctx, name):
    if name not in _RUNS:
        _RUNS[name] = run_mma(ctx, name, dict(LINEAR, mma_dual_tol=1e-9), snapshots=(1, 2, 9))
    return _RUNS[name]


# ---- 2. optimality of the solved subproblems ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [GOLDEN, "equality"])
def test_subproblem_optimality_outside_the_library(ctx, name):
    tol = 1e-9
    mma, rows, snaps = dual_run(ctx, name)
    assert sorted(snaps) == [1, 2, 9]
    for k, s in sorted(snaps.items()):
        sp, x, z = s["sp"], s["x"], s["z"]
        lower, upper = sp.box(PENALTY_GAMMA)
        assert np.all(sp.L < sp.alpha) and np.all(sp.beta < sp.U)
        assert np.all(z >= lower) and np.all(z <= upper)
        free, low, upp = check_point(sp, z, x, "%s @%d" % (name, k))  # alpha <= x <= beta and stationarity
        c = sp.cons + accurate_sum(sp.A * (x - sp.xk))
        pg = np.abs(projected_gradient(z, -c, lower, upper)).max()
        print("%s @%d: max|pg| %.2e, %d free, z = %s" % (name, k, pg, free.sum(), z))
        assert pg <= 10 * tol
        # the bound multipliers close the stationarity condition of every element: r - zl + zu = 0, zl, zu >= 0,
        # zl = 0 off alpha, zu = 0 off beta
        zl, zu = s["zl"], s["zu"]
        assert np.all(zl >= 0.0) and np.all(zu >= 0.0) and not zl[~low].any() and not zu[~upp].any()
        r = residual_longdouble(sp, z, x)
        assert np.all(np.abs(r - zl + zu) <= residual_bound(sp, z, x))
        st = s["stats"]
        assert st["evaluations"] == s["state"]["subproblem_iter"] and st["solves"] == k
        assert st["last_status"] == 0 and st["last_pg"] <= tol
    st = mma.getDualStats()
    assert st["evaluations"] == mma.getState()["subproblem_iter"] == rows[-1][0]
    assert mma.getDualLinearStats()["cap_hits"] == 0


# ---- 3. whole runs against the interior-point path ------------------------------------------------------------------
@pytest.mark.parametrize("name", [GOLDEN, "equality"])
def test_whole_runs_against_the_interior_point(ctx, name):
    _, rows_a, _ = run_mma(ctx, name, {})
    _, rows_b, _ = run_mma(ctx, name, {"abs_res_tol": 1e-9})
    mma_d, rows_d, _ = dual_run(ctx, name)
    ncmp = min(len(rows_a), len(rows_b), len(rows_d))
    assert ncmp >= 15
    fa, fb, fd = (np.array([r[1] for r in rows[:ncmp]]) for rows in (rows_a, rows_b, rows_d))
    scale = np.maximum(1.0, np.abs(fb))
    d_ref = np.maximum.accumulate(np.abs(fa - fb) / scale)
    d_dual = np.abs(fd - fb) / scale
    per_iter_a = rows_a[-1][0] / (len(rows_a) - 1)
    per_iter_d = rows_d[-1][0] / (len(rows_d) - 1)
    record = dict(case=name, rows=ncmp, d_ref=d_ref.tolist(), d_dual=d_dual.tolist(),
                  worst_ratio=float((d_dual / np.maximum(1e-12, d_ref)).max()),
                  ip_iterations_per_mma_iteration=per_iter_a, dual_evaluations_per_mma_iteration=per_iter_d,
                  dual_stats=mma_d.getDualStats(), linear_stats=mma_d.getDualLinearStats(),
                  multipliers=mma_d.getOptimizedPoint()[1].tolist())
    d_gold = None
    if name != "equality":  # the reference's own table
        g, _ = load_golden(name)
        gold = parse_mma_table(g["paropt_mma"])
        ng = min(len(gold), len(rows_d))
        fg = np.array([gold[k][1][0] for k in range(ng)])
        d_gold = np.abs(np.array([r[1] for r in rows_d[:ng]]) - fg) / np.maximum(1.0, np.abs(fg))
        record["d_gold_max"] = float(d_gold.max())
    print(json.dumps({k: v for k, v in record.items() if k not in ("d_ref", "d_dual")}))
    out = os.environ.get("PAROPT_AMD_PROFILE_DIR")
    if out:  # the measurement of profiles/r16_mma_dual_linear_parity.json
        path = os.path.join(out, "r16_mma_dual_linear_parity.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[name] = record
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    for k in range(ncmp):
        assert d_dual[k] <= max(1e-12, d_ref[k]), (k, d_dual[k], d_ref[k])
    if d_gold is not None:
        assert np.all(d_gold <= 1e-4), d_gold
    assert per_iter_d <= per_iter_a, (per_iter_d, per_iter_a)


# ---- 4. interfaces --------------------------------------------------------------------------------------------------
def test_refusals_and_registry(ctx):
    import paropt_amd as pa

    class Untouched(pa.Problem):  # nothing may run: every callback raises
        def getVarsAndBounds(self, x, lb, ub):
            raise AssertionError("the refused solver ran")

        evalObjCon = evalObjConGradient = getVarsAndBounds

    gc.collect()
    sparse = pa.SeparableProblem(ctx, "convex", 240, 3).setWeighting(40, 6, 0, 0)
    dense = pa.SeparableProblem(ctx, "convex", 100, 2)
    equality = Untouched(ctx, 16, 2, ninequality=1)
    cases = [(dense, dict(LINEAR, mma_globalization="conservative"), "not conservative"),
             (sparse, dict(LINEAR, mma_dual_sparse_constraints="groups"), "takes no sparse constraints"),
             (sparse, LINEAR, "sparse constraints"),
             (equality, {"mma_subproblem_solver": "dual", "mma_dual_linearized_constraints": "newton"},
              "a dense equality constraint has a free multiplier, which can make P or Q negative"),
             # the default keeps every refusal of the dual sub-solver
             (dense, {"mma_subproblem_solver": "dual", "mma_use_constraint_linearization": 1},
              "linearised constraints have no rational dual")]
    for prob, opts, sentence in cases:
        mma = pa.MMA(prob, opts)
        live = pa.live_objects()
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2 and sentence in str(e.value), str(e.value)
        assert mma.getState()["mma_iter"] == 0
        assert pa.live_objects() == live  # refused before anything is allocated
        del mma
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.MMA(dense, {"mma_dual_linearized_constraints": "bisection"})
    assert e.value.code == 5 and "mma_dual_linearized_constraints" in str(e.value)


def test_vector_count_getters_and_no_interior_point(ctx):
    import paropt_amd as pa

    _UPLOADS.clear()
    _RUNS.clear()
    gc.collect()
    start = pa.live_objects()[0]
    for c in (3, 9):  # the fused and the panel form
        prob = pa.SeparableProblem(ctx, "convex", 3000, c)
        base = pa.live_objects()[0]
        mma = pa.MMA(prob, dict(LINEAR, mma_max_iterations=3))
        mma.optimize()
        assert pa.live_objects()[0] - base == 17 + c  # no p_i, q_i, no panel columns, no interior point
        st = mma.getDualStats()
        assert st["solves"] == 3 and st["evaluations"] == mma.getState()["subproblem_iter"]
        assert mma.getDualLinearStats()["cap_hits"] == 0 and mma.getDualLinearStats()["max_steps"] >= 1
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.getSubproblem()
        assert e.value.code == 2 and "po_mma_get_linear_subproblem" in str(e.value)
        s = mma.getLinearSubproblem()
        assert len(s["A"]) == c and s["cons"].shape == (c,) and s["xk"].to_numpy().shape == (3000,)
        assert pa.live_objects()[0] - base == 17 + c  # (borrowed views)
        # the sub-solver's mode cannot change once the vectors exist
        mma.setOption("mma_dual_linearized_constraints", "refuse")
        with pytest.raises(pa.ParOptAMDError) as e:
            mma.optimize()
        assert e.value.code == 2
        del mma, s, e  # (the exception's traceback holds the solver)
        gc.collect()
        assert pa.live_objects()[0] == base
        del prob
        gc.collect()
    assert pa.live_objects()[0] == start


def test_facade_optimizer_reaches_the_same_point(ctx):
    import paropt_amd as pa
    from paropt_amd import ParOpt

    _, case = load_golden(GOLDEN)
    _, mopts = mma_options_from_case(case)
    opts = dict(dict(mopts, **LINEAR), mma_dual_tol=1e-9, mma_max_iterations=10)
    mma = pa.MMA(make_problem(ctx, case), opts)
    mma.optimize()
    x1 = mma.getOptimizedPoint()[0].to_numpy()
    opt = ParOpt.Optimizer(make_problem(ctx, case), dict(opts, algorithm="mma", output_file=None, mma_output_file=None))
    opt.optimize()
    x2 = np.array(opt.getOptimizedPoint()[0][:])
    assert np.array_equal(x1, x2)
    assert opt.mma.getLastRow() == mma.getLastRow()
    assert opt.mma.getDualStats()["evaluations"] == mma.getDualStats()["evaluations"] > 0


# ---- 5. two ranks on one GPU ----------------------------------------------------------------------------------------
def _linear_rows(ctx, case, lams):
    import paropt_amd as pa

    opts, mopts = mma_options_from_case(case)
    mma = pa.MMA(make_problem(ctx, case), dict(dict(dict(opts, **mopts), **LINEAR), mma_dual_tol=1e-9,
                                               mma_max_iterations=10))
    rows = []

    def cb(k):
        rows.append(tuple(mma.getLastRow()))
        lams.append(mma.getOptimizedPoint()[1].tobytes())

    mma.setIterationCallback(cb)
    mma.optimize()
    return rows, mma.getDualStats(), mma.getDualLinearStats()


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    _, case = load_golden(GOLDEN)
    lams = []
    rows, stats, lstats = _linear_rows(ctx, case, lams)
    both = [None] * world
    dist.all_gather_object(both, lams)
    if rank == 0:
        q.put((rows, stats, lstats, both))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(ctx):
    _, case = load_golden(GOLDEN)
    lams1 = []
    rows1, stats1, lstats1 = _linear_rows(ctx, case, lams1)
    assert len(rows1) == 11 and stats1["last_status"] == 0
    rows2, stats2, lstats2, both = run_two_ranks(_worker)
    assert both[0] == both[1], "the multipliers differ between the ranks"
    assert len(rows2) == len(rows1)
    for r2, r1 in zip(rows2, rows1):  # the table rows (another summation order over the shards: not the same bits)
        for a, b in zip(r2, r1):
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (r2, r1)
    assert stats2["solves"] == stats1["solves"] and stats2["last_status"] == 0
    assert lstats1["cap_hits"] == 0 and lstats2["cap_hits"] == 0
