"""
GPU parity of the interior-point path (through the C ABI).

  * against the golden trajectories of the compiled reference (tests/golden/ip_*.npz):
    integer bookkeeping (iteration / evaluation counters, quasi-Newton size, info tokens)
    bit-exact over the compared window; mu, fobj, vector norms, dense multipliers and vectors to the tolerance
    SCHEDULE of tests/conftest.py: at iteration k, max(1e-12, 100 x the reference's own self-disagreement up to k)
    (the iteration is nonlinear, the product re-associates every reduction and fuses the Schur complements:
    DESIGN.md "Parity");
  * against the numpy oracle on larger hash-seeded instances where no golden exists;
  * single KKT step against the reference's private-method dump (1e-5 of the step's max).
"""
import numpy as np
import pytest

from conftest import (GOLDEN_WINDOWS, golden_names, golden_vec_view, golden_window, ip_options_from_case,
                      load_golden, tolerance_schedule)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def info_tokens(text):
    toks = {}
    for ln in str(text).splitlines():
        parts = ln.split()
        if len(parts) >= 15 and parts[0].isdigit():
            toks[int(parts[0])] = parts[15:]
    return toks


def build_gpu(ctx, case):
    """(problem, solver) of a golden's case record, not yet run (tools/ip_digest.py imports this half)"""
    import paropt_amd as pa

    a = case["args"]
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a.get("c", 2), a.get("seed", 0),
                               a.get("eig_min", 1.0), a.get("eig_max", 100.0))
    if a.get("nwcon", 0) > 0:
        prob.setWeighting(a["nwcon"], a["nw"], a.get("nwstart", 0), a.get("nwskip", 0),
                          a.get("nwineq", a["nwcon"]))
    if a.get("chain_span", 0) > 0:  # CSR form of the sparse constraints (device sparse Cholesky)
        prob.setChain(a["chain_span"], a.get("chain_stride", 1), a.get("chain_reverse", 0))
    if not (a.get("use_lower", 1) and a.get("use_upper", 1)):
        prob.setVarBoundOptions(a.get("use_lower", 1), a.get("use_upper", 1))
    if a.get("bounds_mode", 0):
        prob.setBoundsMode(a["bounds_mode"])
    opts = ip_options_from_case(case)
    opts["write_output_frequency"] = 0
    return prob, pa.InteriorPoint(prob, opts)


def run_gpu(ctx, case, want_vectors=False):
    prob, ip = build_gpu(ctx, case)
    snaps = []

    def cb(k):
        s = ip.snapshot()
        if want_vectors:
            x, z, zl, zu = ip.getOptimizedPoint()
            s["x"] = x.to_numpy()
            s["zl"] = zl.to_numpy() if zl is not None else None
            s["zu"] = zu.to_numpy() if zu is not None else None
            wv = ip.getOptimizedSparse()
            if wv is not None:
                for key, v in zip(("zw", "sw", "tw", "zsw", "ztw"), wv):
                    s[key] = v.to_numpy()
        snaps.append(s)

    ip.setIterationCallback(cb)
    ip.optimize()
    return ip, snaps


# multi-rank reference runs with dense constraints only are the same global problem: run here on one rank and
# compared on rank 0's shard of the vectors (conftest.golden_vec_view)
MULTI_RANK_OK = ("ip_convex_badbounds5_n201_c2_r2", "ip_quadratic_n100000_c8_bfgs20_r4",
                 "ip_convex_n100000_c32_bfgs10_r4", "ip_convex_n100000_c32_sr1_r4")
IP_CASES = [n for n in golden_names("ip_") + golden_names("ipw_") + golden_names("ipcsr_")
            if (not n.endswith("_r2") or n in MULTI_RANK_OK) and "checkpoint" not in n
            and "nwblock" not in n]  # nwblock: test_gpu_compat


@pytest.mark.parametrize("name", IP_CASES)
def test_ip_trajectory_golden(ctx, name):
    g, case = load_golden(name)
    ip, snaps = run_gpu(ctx, case, want_vectors=True)
    nref = 1 + max(int(k[2:5]) for k in g if k.startswith("it") and k.endswith("/mu"))
    # the WHOLE recorded trajectory (round 5: the tolerance schedule follows the reference's own round-off growth, so
    # no flat window is needed), except the goldens of GOLDEN_WINDOWS, whose integer bookkeeping the reference itself
    # does not reproduce past the listed iteration (tests/conftest.py)
    window = golden_window(name, nref)
    ncmp = min(window, nref, len(snaps))
    assert ncmp >= min(window, nref)
    tol = tolerance_schedule(name)
    for k in range(ncmp):
        p = "it%03d/" % k
        s = snaps[k]
        np.testing.assert_array_equal(s["counters"], g[p + "counters"], err_msg="counters @%d" % k)
        if p + "qn_size" in g:  # absent when the run has no quasi-Newton object (qn_type = none)
            assert s.get("qn_size", 0) == int(g[p + "qn_size"][0]), "qn size @%d" % k
        # SURVEY 8a' integer bookkeeping, bit-exact: pivot rows of the LU factorizations of G and of the compact
        # quasi-Newton matrix (LAPACK numbering), entries sitting at their clamp values
        for key in ("gpiv", "mfpiv", "clamped"):
            if p + key in g:
                np.testing.assert_array_equal(np.asarray(s[key]), g[p + key], err_msg="%s @%d" % (key, k))
        # state: the tolerance schedule of tests/conftest.py -- max(1e-12, 100 x what the REFERENCE's own trajectory
        # moves by up to iteration k when only the summation order of its reductions changes), in the normalisations
        # of oracle/reference_self_disagreement.py
        err = abs(s["mu"] - g[p + "mu"][0]) / abs(g[p + "mu"][0])
        assert err <= tol("mu", k), "mu @%d: %.2e > %.2e" % (k, err, tol("mu", k))
        err = abs(s["fobj"] - g[p + "fobj"][0]) / max(1.0, abs(g[p + "fobj"][0]))
        assert err <= tol("fobj", k), "fobj @%d: %.2e > %.2e" % (k, err, tol("fobj", k))
        na, nb = np.asarray(s["norms"]), np.asarray(g[p + "norms"])
        used = ~(np.isnan(na) | np.isnan(nb)) & (nb != 0)  # a side the problem declares unused has no multiplier vector
        if used.any():
            err = (np.abs(na[used] - nb[used]) / np.abs(nb[used])).max()
            assert err <= tol("norms", k), "norms @%d: %.2e > %.2e" % (k, err, tol("norms", k))
        for key in ("z", "s", "t", "zs", "zt"):
            ref = g[p + key]
            if ref.size:
                err = np.abs(s[key] - ref).max() / max(1.0, np.abs(ref).max())
                assert err <= tol("dense", k), "%s @%d: %.2e > %.2e" % (key, k, err, tol("dense", k))
        if p + "wnorms" in g:
            wa, wb = np.asarray(s["wnorms"]), np.asarray(g[p + "wnorms"])
            nz = wb != 0
            if nz.any():
                err = (np.abs(wa[nz] - wb[nz]) / np.abs(wb[nz])).max()
                assert err <= tol("wnorms", k), "wnorms @%d: %.2e > %.2e" % (k, err, tol("wnorms", k))
        if p + "x" in g:
            keys = ("x", "zl", "zu") + (("zw", "sw", "tw", "zsw", "ztw") if p + "zw" in g else ())
            for key in keys:
                if s[key] is None:
                    continue
                ref = g[p + key]
                mine_v = golden_vec_view(s[key], case) if key in ("x", "zl", "zu") else s[key]
                err = np.abs(mine_v - ref).max() / max(1.0, np.abs(ref).max())
                assert err <= tol("vec", k), "%s @%d: %.2e > %.2e" % (key, k, err, tol("vec", k))
    if "check_flag" in g:  # bound repairs of initAndCheckDesignAndBounds: flag bits and the repaired bounds
        assert ip.getDebugInts()["check_flag"] == int(g["check_flag"][0])
        if "it000/lb" in g:
            lbv, ubv = ip.getBounds()
            np.testing.assert_array_equal(golden_vec_view(lbv.to_numpy(), case), g["it000/lb"])
            np.testing.assert_array_equal(golden_vec_view(ubv.to_numpy(), case), g["it000/ub"])
    toks = info_tokens(g["paropt_out"])
    mine = info_tokens(ip.getHistory())
    for k in range(1, ncmp):
        assert mine.get(k, []) == toks.get(k, []), "info tokens @%d: %s vs %s" % (k, mine.get(k), toks.get(k))
    if "sr1" not in name and name not in GOLDEN_WINDOWS:
        np.testing.assert_array_equal(np.array(ip.getIterationCounters()), g["final/counters"])
        assert abs(ip.getObjective()[0] - g["final/fobj"][0]) <= 1e-6 * max(1.0, abs(g["final/fobj"][0]))
        if "hvec" in name:  # total Hessian-vector products = total GMRES iterations (nhvc column)
            rows = [ln.split() for ln in str(g["paropt_out"]).splitlines() if ln[:5].strip().isdigit()]
            assert ip.getHvecCount() == int(rows[-1][3])


KAT_CASES = ["ip_quadratic_n257_c3_bfgs", "ip_quadratic_n1000_c8_bfgs20", "ip_convex_n300_c5_bfgs",
             "ip_convex_n300_c5_sr1"]


@pytest.mark.parametrize("name", KAT_CASES)
def test_ip_single_step_kat(ctx, name):
    """computeKKTRes + setUpKKTDiagSystem + setUpKKTSystem + computeKKTStep of the reference
    (private methods) at iteration kat_iter vs the fused device step from the same state."""
    import paropt_amd as pa

    g, case = load_golden(name)
    a = case["args"]
    kat = a["kat_iter"]
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a.get("c", 2), 0, a.get("eig_min", 1.0),
                               a.get("eig_max", 100.0))
    opts = ip_options_from_case(case)
    opts["write_output_frequency"] = 0
    ip = pa.InteriorPoint(prob, opts)
    out = {}

    def cb(k):
        if k == kat:
            out["x"] = ip.getOptimizedPoint()[0].to_numpy()
            out.update({"step_" + key: v for key, v in ip.debugKKTStep(ip.getBarrierParameter()).items()})
            out["comp"] = ip.getComplementarity()

    ip.setIterationCallback(cb)
    ip.optimize()
    assert "step_x" in out
    np.testing.assert_allclose(out["x"], g["kat/x"], rtol=0, atol=1e-7)
    for key in ("x", "zl", "zu", "z", "s", "t", "zs", "zt"):
        ref = g["kat/step_" + key]
        np.testing.assert_allclose(out["step_" + key], ref, rtol=0,
                                   atol=2e-5 * max(1e-3, np.abs(ref).max()), err_msg=key)
    assert abs(out["comp"] - g["kat/comp"][0]) <= 1e-6 * abs(g["kat/comp"][0])


@pytest.mark.parametrize("problem,n,c,qn,m", [
    ("quadratic", 100003, 8, "bfgs", 20),   # config 2 shape (c=8, L-BFGS(20)), odd n
    ("convex", 65536, 32, "bfgs", 10),      # config 3 shape with the convergent L-BFGS variant
    ("convex", 50001, 32, "sr1", 10),       # config 3 proper (L-SR1): short window
])
def test_ip_vs_oracle_large(ctx, problem, n, c, qn, m):
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    opts = {"qn_subspace_size": m, "qn_type": qn, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 12 if qn == "sr1" else 30}
    oip = po.InteriorPoint(po.SepProblem(problem, n, c), opts)
    osn = []
    oip.hook = lambda s, k: osn.append(s.snapshot())
    oip.optimize()
    gopts = dict(opts, write_output_frequency=0)
    ip = pa.InteriorPoint(pa.SeparableProblem(ctx, problem, n, c), gopts)
    gsn = []
    ip.setIterationCallback(lambda k: gsn.append(ip.snapshot()))
    ip.optimize()
    ncmp = min(len(osn), len(gsn), 8 if qn == "sr1" else 30)
    assert ncmp >= (8 if qn == "sr1" else 12)
    for k in range(ncmp):
        np.testing.assert_array_equal(gsn[k]["counters"], osn[k]["counters"], err_msg="counters @%d" % k)
        assert gsn[k]["qn_size"] == osn[k]["qn_size"]
        assert abs(gsn[k]["mu"] - osn[k]["mu"]) <= 1e-6 * abs(osn[k]["mu"])
        assert abs(gsn[k]["fobj"] - osn[k]["fobj"]) <= 1e-6 * max(1.0, abs(osn[k]["fobj"]))
        np.testing.assert_allclose(gsn[k]["norms"], osn[k]["norms"], rtol=1e-6)
    assert [t["info"].split() for t in oip.trace[1:ncmp]] == [
        info_tokens(ip.getHistory()).get(k, []) for k in range(1, ncmp)]


SWEEP = [
    # problem, n, c, qn, m, options, weighting (nwcon, nw, nwstart, nwskip, nwineq) or None
    ("quadratic", 1, 1, "bfgs", 3, {}, None),
    ("quadratic", 2, 1, "sr1", 2, {}, None),
    ("convex", 127, 3, "bfgs", 4, {"barrier_strategy": "mehrotra"}, None),
    ("convex", 129, 2, "bfgs", 4, {"barrier_strategy": "mehrotra_predictor_corrector"}, None),
    ("quadratic", 511, 5, "bfgs", 7, {"norm_type": "l1"}, None),
    ("quadratic", 513, 17, "bfgs", 6, {"barrier_strategy": "complementarity_fraction"}, None),
    ("convex", 1025, 33, "bfgs", 12, {"use_line_search": False}, None),
    ("rosenbrock", 255, 2, "bfgs", 5, {"abs_res_tol": 1e-6, "starting_point_strategy": "least_squares_multipliers"}, None),
    ("convex", 513, 2, "bfgs", 5, {}, (51, 7, 3, 3, 51)),            # groups straddle the 512-variable tile
    ("convex", 1200, 3, "bfgs", 4, {}, (2, 513, 10, 60, 1)),        # groups wider than a tile: untiled kernels
    ("quadratic", 777, 4, "sr1", 5, {}, (97, 8, 1, 0, 40)),         # mixed inequality / equality groups
    ("convex", 300, 2, "bfgs", 5, {"use_diag_hessian": True}, (60, 5, 0, 0, 60)),
    ("convex", 640, 3, "bfgs", 6, {"use_hvec_product": True, "gmres_subspace_size": 8, "nk_switch_tol": 1e3,
                                   "max_gmres_rtol": 1.0}, None),
    # panels wider than one launch of the kernels (c + k > 80: blocked Gram; > 96: collapsed panel sums) on the
    # branches that take other kernels than the plain quasi-Newton iteration (which has reference-run goldens)
    ("convex", 900, 97, "bfgs", 4, {"barrier_strategy": "mehrotra_predictor_corrector"}, None),
    ("quadratic", 700, 101, "bfgs", 3, {"use_line_search": False, "norm_type": "l2"}, None),
    ("convex", 1000, 90, "bfgs", 5, {}, (100, 8, 0, 2, 100)),       # sparse constraints + 100 panel columns
    ("convex", 800, 99, "bfgs", 4, {"use_diag_hessian": True}, None),
    ("convex", 640, 98, "bfgs", 3, {"use_hvec_product": True, "gmres_subspace_size": 6, "nk_switch_tol": 1e3,
                                    "max_gmres_rtol": 1.0}, None),
    ("quadratic", 600, 60, "bfgs", 15, {}, None),                   # 60 + 30 = 90 columns: blocked Gram, fused passes
    # iterative refinement off and twice, on the dense and on the weighting path (the default is one step)
    ("convex", 257, 3, "bfgs", 5, {"iterative_refinement_steps": 0}, None),
    ("convex", 257, 3, "bfgs", 5, {"iterative_refinement_steps": 2}, None),
    ("quadratic", 300, 4, "sr1", 4, {"iterative_refinement_steps": 0}, None),
    ("quadratic", 300, 4, "sr1", 4, {"iterative_refinement_steps": 2}, None),
    ("convex", 513, 2, "bfgs", 5, {"iterative_refinement_steps": 0}, (51, 7, 3, 3, 51)),
    ("convex", 513, 2, "bfgs", 5, {"iterative_refinement_steps": 2}, (51, 7, 3, 3, 51)),
]


@pytest.mark.parametrize("problem,n,c,qn,m,extra,wt", SWEEP)
def test_ip_size_and_option_sweep(ctx, problem, n, c, qn, m, extra, wt):
    """Awkward sizes (1, 2, odd, one off the tile sizes 128 / 512 / 1024, panels of 1..33 columns) and
    option combinations without a golden, against the oracle: counters and info tokens exactly."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    opts = {"qn_subspace_size": m, "qn_type": qn, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 8 if qn == "sr1" else 14}
    opts.update(extra)
    wargs = dict(nwcon=wt[0], nw=wt[1], nwstart=wt[2], nwskip=wt[3], nwineq=wt[4]) if wt else {}
    oip = po.InteriorPoint(po.SepProblem(problem, n, c, **wargs), opts)
    osn = []
    oip.hook = lambda s, k: osn.append(s.snapshot())
    oip.optimize()
    prob = pa.SeparableProblem(ctx, problem, n, c)
    if wt:
        prob.setWeighting(*wt)
    ip = pa.InteriorPoint(prob, dict(opts, write_output_frequency=0))
    gsn = []
    ip.setIterationCallback(lambda k: gsn.append(ip.snapshot()))
    ip.optimize()
    ncmp = min(len(osn), len(gsn))
    assert ncmp >= min(len(osn), 6)
    for k in range(ncmp):
        np.testing.assert_array_equal(gsn[k]["counters"], osn[k]["counters"], err_msg="counters @%d" % k)
        assert gsn[k]["qn_size"] == osn[k]["qn_size"]
        assert abs(gsn[k]["mu"] - osn[k]["mu"]) <= 1e-6 * abs(osn[k]["mu"]), k
        assert abs(gsn[k]["fobj"] - osn[k]["fobj"]) <= 1e-6 * max(1.0, abs(osn[k]["fobj"])), k
        np.testing.assert_allclose(gsn[k]["norms"], osn[k]["norms"], rtol=1e-6, atol=1e-12)
        if wt:
            np.testing.assert_allclose(gsn[k]["wnorms"], osn[k]["wnorms"], rtol=1e-6)
    assert [t["info"].split() for t in oip.trace[1:ncmp]] == [
        info_tokens(ip.getHistory()).get(k, []) for k in range(1, ncmp)]


def test_python_callback_problem(ctx):
    """The drop-in boundary for user problems: a Python-implemented problem (host arrays via
    getArray, as the reference's examples do) driven by the device solver -- the 2-constraint
    Rosenbrock of examples/rosenbrock/rosenbrock.cpp, compared with the built-in device problem."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n = 100
    oracle_prob = po.SepProblem("rosenbrock", n, 2)

    class Rosen(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = -1.0, -2.0, 1.0

        def evalObjCon(self, x):
            return oracle_prob.eval_obj_con(x)

        def evalObjConGradient(self, x, g, A):
            _, gg, aa = oracle_prob.eval_obj_con_gradient(x)
            g[:] = gg
            A[0][:], A[1][:] = aa[0], aa[1]
            return 0

    opts = {"qn_subspace_size": 10, "abs_res_tol": 1e-6, "max_major_iters": 120, "write_output_frequency": 0}
    ip1 = pa.InteriorPoint(Rosen(ctx, n, 2), opts)
    ip1.optimize()
    ip2 = pa.InteriorPoint(pa.SeparableProblem(ctx, "rosenbrock", n), opts)
    ip2.optimize()
    assert ip1.getIterationCounters() == ip2.getIterationCounters()
    np.testing.assert_allclose(ip1.getOptimizedPoint()[0].to_numpy(), ip2.getOptimizedPoint()[0].to_numpy(),
                               rtol=0, atol=1e-9)
    g, _ = load_golden("ip_rosenbrock_n100")
    np.testing.assert_array_equal(np.array(ip1.getIterationCounters()), g["final/counters"])


def test_python_callback_exception_is_not_swallowed(ctx):
    """An exception thrown inside a problem callback stops the solve (non-zero callback return) and is re-raised
    by optimize() -- it must not be reported as a successful evaluation."""
    import paropt_amd as pa

    n = 50
    calls = {"n": 0}

    class P(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:] = 0.5
            lb[:] = 0.0
            ub[:] = 1.0

        def evalObjCon(self, x):
            calls["n"] += 1
            if calls["n"] == 3:
                raise ZeroDivisionError("user bug")
            return 0, float(np.dot(x - 0.3, x - 0.3)), np.array([x.sum() - 5.0])

        def evalObjConGradient(self, x, g, A):
            g[:] = 2.0 * (x - 0.3)
            A[0][:] = 1.0
            return 0

    ip = pa.InteriorPoint(P(ctx, n, 1), {"max_major_iters": 20, "write_output_frequency": 0})
    with pytest.raises(ZeroDivisionError):
        ip.optimize()
    assert calls["n"] == 3  # no user code ran after the exception


def test_python_callback_sparse_constraints(ctx):
    """Sparse (weighting) constraints through the callback boundary: the reference's own example
    (examples/rosenbrock/rosenbrock.cpp: nwcon=5, nw=5, start 1, skip 1) implemented in Python on
    host arrays -- this exercises the generic column-by-column U = Aw (Dinv o P) fallback -- against
    the built-in structured problem and the golden trajectory of the compiled reference."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n = 100
    op = po.SepProblem("rosenbrock", n, 2, nwcon=5, nw=5, nwstart=1, nwskip=1)

    class RosenW(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = -1.0, -2.0, 1.0

        def evalObjCon(self, x):
            return op.eval_obj_con(x)

        def evalObjConGradient(self, x, g, A):
            _, gg, aa = op.eval_obj_con_gradient(x)
            g[:] = gg
            A[0][:], A[1][:] = aa[0], aa[1]
            return 0

        def evalSparseCon(self, x, out):
            out[:] = op.eval_sparse_con(x)

        def addSparseJacobian(self, alpha, x, px, out):
            op.add_sparse_jacobian(alpha, px, out)

        def addSparseJacobianTranspose(self, alpha, x, pzw, out):
            op.add_sparse_jacobian_transpose(alpha, pzw, out)

        def addSparseInnerProduct(self, alpha, x, cvec, A):
            op.add_sparse_inner_product(alpha, cvec, A)

    g, case = load_golden("ipw_rosenbrock_n100_w5")
    opts = ip_options_from_case(case)
    opts["write_output_frequency"] = 0
    ip1 = pa.InteriorPoint(RosenW(ctx, n, 2, nwcon=5, nwinequality=5), opts)
    ip1.optimize()
    ip2 = pa.InteriorPoint(pa.SeparableProblem(ctx, "rosenbrock", n).setWeighting(5, 5, 1, 1), opts)
    ip2.optimize()
    assert ip1.getIterationCounters() == ip2.getIterationCounters()
    np.testing.assert_allclose(ip1.getOptimizedPoint()[0].to_numpy(), ip2.getOptimizedPoint()[0].to_numpy(),
                               rtol=0, atol=1e-8)
    for a, b in zip(ip1.getOptimizedSparse(), ip2.getOptimizedSparse()):
        np.testing.assert_allclose(a.to_numpy(), b.to_numpy(), rtol=0, atol=1e-8)
    np.testing.assert_array_equal(np.array(ip1.getIterationCounters()), g["final/counters"])
    np.testing.assert_allclose(ip1.getOptimizedPoint()[0].to_numpy(), g["final/x"], rtol=0, atol=1e-6)


def test_weighting_large_vs_oracle(ctx):
    """Config-4 shape at a size the oracle finishes quickly: convex objective, 8 dense constraints,
    one weighting constraint per group of 20 variables (n = 20000, nwcon = 1000)."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n, c, nw = 20000, 8, 20
    opts = {"qn_type": "bfgs", "qn_subspace_size": 10, "abs_res_tol": 1e-8,
            "starting_point_strategy": "affine_step", "start_affine_multiplier_min": 0.01,
            "penalty_gamma": 1000.0, "max_major_iters": 15}
    oprob = po.SepProblem("convex", n, c, nwcon=n // nw, nw=nw, nwstart=0, nwskip=0)
    oip = po.InteriorPoint(oprob, dict(opts))
    osnaps = []
    oip.hook = lambda ip_, k: osnaps.append(ip_.snapshot())
    oip.optimize()
    prob = pa.SeparableProblem(ctx, "convex", n, c).setWeighting(n // nw, nw, 0, 0)
    ip = pa.InteriorPoint(prob, dict(opts, write_output_frequency=0))
    snaps = []
    ip.setIterationCallback(lambda k: snaps.append(ip.snapshot()))
    ip.optimize()
    assert len(snaps) == len(osnaps)
    for k, (a, b) in enumerate(zip(snaps, osnaps)):
        np.testing.assert_array_equal(a["counters"], b["counters"], err_msg="counters @%d" % k)
        assert abs(a["mu"] - b["mu"]) <= 1e-6 * abs(b["mu"]), k
        assert abs(a["fobj"] - b["fobj"]) <= 1e-7 * max(1.0, abs(b["fobj"])), k
        np.testing.assert_allclose(a["norms"], b["norms"], rtol=1e-6, err_msg="norms @%d" % k)
        np.testing.assert_allclose(a["wnorms"], b["wnorms"], rtol=1e-6, err_msg="wnorms @%d" % k)


def test_python_hessian_callbacks(ctx):
    """evalHvecProduct / evalHessianDiag through the callback boundary (use_hvec_product with the
    GMRES inexact Newton step, use_diag_hessian): a Python problem against the built-in one and the
    reference's golden trajectories."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n = 100
    op = po.SepProblem("rosenbrock", n, 2)

    class Rosen(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = -1.0, -2.0, 1.0

        def evalObjCon(self, x):
            return op.eval_obj_con(x)

        def evalObjConGradient(self, x, g, A):
            _, gg, aa = op.eval_obj_con_gradient(x)
            g[:] = gg
            A[0][:], A[1][:] = aa[0], aa[1]
            return 0

        def evalHvecProduct(self, x, z, zw, px, hvec):
            hvec[:] = op.hvec_product(x, z, px)
            return 0

        def evalHessianDiag(self, x, z, zw, hdiag):
            hdiag[:] = op.hessian_diag(x, z)
            return 0

    for name in ("ip_rosenbrock_hvec_n100", "ip_rosenbrock_diaghess_n100"):
        g, case = load_golden(name)
        opts = ip_options_from_case(case)
        opts["write_output_frequency"] = 0
        ip1 = pa.InteriorPoint(Rosen(ctx, n, 2), opts)
        ip1.optimize()
        ip2 = pa.InteriorPoint(pa.SeparableProblem(ctx, "rosenbrock", n), opts)
        ip2.optimize()
        assert ip1.getIterationCounters() == ip2.getIterationCounters()
        np.testing.assert_array_equal(np.array(ip1.getIterationCounters()), g["final/counters"])
        np.testing.assert_allclose(ip1.getOptimizedPoint()[0].to_numpy(), g["final/x"], rtol=0, atol=1e-6)
        if "hvec" in name:
            assert "iNK" in ip1.getHistory()


def test_external_quasi_newton_and_penalties(ctx):
    """setQuasiNewton / setPenaltyGamma(array) / getIterationCounters' nhvec (src/ParOptInteriorPoint.h:
    157-185): a caller-owned L-BFGS gives the same trajectory as the solver's own, per-constraint penalties
    equal to the scalar default change nothing, a detached approximation needs the sequential linear mode."""
    import paropt_amd as pa

    n, c = 3000, 3
    opts = {"qn_subspace_size": 6, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 25, "write_output_frequency": 0}
    ip1 = pa.InteriorPoint(pa.SeparableProblem(ctx, "quadratic", n, c), opts)
    ip1.optimize()
    prob2 = pa.SeparableProblem(ctx, "quadratic", n, c)
    ip2 = pa.InteriorPoint(prob2, opts)
    qn = pa.LBFGS(ctx, prob2.nvars, 6)
    ip2.setQuasiNewton(qn)
    ip2.setMultiplePenaltyGamma([1000.0] * c)
    ip2.optimize()
    assert ip1.getIterationCounters() == ip2.getIterationCounters()
    np.testing.assert_allclose(ip2.getOptimizedPoint()[0].to_numpy(), ip1.getOptimizedPoint()[0].to_numpy(),
                               rtol=0, atol=1e-12)
    k = C_int_size(qn)
    assert k == 12  # the caller's object holds the pairs
    assert ip2.getHvecCount() == 0
    ip3 = pa.InteriorPoint(pa.SeparableProblem(ctx, "quadratic", n, c), dict(opts, max_major_iters=5))
    ip3.setQuasiNewton(None)
    with pytest.raises(pa.ParOptAMDError):
        ip3.optimize()  # neither a quasi-Newton approximation nor a sequential linear method


def C_int_size(qn):
    import ctypes as C

    from paropt_amd import lib as L

    k, b0 = C.c_int(), C.c_double()
    L.check(L.lib.po_qn_get_compact(qn._h, C.byref(k), C.byref(b0), None, None, None))
    return k.value


def test_option_errors(ctx):
    import paropt_amd as pa

    ip = pa.InteriorPoint(pa.SeparableProblem(ctx, "quadratic", 100, 2))
    with pytest.raises(pa.ParOptAMDError):
        ip.setOption("no_such_option", 1)
    with pytest.raises(pa.ParOptAMDError):
        ip.setOption("qn_type", "nonsense")
    with pytest.raises(pa.ParOptAMDError):
        ip.setOption("max_line_iters", 1000)  # out of range [1, 100]


def test_explicit_and_analytic_panel_dots_agree(ctx, monkeypatch):
    """The W-based shortcuts (P^T px from the weighted Gram, fused refinement residual, rx-based
    quasi-Newton gradient difference) against the same solver with every one of those quantities
    re-measured by explicit passes (PAROPT_AMD_EXPLICIT_DOTS=1)."""
    import paropt_amd as pa

    opts = {"qn_subspace_size": 8, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 40, "write_output_frequency": 0}
    runs = []
    for explicit in (False, True):
        if explicit:
            monkeypatch.setenv("PAROPT_AMD_EXPLICIT_DOTS", "1")
        else:
            monkeypatch.delenv("PAROPT_AMD_EXPLICIT_DOTS", raising=False)
        ip = pa.InteriorPoint(pa.SeparableProblem(ctx, "convex", 30011, 12), opts)
        sn = []
        ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
        ip.optimize()
        runs.append((sn, ip.getHistory(), ip.getOptimizedPoint()[0].to_numpy()))
    monkeypatch.delenv("PAROPT_AMD_EXPLICIT_DOTS", raising=False)
    a, b = runs
    assert len(a[0]) == len(b[0])
    for sa, sb in zip(a[0], b[0]):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["qn_size"] == sb["qn_size"]
        assert abs(sa["fobj"] - sb["fobj"]) <= 1e-8 * max(1.0, abs(sb["fobj"]))
        np.testing.assert_allclose(sa["norms"], sb["norms"], rtol=1e-8)
    assert info_tokens(a[1]) == info_tokens(b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-8)


@pytest.mark.parametrize("problem,qn,strategy", [("convex", "sr1", "monotone"), ("quadratic", "bfgs", "monotone"),
                                                 ("convex", "bfgs", "mehrotra_predictor_corrector")])
def test_linear_constraint_declaration_changes_nothing(ctx, problem, qn, strategy):
    """po_problem_set_linear_constraints: the Jacobian of the first gradient evaluation is kept, the gradient
    callback is asked for the objective gradient only, and A^T z follows the multiplier steps by recurrence
    (rebuilt every 16 iterations) instead of streaming the constraint gradients: same trajectory as the plain
    contract (counters / tokens bit-exact, state to 1e-8)."""
    import paropt_amd as pa

    # (the L-SR1 run on this problem does not settle -- SURVEY 8c -- and amplifies round-off: short window)
    opts = {"qn_type": qn, "qn_subspace_size": 6, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 24 if qn == "sr1" else 45, "write_output_frequency": 0, "barrier_strategy": strategy}
    runs = []
    for flag in (False, True):
        prob = pa.SeparableProblem(ctx, problem, 20011, 7)
        prob.setLinearConstraints(flag)
        ip = pa.InteriorPoint(prob, opts)
        sn = []
        ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
        ip.optimize()
        runs.append((sn, ip.getHistory(), ip.getOptimizedPoint()[0].to_numpy(), ip.getPhaseTimes()))
    a, b = runs
    assert len(a[0]) == len(b[0]) and len(a[0]) > 20
    # The recurrence re-associates A^T z (differences of 1e-14 at the second iteration); the convex problem's
    # trajectories are sensitive (|opt| stays O(100) for dozens of iterations) and amplify that by about one
    # decade every three iterations, so the state is compared over the first 18 iterations (through one rebuild
    # of A^T z at iteration 16) and the integer bookkeeping over the whole run where the problem is well behaved.
    # (the L-SR1 run takes a knife-edge line-search decision at iteration 15 -- 2 vs 3 trial points on differences
    # of 1e-12 -- after which the two runs are different trajectories: the same sensitivity the golden window of
    # the L-SR1 cases documents)
    window = len(a[0]) if problem == "quadratic" else (14 if qn == "sr1" else 18)
    for sa, sb in list(zip(a[0], b[0]))[:window]:
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["qn_size"] == sb["qn_size"]
        assert abs(sa["fobj"] - sb["fobj"]) <= 1e-8 * max(1.0, abs(sb["fobj"]))
        np.testing.assert_allclose(sa["norms"], sb["norms"], rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(sa["z"], sb["z"], rtol=1e-6, atol=1e-8)
    if problem == "quadratic":
        assert info_tokens(a[1]) == info_tokens(b[1])
        np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-7)
    else:
        ta, tb = info_tokens(a[1]), info_tokens(b[1])
        assert {k: v for k, v in ta.items() if k < window} == {k: v for k, v in tb.items() if k < window}


def test_linear_constraints_python_callback_gets_no_jacobian(ctx):
    """With the declaration, a callback problem sees Ac = None after the first gradient evaluation of an
    optimize() call (and never without it)."""
    import paropt_amd as pa

    n, c = 500, 2
    rng = np.random.default_rng(3)
    A = rng.uniform(0.0, 1.0, size=(c, n))
    q = rng.uniform(1.0, 5.0, size=n)
    calls = []

    class P(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:] = 0.5
            lb[:] = 0.0
            ub[:] = 1.0

        def evalObjCon(self, x):
            return 0, float(0.5 * np.dot(q * x, x)), (A @ x - 0.1 * A.sum(axis=1))

        def evalObjConGradient(self, x, g, Ac):
            calls.append(Ac is None)
            g[:] = q * x
            if Ac is not None:
                for j in range(c):
                    Ac[j][:] = A[j]
            return 0

    opts = {"qn_subspace_size": 4, "abs_res_tol": 1e-7, "max_major_iters": 12, "write_output_frequency": 0}
    res = []
    for flag in (False, True):
        calls.clear()
        prob = P(ctx, n, c)
        if flag:
            prob.setLinearConstraints(True)
        ip = pa.InteriorPoint(prob, opts)
        ip.optimize()
        res.append((list(calls), ip.getOptimizedPoint()[0].to_numpy(), ip.getIterationCounters()))
    assert not any(res[0][0])
    assert res[1][0][0] is False and all(res[1][0][1:]) and len(res[1][0]) > 3
    assert res[0][2] == res[1][2]
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("problem,extra", [("quadratic", {}), ("convex", {"qn_type": "sr1"}),
                                           ("rosenbrock", {"use_hvec_product": True, "gmres_subspace_size": 10})])
def test_step_and_gradient_verification_options(ctx, problem, extra):
    """step_verification_frequency / gradient_verification_frequency (src/ParOptInteriorPoint.cpp:4522-4525,
    4635-4639, 5056-5073): the diagnostics land in the iteration history, the computed step zeroes every block of the
    linearised KKT system, the user's gradients pass the finite-difference check, and the iterates are exactly those
    of the run without the diagnostics."""
    import re

    import paropt_amd as pa

    base = dict({"qn_subspace_size": 6, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
                 "max_major_iters": 16, "write_output_frequency": 0}, **extra)
    runs = []
    for diag in (False, True):
        opts = dict(base)
        if diag:
            opts.update(step_verification_frequency=5, gradient_verification_frequency=7)
        ip = pa.InteriorPoint(pa.SeparableProblem(ctx, problem, 3001, 4), opts)
        ip.optimize()
        runs.append((ip.getHistory(), ip.getOptimizedPoint()[0].to_numpy(), ip.getIterationCounters()))
    plain, diag = runs
    assert plain[2] == diag[2]
    np.testing.assert_array_equal(plain[1], diag[1])
    hist = diag[0]
    assert "Residual step check" not in plain[0] and "Gradient check" not in plain[0]
    for k in (0, 5, 10, 15):
        assert "Residual step check for iteration %d:" % k in hist
    # every block of the linearised system is solved to round-off relative to the size of the step / state
    vals = [float(v) for v in re.findall(r"max \|[^|]*\|:\s+([0-9.eE+-]+)", hist)]
    assert len(vals) == 4 * 8
    assert max(vals) < 1e-6, vals
    assert hist.count("Gradient check") == 3  # iterations 0, 7, 14
    rel = [float(ln.split()[3]) for ln in hist.splitlines()
           if len(ln.split()) == 4 and ln.split()[0][0] in "-0123456789" and "e" in ln.split()[3]]
    ncon = 2 if problem == "rosenbrock" else 4
    assert len(rel) >= 3 * (1 + ncon) and max(rel) < 1e-3, rel  # forward differences, dh = 1e-6
    if problem == "rosenbrock":
        assert "Hessian-vector product test" in hist


def test_solution_file_format(ctx, tmp_path):
    """The binary checkpoint of writeSolutionFile (src/ParOptInteriorPoint.cpp:883-972): same
    layout as the file the reference left behind (header ints bit-exact, payload to 1e-6), and a
    readSolutionFile round trip."""
    import struct

    import paropt_amd as pa

    g, case = load_golden("ip_quadratic_checkpoint_n130_c3")
    ref = g["checkpoint_bytes"].tobytes()
    a = case["args"]
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"])
    opts = ip_options_from_case(case)
    ip = pa.InteriorPoint(prob, opts)
    path = str(tmp_path / "ckpt.bin")
    ip.optimize(checkpoint=path)
    mine = open(path, "rb").read()
    assert len(mine) == len(ref) == 12 + (5 * a["c"] + 1) * 8 + 3 * a["n"] * 8
    assert mine[:12] == ref[:12] and struct.unpack("<3i", mine[:12]) == (a["n"], 0, a["c"])
    pm = np.frombuffer(mine[12:], dtype="<f8")
    pr = np.frombuffer(ref[12:], dtype="<f8")
    np.testing.assert_allclose(pm, pr, rtol=1e-6, atol=1e-6 * np.abs(pr).max())
    # restart: a fresh solver reads the reference's own file
    refpath = str(tmp_path / "ref.bin")
    open(refpath, "wb").write(ref)
    ip2 = pa.InteriorPoint(pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"]), opts)
    ip2.readSolutionFile(refpath)
    x, z, zl, zu = ip2.getOptimizedPoint()
    c = a["c"]
    np.testing.assert_array_equal(x.to_numpy(), pr[1 + 5 * c: 1 + 5 * c + a["n"]])
    np.testing.assert_array_equal(z, pr[1 + 2 * c: 1 + 3 * c])
    assert ip2.getBarrierParameter() == pr[0]
    with pytest.raises(pa.ParOptAMDError):
        pa.InteriorPoint(pa.SeparableProblem(ctx, a["problem"], a["n"] + 1, a["c"]), opts).readSolutionFile(refpath)


def test_solution_file_format_sparse(ctx, tmp_path):
    """Checkpoint layout with sparse constraints: the header carries nwcon and zw, sw follow zu
    (src/ParOptInteriorPoint.cpp:951-968)."""
    import struct

    import paropt_amd as pa

    g, case = load_golden("ipw_convex_checkpoint_n120_c2_w20")
    ref = g["checkpoint_bytes"].tobytes()
    a = case["args"]

    def make():
        return pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"]).setWeighting(
            a["nwcon"], a["nw"], a["nwstart"], a["nwskip"])

    opts = ip_options_from_case(case)
    ip = pa.InteriorPoint(make(), opts)
    path = str(tmp_path / "ckpt.bin")
    ip.optimize(checkpoint=path)
    mine = open(path, "rb").read()
    assert len(mine) == len(ref) == 12 + (5 * a["c"] + 1) * 8 + 3 * a["n"] * 8 + 2 * a["nwcon"] * 8
    assert mine[:12] == ref[:12] and struct.unpack("<3i", mine[:12]) == (a["n"], a["nwcon"], a["c"])
    pm = np.frombuffer(mine[12:], dtype="<f8")
    pr = np.frombuffer(ref[12:], dtype="<f8")
    np.testing.assert_allclose(pm, pr, rtol=1e-6, atol=1e-6 * np.abs(pr).max())
    refpath = str(tmp_path / "ref.bin")
    open(refpath, "wb").write(ref)
    ip2 = pa.InteriorPoint(make(), opts)
    ip2.readSolutionFile(refpath)
    zw, sw = ip2.getOptimizedSparse()[:2]
    base = 1 + 5 * a["c"] + 3 * a["n"]
    np.testing.assert_array_equal(zw.to_numpy(), pr[base: base + a["nwcon"]])
    np.testing.assert_array_equal(sw.to_numpy(), pr[base + a["nwcon"]: base + 2 * a["nwcon"]])


def test_output_file_table(ctx, tmp_path):
    """`output_file` receives the iteration table in the reference's column layout
    (src/ParOptInteriorPoint.cpp:4777-4801): the values printed by the reference and by the device
    solver agree to the printed precision for the compared iterations."""
    import paropt_amd as pa

    g, case = load_golden("ip_quadratic_n257_c3_bfgs")
    a = case["args"]
    opts = ip_options_from_case(case)
    opts["write_output_frequency"] = 0
    opts["output_file"] = str(tmp_path / "paropt.out")
    ip = pa.InteriorPoint(pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"]), opts)
    ip.optimize()

    def rows(text):
        out = {}
        for ln in str(text).splitlines():
            p = ln.split()
            if len(p) >= 15 and p[0].isdigit():
                out[int(p[0])] = p
        return out

    mine, ref = rows(open(opts["output_file"]).read()), rows(g["paropt_out"])
    assert len(mine) == len(ref)
    for k in range(1, 20):
        assert mine[k][:4] == ref[k][:4]                      # iter nobj ngrd nhvc
        assert mine[k][4:7] == ref[k][4:7]                    # alpha alphx alphz (2 digits)
        assert abs(float(mine[k][7]) - float(ref[k][7])) <= 2e-5 * max(1.0, abs(float(ref[k][7])))  # fobj
        assert mine[k][11] == ref[k][11]                      # mu
        assert mine[k][15:] == ref[k][15:]                    # info tokens


@pytest.mark.parametrize("problem,qn", [("quadratic", "bfgs"), ("convex", "sr1"), ("rosenbrock", "bfgs")])
def test_check_kkt_step_residual(ctx, problem, qn):
    """The reference's checkKKTStep (src/ParOptInteriorPoint.cpp:6212-6360) without the reference: at an interior
    iteration the fused device step p must satisfy the linearised KKT system K p = r assembled DENSELY in numpy from
    the state, the problem data and the compact quasi-Newton matrix B = b0 I - Z d0 M^-1 d0 Z^T (no oracle code
    on either side of the comparison)."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po  # only for the problem data (hash-seeded vectors)

    n, c = 200, 3
    data = po.SepProblem(problem, n, c)
    c = data.c
    prob = pa.SeparableProblem(ctx, problem, n, c)
    ip = pa.InteriorPoint(prob, {"qn_type": qn, "qn_subspace_size": 5, "max_major_iters": 9, "abs_res_tol": 1e-30})
    got = {}

    def cb(k):
        if k != 8:
            return
        mu = ip.getBarrierParameter()
        x, z, zl, zu = ip.getOptimizedPoint()
        s, t, zs, zt = ip.getOptimizedSlacks()
        b0, d0, M, Z = ip.getQuasiNewton().getCompactMat()
        got.update(mu=mu, x=x.to_numpy(), z=np.array(z), zl=zl.to_numpy(), zu=zu.to_numpy(), s=np.array(s),
                   t=np.array(t), zs=np.array(zs), zt=np.array(zt), b0=b0, d0=d0, M=M,
                   Z=[v.to_numpy() for v in Z], p=ip.debugKKTStep(mu))

    ip.setIterationCallback(cb)
    ip.optimize()
    g = got
    x, p = g["x"], g["p"]
    _, grad, A = data.eval_obj_con_gradient(x)
    _, _, cons = data.eval_obj_con(x)
    A = np.array(A)
    _, lb, ub = data.vars_and_bounds()
    beta, mu = 1.0, g["mu"]  # rel_bound_barrier = 1
    gam = 1000.0
    # residual of the perturbed KKT conditions (computeKKTRes :1337-1446); all constraints are inequalities
    rx = g["zl"] - g["zu"] - grad + A.T @ g["z"]
    rz = -(cons - g["s"] + g["t"])
    rs = -(0.0 - g["zs"] + g["z"])
    rt = -(gam - g["zt"] - g["z"])
    rzs = -(g["s"] * g["zs"] - mu)
    rzt = -(g["t"] * g["zt"] - mu)
    rzl = -((x - lb) * g["zl"] - beta * mu)
    rzu = -((ub - x) * g["zu"] - beta * mu)
    k = len(g["Z"])
    B = g["b0"] * np.eye(n)
    if k > 0:
        Zm = np.array(g["Z"]).T
        if qn == "bfgs":
            B -= (Zm * g["d0"]) @ np.linalg.solve(g["M"], (Zm * g["d0"]).T)
        else:
            B -= Zm @ np.linalg.solve(g["M"], Zm.T)
    # the step must zero the linearised residual (addKKTResStep :1451-1583)
    ex = rx - B @ p["x"] + A.T @ p["z"] + p["zl"] - p["zu"]
    ez = rz - (A @ p["x"] - p["s"] + p["t"])
    es = rs + (p["zs"] - p["z"])
    et = rt + (p["zt"] + p["z"])
    ezs = rzs - (p["s"] * g["zs"] + g["s"] * p["zs"])
    ezt = rzt - (p["t"] * g["zt"] + g["t"] * p["zt"])
    ezl = rzl - ((x - lb) * p["zl"] + p["x"] * g["zl"])
    ezu = rzu - ((ub - x) * p["zu"] - p["x"] * g["zu"])
    scale = max(1.0, np.abs(rx).max(), np.abs(rz).max(), np.abs(rzl).max(), np.abs(rzu).max())
    for name, e in (("x", ex), ("z", ez), ("s", es), ("t", et), ("zs", ezs), ("zt", ezt), ("zl", ezl), ("zu", ezu)):
        assert np.abs(e).max() <= 1e-9 * scale, (name, np.abs(e).max(), scale)


@pytest.mark.parametrize("form", ["weighting", "chain"])
def test_check_kkt_step_residual_sparse(ctx, form):
    """checkKKTStep with sparse constraints, block form (nwblock = 1) and CSR form (device sparse Cholesky): the
    fused step, including its five w-sized blocks, against the dense linearised KKT system in numpy."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po  # problem data only

    n, c = 240, 2
    if form == "weighting":
        data = po.SepProblem("convex", n, c, nwcon=39, nw=5, nwstart=3, nwskip=1)
        prob = pa.SeparableProblem(ctx, "convex", n, c).setWeighting(39, 5, 3, 1)
    else:
        data = po.SepProblem("convex", n, c, chain=(3, 2))
        prob = pa.SeparableProblem(ctx, "convex", n, c).setChain(3, 2)
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": 5, "max_major_iters": 7, "abs_res_tol": 1e-30,
                                 "penalty_gamma": 1000.0})
    g = {}

    def cb(k):
        if k != 6:
            return
        mu = ip.getBarrierParameter()
        x, z, zl, zu = ip.getOptimizedPoint()
        s, t, zs, zt = ip.getOptimizedSlacks()
        wv = [v.to_numpy() for v in ip.getOptimizedSparse()]
        b0, d0, M, Z = ip.getQuasiNewton().getCompactMat()
        g.update(mu=mu, x=x.to_numpy(), z=np.array(z), zl=zl.to_numpy(), zu=zu.to_numpy(), s=np.array(s),
                 t=np.array(t), zs=np.array(zs), zt=np.array(zt), w=wv, b0=b0, d0=d0, M=M,
                 Z=[v.to_numpy() for v in Z], p=ip.debugKKTStep(mu))

    ip.setIterationCallback(cb)
    ip.optimize()
    x, p = g["x"], g["p"]
    _, _, cons = data.eval_obj_con(x)
    _, grad, A = data.eval_obj_con_gradient(x)
    A = np.array(A)
    cw = data.eval_sparse_con(x)
    Aw = data.sparse_jacobian_dense()
    zw, sw, tw, zsw, ztw = g["w"]
    _, lb, ub = data.vars_and_bounds()
    mu, gam = g["mu"], 1000.0
    rx = g["zl"] - g["zu"] - grad + A.T @ g["z"] + Aw.T @ zw
    rz = -(cons - g["s"] + g["t"])
    rs, rt = -(0.0 - g["zs"] + g["z"]), -(gam - g["zt"] - g["z"])
    rzs, rzt = -(g["s"] * g["zs"] - mu), -(g["t"] * g["zt"] - mu)
    rzl, rzu = -((x - lb) * g["zl"] - mu), -((ub - x) * g["zu"] - mu)
    rzw = -(cw - sw + tw)
    rsw, rtw = zsw - 0.0 - zw, ztw - gam + zw  # all sparse constraints are inequalities: gamma_sw = 0
    rzsw, rztw = mu - sw * zsw, mu - tw * ztw
    Zm = np.array(g["Z"]).T
    B = g["b0"] * np.eye(n) - (Zm * g["d0"]) @ np.linalg.solve(g["M"], (Zm * g["d0"]).T)
    errs = {
        "x": rx - B @ p["x"] + A.T @ p["z"] + Aw.T @ p["zw"] + p["zl"] - p["zu"],
        "z": rz - (A @ p["x"] - p["s"] + p["t"]),
        "s": rs + (p["zs"] - p["z"]), "t": rt + (p["zt"] + p["z"]),
        "zs": rzs - (p["s"] * g["zs"] + g["s"] * p["zs"]), "zt": rzt - (p["t"] * g["zt"] + g["t"] * p["zt"]),
        "zl": rzl - ((x - lb) * p["zl"] + p["x"] * g["zl"]), "zu": rzu - ((ub - x) * p["zu"] - p["x"] * g["zu"]),
        # sparse rows (:1492-1527)
        "zw": rzw - (Aw @ p["x"] - p["sw"] + p["tw"]),
        "sw": rsw + (p["zsw"] - p["zw"]), "tw": rtw + (p["ztw"] + p["zw"]),
        "zsw": rzsw - (p["sw"] * zsw + sw * p["zsw"]), "ztw": rztw - (p["tw"] * ztw + tw * p["ztw"]),
    }
    scale = max(1.0, np.abs(rx).max(), np.abs(rzw).max(), np.abs(rz).max(), np.abs(rtw).max())
    for name, e in errs.items():
        assert np.abs(e).max() <= 1e-9 * scale, (form, name, np.abs(e).max(), scale)


@pytest.mark.parametrize("problem,qn,strategy,nw", [("convex", "sr1", "monotone", 0), ("quadratic", "bfgs", "monotone", 0),
                                                    ("convex", "bfgs", "mehrotra_predictor_corrector", 0),
                                                    ("rosenbrock", "bfgs", "monotone", 0),
                                                    ("convex", "bfgs", "monotone", 20),
                                                    ("quadratic", "sr1", "mehrotra", 5)])
def test_reduction_batching_changes_no_bit(problem, qn, strategy, nw):
    """Batched reductions (po_ctx_set_reduction_batching): trial-point barrier sums + f + c, and the next
    residual's norms + the quasi-Newton products, share one collective + host sync each.  The partial sums and the
    final stage are the same kernels, so every iterate is the same bits; only the number of host syncs drops."""
    import paropt_amd as pa

    opts = {"qn_type": qn, "qn_subspace_size": 6, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 30, "write_output_frequency": 0, "barrier_strategy": strategy,
            "qn_update_type": "damped_update"}
    runs = []
    for on in (False, True):
        c = pa.Context(0).set_reduction_batching(on)
        prob = pa.SeparableProblem(c, problem, 20000 if nw else 20011, 2 if problem == "rosenbrock" else 7)
        if nw:  # sparse (weighting) constraints: the w-sized reductions join the batches
            prob.setWeighting(20000 // nw // 2, nw, 0, nw)
            opts = dict(opts, penalty_gamma=1000.0, starting_point_strategy="affine_step")
        ip = pa.InteriorPoint(prob, opts)
        sn = []
        ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
        r0 = c.counters()[0]
        ip.optimize()
        runs.append((sn, ip.getOptimizedPoint()[0].to_numpy(), c.counters()[0] - r0, c.batched_reductions()))
    a, b = runs
    assert len(a[0]) == len(b[0]) and len(a[0]) >= 10
    for sa, sb in zip(a[0], b[0]):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["fobj"] == sb["fobj"] and sa["mu"] == sb["mu"]
        np.testing.assert_array_equal(sa["norms"], sb["norms"])
        np.testing.assert_array_equal(sa["z"], sb["z"])
        if nw:
            np.testing.assert_array_equal(sa["wnorms"], sb["wnorms"])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[3] == 0 and b[3] > 2 * len(b[0])
    # at least two host syncs fewer per iteration (three per quasi-Newton update + one per extra trial point)
    assert b[2] <= a[2] - 2 * (len(b[0]) - 1), (a[2], b[2])
    assert a[2] - b[2] == b[3]


@pytest.mark.parametrize("problem,qn,linear", [("convex", "sr1", True), ("convex", "bfgs", False),
                                               ("quadratic", "bfgs", True)])
def test_write_saving_fusions_against_their_plain_forms(monkeypatch, problem, qn, linear):
    """Round-2 fusions that exist to save HBM writes, each against the form it replaces (environment switch read when
    the solver is created):
    * PAROPT_AMD_NO_FUSED_UPDATE: bound-multiplier step + first bracket of y_qn inside the residual pass of the new
      point (kkt_res_update_kernel) vs update_mult_yqn + kkt_res -- the same arithmetic in the same order: every
      iterate is the same bits;
    * PAROPT_AMD_NO_RECOMPUTE: first solve pass stores no step, the refinement pass recomputes it (solve2r_kernel) vs
      stored and re-read -- the recomputed first step differs by the summation order of P alpha: same counters, state
      to 1e-9 over the compared window."""
    import paropt_amd as pa

    opts = {"qn_type": qn, "qn_subspace_size": 6, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": 22, "write_output_frequency": 0}

    def run(env):
        for k in ("PAROPT_AMD_NO_FUSED_UPDATE", "PAROPT_AMD_NO_RECOMPUTE", "PAROPT_AMD_NO_RECOMPUTE_RHS",
                  "PAROPT_AMD_NO_FUSED_MERIT", "PAROPT_AMD_NO_LEAN_STEP", "PAROPT_AMD_NO_RECOMPUTE_DT"):
            monkeypatch.delenv(k, raising=False)
        for k in env:
            monkeypatch.setenv(k, "1")
        c = pa.Context(0)
        prob = pa.SeparableProblem(c, problem, 20011, 7)
        prob.setLinearConstraints(linear)
        ip = pa.InteriorPoint(prob, opts)
        sn = []
        ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
        ip.optimize()
        return sn, ip.getOptimizedPoint()[0].to_numpy()

    base, xb = run([])
    # (the bit-for-bit statement is about the fused multiplier update alone: both runs store the bound-multiplier
    # steps -- the lean step of round 3, which needs the fused update, re-forms them with other round-off)
    stored, xs0 = run(["PAROPT_AMD_NO_LEAN_STEP"])
    plain_upd, xu = run(["PAROPT_AMD_NO_LEAN_STEP", "PAROPT_AMD_NO_FUSED_UPDATE"])
    assert len(base) == len(stored) == len(plain_upd) >= 10
    xb_lean, xb = xb, xs0
    for sa, sb in zip(stored, plain_upd):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["fobj"] == sb["fobj"] and sa["mu"] == sb["mu"]
        np.testing.assert_array_equal(sa["norms"], sb["norms"])
        np.testing.assert_array_equal(sa["z"], sb["z"])
    np.testing.assert_array_equal(xb, xu)
    # PAROPT_AMD_NO_RECOMPUTE_DT (round 3): the refinement pass READS Dinv and the first right-hand side t instead of
    # re-forming them from the bound data and rx it loads anyway -- the same expressions as dinv_d1_kernel: same bits
    read_dt, xr = run(["PAROPT_AMD_NO_RECOMPUTE_DT"])
    assert len(read_dt) == len(base)
    for sa, sb in zip(base, read_dt):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["fobj"] == sb["fobj"] and sa["mu"] == sb["mu"]
        np.testing.assert_array_equal(sa["norms"], sb["norms"])
        np.testing.assert_array_equal(sa["z"], sb["z"])
    np.testing.assert_array_equal(xb_lean, xr)
    window = 12 if qn == "sr1" else len(base)
    # ... PAROPT_AMD_NO_RECOMPUTE_RHS: only the step is recomputed, the refinement right-hand side is stored;
    # PAROPT_AMD_NO_FUSED_MERIT (round 3): the complementarity / merit sums of the final step in their own pass
    # (comp_merit_kernel) instead of inside the refinement pass (solve2r_kernel<.,1>, polynomial form of the
    # complementarity at the scaled step): sums in another order, same counters, state to 1e-9
    # PAROPT_AMD_NO_LEAN_STEP (round 3): the refinement pass stores the bound-multiplier steps (pzl, pzu) instead of
    # leaving them to be re-formed from px inside the multiplier update (they differ by the round-off the refinement
    # corrects)
    for switch in ("PAROPT_AMD_NO_RECOMPUTE", "PAROPT_AMD_NO_RECOMPUTE_RHS", "PAROPT_AMD_NO_FUSED_MERIT",
                   "PAROPT_AMD_NO_LEAN_STEP"):
        other, xs = run([switch])
        assert len(other) == len(base), switch
        for sa, sb in list(zip(base, other))[:window]:
            np.testing.assert_array_equal(sa["counters"], sb["counters"], err_msg=switch)
            assert abs(sa["fobj"] - sb["fobj"]) <= 1e-9 * max(1.0, abs(sb["fobj"])), switch
            np.testing.assert_allclose(sa["norms"], sb["norms"], rtol=1e-7, atol=1e-9, err_msg=switch)
            np.testing.assert_allclose(sa["z"], sb["z"], rtol=1e-6, atol=1e-9, err_msg=switch)


def test_host_writes_through_get_array_reach_the_solver(ctx):
    """multipliers seeded through getOptimizedPoint() + getArray() (the reference's pointer contents are
    used directly with starting_point_strategy = no_start_strategy, src/ParOptInteriorPoint.cpp:4577-4585) must not
    be dropped when optimize() ends the live state of the solver's mirrors."""
    import paropt_amd as pa

    n, c = 3001, 2
    opts = {"qn_subspace_size": 5, "abs_res_tol": 1e-8, "starting_point_strategy": "no_start_strategy",
            "max_major_iters": 3, "write_output_frequency": 0}

    def first_norms(seed_host):
        prob = pa.SeparableProblem(ctx, "quadratic", n, c)
        ip = pa.InteriorPoint(prob, opts)
        x, z, zl, zu = ip.getOptimizedPoint()
        if seed_host:
            a = zl.getArray()  # live host view of the solver's own vector
            a[:] = 0.25 + 0.5 * np.arange(n) / n
            b = zu.getArray()
            b[:] = 0.75
        else:
            zl.from_numpy(0.25 + 0.5 * np.arange(n) / n)
            zu.from_numpy(np.full(n, 0.75))
        seen = []
        ip.setIterationCallback(lambda k: seen.append(ip.snapshot()["norms"].copy()) if k == 0 else None)
        ip.optimize()
        return seen[0], ip.getOptimizedPoint()[0].to_numpy()

    n_host, x_host = first_norms(True)
    n_dev, x_dev = first_norms(False)
    expect_zl = np.linalg.norm(0.25 + 0.5 * np.arange(n) / n)
    assert abs(n_host[1] - expect_zl) <= 1e-12 * expect_zl and abs(n_host[2] - 0.75 * np.sqrt(n)) <= 1e-12 * n
    np.testing.assert_array_equal(n_host, n_dev)
    np.testing.assert_array_equal(x_host, x_dev)
@pytest.mark.gpu
@pytest.mark.parametrize("nwcon", [0, 40])
def test_check_merit_func_gradient_and_small_methods(ctx, nwcon, capfd):
    """VERDICT r3 missing #5: checkMeritFuncGradient (reference .cpp:3280-3432: the forward difference of the merit
    function along -g/|g| with its fixed slack steps agrees with evalMeritInitDeriv's derivative), checkGradients(dh),
    setBFGSUpdateType and setUseDiagHessian of ParOptInteriorPoint."""
    import paropt_amd as pa

    n, c = 400, 3
    prob = pa.SeparableProblem(ctx, "convex", n, c)
    if nwcon:
        prob.setWeighting(nwcon, 5, 3, 2)
    ip = pa.InteriorPoint(prob, {"qn_subspace_size": 4, "max_major_iters": 3, "write_output_frequency": 0})
    ip.optimize()
    x = ip.getOptimizedPoint()[0]
    xpt = pa.PVec(ctx, n).from_numpy(x.to_numpy())
    fd, actual = ip.checkMeritFuncGradient(xpt, 1e-7)
    assert abs(fd - actual) <= 2e-5 * max(1.0, abs(actual)), (fd, actual)
    out = capfd.readouterr().out
    assert "Merit function test" in out and "dm FD:" in out
    fd2, actual2 = ip.checkMeritFuncGradient(None, 1e-7)  # the step of the previous call is still in place
    assert abs(fd2 - actual2) <= 2e-5 * max(1.0, abs(actual2)), (fd2, actual2)
    rep = ip.checkGradients(1e-6)
    assert "Objective gradient test" in rep and "Constraint gradient test" in rep
    ip.setBFGSUpdateType("damped_update")
    ip.setUseDiagHessian(False)


@pytest.mark.gpu
def test_reset_design_and_bounds_wins_over_a_live_mirror(ctx, tmp_path):
    """a caller that still holds getArray views of the previous optimum calls resetDesignAndBounds() (or
    readSolutionFile()) and optimizes again.  The reference has ONE buffer: the reset is what the solve starts from and
    what the caller's pointer shows.  The live mirror must be refreshed by the internal writer, not uploaded over it."""
    import paropt_amd as pa

    n, c = 2001, 2
    opts = {"qn_subspace_size": 5, "abs_res_tol": 1e-8, "max_major_iters": 6, "write_output_frequency": 0}
    prob = pa.SeparableProblem(ctx, "quadratic", n, c)
    ip = pa.InteriorPoint(prob, opts)
    first = []
    ip.setIterationCallback(lambda k: first.append(ip.getOptimizedPoint()[0].to_numpy().copy()) if k == 0 else None)
    ip.optimize()
    x0 = first[0]                      # the point the first solve started from (after the bound checks)
    ckpt = str(tmp_path / "sol.bin")
    ip.writeSolutionFile(ckpt)
    x = ip.getOptimizedPoint()[0]
    xopt = x.to_numpy().copy()
    assert np.abs(xopt - x0).max() > 1e-3
    view = x.getArray()                # live host view of the solver's own vector: holds the optimum
    np.testing.assert_array_equal(view, xopt)
    ip.resetDesignAndBounds()
    np.testing.assert_array_equal(view, x.to_numpy())  # the caller's pointer shows the reset point ...
    assert np.abs(view - xopt).max() > 1e-3
    first.clear()
    ip.resetQuasiNewtonHessian()
    ip.optimize()
    np.testing.assert_array_equal(first[0], x0)        # ... and the solve starts from it, not from the stale mirror
    # the same through readSolutionFile: the restart point is the file's, also behind a live view
    view = ip.getOptimizedPoint()[0].getArray()
    view[:] = 0.123
    ip.readSolutionFile(ckpt)
    np.testing.assert_array_equal(view, xopt)

@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seq_lin_c3", "bfgs_c3", "quadratic_c2_large", "quadratic_odd_small", "no_line_search"])
def test_predictor_corrector_fused_corrector_against_its_plain_form(ctx, case):
    """Round 6: under mehrotra_predictor_corrector the corrector right-hand side is ONE pass (corr_d1_dots_kernel: the
    bits of corrector + d1 + mdot), the corrector solve takes the sums of scaleKKTStep / evalMeritInitDeriv itself
    (solve2c_kernel: same step, polynomial complementarity) and the affine step's complementarity comes from the
    polynomial its refinement pass took -- 3 launches and one to two host round trips per iteration less.  Against the
    plain sequence (debug switches 14 / 15 = 0) in the same process on convergent iterations: counters and table tokens
    equal, iterates to round-off (the merit sums are cut differently and the polynomial re-associates the
    complementarity: 1e-16-level changes in the barrier parameter and the merit derivative)."""
    import paropt_amd as pa
    from paropt_amd import lib as L

    SW_MPC_FUSE, SW_MPC_POLY = 14, 15
    cfg = {
        "seq_lin_c3": dict(kind="convex", n=20001, c=3, iters=16, opts={"qn_type": "bfgs", "qn_subspace_size": 3,
                                                                         "sequential_linear_method": True}),
        "bfgs_c3": dict(kind="quadratic", n=300, c=3, iters=30, opts={"qn_type": "bfgs", "qn_subspace_size": 10}),
        # (more than one pair per thread: the grids cover 2 x 256 x 4 x 256 and 2 x 256 x 5 x 256 elements per sweep)
        "quadratic_c2_large": dict(kind="quadratic", n=1200003, c=2, iters=24,
                                   opts={"qn_type": "bfgs", "qn_subspace_size": 3, "init_barrier_param": 1e-3}),
        "quadratic_odd_small": dict(kind="quadratic", n=511, c=2, iters=30, opts={"qn_type": "bfgs", "qn_subspace_size": 4,
                                                                                  "sequential_linear_method": True}),
        "no_line_search": dict(kind="quadratic", n=3001, c=3, iters=30, opts={"qn_type": "bfgs", "qn_subspace_size": 5,
                                                                              "use_line_search": False}),
    }[case]

    def run(fuse, poly):
        L.lib.po_debug_set_switch(SW_MPC_FUSE, fuse)
        L.lib.po_debug_set_switch(SW_MPC_POLY, poly)
        try:
            prob = pa.SeparableProblem(ctx, cfg["kind"], cfg["n"], cfg["c"], 5)
            # (every solve starts monotone, reference :4427-4441: the predictor-corrector takes over at the first
            # barrier reduction)
            ip = pa.InteriorPoint(prob, dict({"abs_res_tol": 1e-9, "start_affine_multiplier_min": 0.01,
                                              "max_major_iters": cfg["iters"],
                                              "barrier_strategy": "mehrotra_predictor_corrector",
                                              "write_output_frequency": 0}, **cfg["opts"]))
            sn = []
            ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
            n0 = ctx.counters()[1]
            ip.optimize()
            launches = ctx.counters()[1] - n0
            x, z, zl, zu = ip.getOptimizedPoint()[:4]
            return sn, x.to_numpy(), np.array(z), zl.to_numpy(), zu.to_numpy(), ip.getHistory(), launches
        finally:
            L.lib.po_debug_set_switch(SW_MPC_FUSE, -1)
            L.lib.po_debug_set_switch(SW_MPC_POLY, -1)

    a = run(0, 0)
    for fuse, poly in ((1, 0), (1, 1)):
        b = run(fuse, poly)
        assert b[6] < a[6], ("the predictor-corrector phase was not reached, or the fused path not taken", a[6], b[6])
        assert len(a[0]) == len(b[0]) >= 8
        for k, (sa, sb) in enumerate(zip(a[0], b[0])):
            np.testing.assert_array_equal(sa["counters"], sb["counters"], err_msg="counters @%d" % k)
            assert abs(sa["mu"] - sb["mu"]) <= 1e-9 * abs(sa["mu"]), (k, sa["mu"], sb["mu"])
            assert abs(sa["fobj"] - sb["fobj"]) <= 1e-9 * max(1.0, abs(sa["fobj"])), (k, sa["fobj"], sb["fobj"])
            np.testing.assert_allclose(sa["norms"], sb["norms"], rtol=1e-9)
        for va, vb in zip(a[1:5], b[1:5]):
            np.testing.assert_allclose(va, vb, rtol=0, atol=1e-8 * max(1.0, float(np.abs(va).max())))
        tokens = lambda h: [ln.split()[15:] for ln in h.splitlines() if ln[:5].strip().isdigit()]  # noqa: E731
        assert len(tokens(a[5])) >= 8 and tokens(a[5]) == tokens(b[5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seq_lin", "fixed_bfgs", "seq_lin_mpc", "odd_small"])
def test_dinv_and_rhs_left_by_the_residual_pass_keep_every_bit(ctx, case):
    """Round 6: when no quasi-Newton update follows the step (a fixed approximation -- the trust-region subproblem
    solves -- or the sequential linear method) the diagonal of the next KKT system is known when the residual of the new
    point is taken, and that pass (kkt_res_update_kernel) leaves Dinv and t = Dinv o d1 of the next first solve behind:
    setUpKKTSystem skips its pass over the bound data whenever diagonal and barrier parameter still match (they do not
    at a barrier switch: the plain pass runs).  Same expressions on the same operands: against the plain sequence
    (debug switch 16 = 0) in the same process every iterate, multiplier, norm, counter and table row has the same bits,
    with one launch less per iteration."""
    import paropt_amd as pa
    from paropt_amd import lib as L

    SW_SPEC_DT = 16
    cfg = {
        "seq_lin": dict(kind="convex", n=400003, c=3, iters=14, opts={"qn_type": "bfgs", "qn_subspace_size": 3,
                                                                       "sequential_linear_method": True}),
        "fixed_bfgs": dict(kind="quadratic", n=300001, c=4, iters=14,
                           opts={"qn_type": "bfgs", "qn_subspace_size": 4, "use_quasi_newton_update": False}),
        "seq_lin_mpc": dict(kind="convex", n=20001, c=3, iters=16,
                            opts={"qn_type": "bfgs", "qn_subspace_size": 3, "sequential_linear_method": True,
                                  "barrier_strategy": "mehrotra_predictor_corrector"}),
        "odd_small": dict(kind="quadratic", n=511, c=2, iters=30, opts={"qn_type": "bfgs", "qn_subspace_size": 4,
                                                                        "sequential_linear_method": True,
                                                                        "barrier_strategy": "mehrotra"}),
    }[case]

    def run(spec):
        L.lib.po_debug_set_switch(SW_SPEC_DT, spec)
        try:
            prob = pa.SeparableProblem(ctx, cfg["kind"], cfg["n"], cfg["c"], 7)
            ip = pa.InteriorPoint(prob, dict({"abs_res_tol": 1e-9, "start_affine_multiplier_min": 0.01,
                                              "max_major_iters": cfg["iters"], "write_output_frequency": 0}, **cfg["opts"]))
            sn = []
            ip.setIterationCallback(lambda k: sn.append(ip.snapshot()))
            n0 = ctx.counters()[1]
            ip.optimize()
            launches = ctx.counters()[1] - n0
            x, z, zl, zu = ip.getOptimizedPoint()[:4]
            return sn, x.to_numpy(), np.array(z), zl.to_numpy(), zu.to_numpy(), ip.getHistory(), launches
        finally:
            L.lib.po_debug_set_switch(SW_SPEC_DT, -1)

    a, b = run(0), run(1)
    assert len(a[0]) == len(b[0]) >= 8
    assert b[6] <= a[6] - (len(a[0]) - 4), ("one launch less in (nearly) every iteration", a[6], b[6], len(a[0]))
    for sa, sb in zip(a[0], b[0]):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa["fobj"] == sb["fobj"] and sa["mu"] == sb["mu"]
        np.testing.assert_array_equal(sa["norms"], sb["norms"])
    for va, vb in zip(a[1:5], b[1:5]):
        np.testing.assert_array_equal(va, vb)
    table = lambda h: [ln for ln in h.splitlines() if ln[:5].strip().isdigit()]  # noqa: E731
    assert len(table(a[5])) >= 8 and table(a[5]) == table(b[5])


# The four bench shapes at n = 2001, each a fixed-length solve (abs_res_tol out of reach).  launches / syncs: what
# optimize() adds to Context.counters() -- taken with tools/ip_digest.py from the library of the commit BEFORE the host
# code of the solve passes was restructured (profiles/r15_ip_digest_parent.jsonl), not from the build under
# test: a restructuring of the host code may not add, drop or reorder a launch or a host round trip.
_FIXED = {"abs_res_tol": 1e-30, "start_affine_multiplier_min": 0.01, "max_major_iters": 12}
ON_RECORD = {
    "config2": dict(ip=dict(problem="quadratic", n=2001, c=8, wt=None,
                            opts=dict(_FIXED, qn_type="bfgs", qn_subspace_size=20)), launches=245, syncs=72),
    "config3": dict(ip=dict(problem="convex", n=2001, c=32, wt=None,
                            opts=dict(_FIXED, qn_type="sr1", qn_subspace_size=10)), launches=241, syncs=71),
    "config4": dict(ip=dict(problem="convex", n=2001, c=4, wt=(100, 20, 0, 0, 100),
                            opts=dict(_FIXED, qn_type="bfgs", qn_subspace_size=10)), launches=548, syncs=90),
    "config5": dict(tr=dict(problem="quadratic", n=2001, c=4, eig=(10, 0, 0, 2.0),
                            opts={"qn_subspace_size": 10, "tr_max_iterations": 4, "max_major_iters": 200}),
                    launches=3709, syncs=1368),
    # One case per branch of the driver (optimize(), lineSearch(), computeStepAndUpdate()): a golden's own case record,
    # with `extra` options where no golden takes the branch; `tokens`: what the info column has to show for the case to
    # be still on its branch.  launches / syncs: printed by tools/ip_digest.py with the library of the commit BEFORE
    # optimize() was cut into stages (profiles/r27_ip_digest_parent.jsonl).
    "line_search_failure_reset_rebuilt_trial": dict(golden="ip_quadratic_clamp_n200_c2",
                                                    tokens=("LFail", "resetH", "LMxItr"), launches=1225, syncs=340),
    "newton_krylov_min_step": dict(golden="ip_convex_hvec_noprecon_n200_c2", tokens=("iNK", "LMnStp", "skipH"),
                                   launches=19409, syncs=6157),
    "no_line_search": dict(golden="ip_quadratic_nolinesearch_n200_c2", launches=877, syncs=291),
    "complementarity_fraction": dict(golden="ip_quadratic_compfrac_n200_c2", tokens=("LNoImprv",),
                                     launches=1061, syncs=333),
    "mehrotra_comp_equal_step": dict(golden="ip_rosenbrock_mehrotra_n100", tokens=("cmpEq",), launches=717, syncs=248),
    "damped_update": dict(golden="ip_convex_nolower_n200_c2", extra={"qn_update_type": "damped_update"},
                          tokens=("dampH",), launches=509, syncs=148),
    "fixed_lbfgs_diagonal_step": dict(golden="ip_quadratic_clamp_n200_c2",
                                      extra={"use_quasi_newton_update": 0, "max_line_iters": 1},
                                      tokens=("DQN", "LFail"), launches=578, syncs=210),
    "no_approximation_sequential_linear_step": dict(golden="ip_quadratic_clamp_n200_c2",
                                                    extra={"use_quasi_newton_update": 0, "max_line_iters": 1,
                                                           "qn_type": "none", "use_diag_hessian": 1},
                                                    tokens=("SLP", "LFail"), launches=1005, syncs=330),
}


def golden_case(name, **extra):
    """the case record of a golden, with interior-point options added or replaced"""
    case = load_golden(name)[1]
    case["args"].update({"opt." + k: v for k, v in extra.items()})
    return case


@pytest.mark.parametrize("name", sorted(ON_RECORD))
def test_launches_and_syncs_of_the_configurations_on_record(ctx, name):
    import paropt_amd as pa

    rec = ON_RECORD[name]
    if "golden" in rec:
        prob, solver = build_gpu(ctx, golden_case(rec["golden"], **rec.get("extra", {})))
    else:
        a = rec.get("ip") or rec["tr"]
        prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"])
        if "tr" in rec:
            solver = pa.TrustRegion(prob, a["opts"])
            solver.setEigenModelSynthetic(*a["eig"])
        else:
            if a["wt"]:
                prob.setWeighting(*a["wt"])
            solver = pa.InteriorPoint(prob, dict(a["opts"], write_output_frequency=0))
    syncs0, launches0 = ctx.counters()
    solver.optimize()
    syncs1, launches1 = ctx.counters()
    assert (launches1 - launches0, syncs1 - syncs0) == (rec["launches"], rec["syncs"])
    # a case that is here for a branch of the driver has to keep reaching it ("iNK": the token carries a count)
    seen = {t for row in info_tokens(solver.getHistory()).values() for t in row}
    for token in rec.get("tokens", ()):
        assert any(t == token or (token == "iNK" and t.startswith("iNK")) for t in seen), (token, sorted(seen))
