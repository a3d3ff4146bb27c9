"""
Digest of the interior point, one JSON line per configuration: the iteration history, SHA-256 of x, zl, zu (and the five
sparse blocks), z, the iteration counters, and what optimize() added to the context's counters -- kernel launches,
host-synchronising reductions, polled completions / collectives, batched reductions, algorithmic bytes.  Two libraries
compute the same thing bit for bit, with the same launches, exactly when their outputs are byte-identical:

    PAROPT_AMD_LIB=<one libparopt_amd.so> python tools/ip_digest.py > a.jsonl
    PAROPT_AMD_LIB=<another>              python tools/ip_digest.py > b.jsonl
    cmp a.jsonl b.jsonl

--brief prints, per configuration, the iteration counters, the counter deltas and the SHA-256 of the full line instead of
the line itself (the form kept under profiles/): equal files still mean equal full outputs.

Configurations, all at 6-14 iterations: the size-and-option sweep and the configurations on record of
tests/test_gpu_ip.py (imported, not copied); the sizes at which setUpKKTSystem / solveKKT choose another form (L-SR1
columns formed in the Gram pass: at most 12; Gram panel with t: kWgramMaxVecs = 80; fused corrector: kCorrDotsMax = 15;
one kernel's argument tables: kMaxPanel = 96; no dense constraint; sequential linear method; a fixed quasi-Newton
approximation; linear constraints); four TrustRegion iterations on a quadratic and on an eigenvalue subproblem (the table
without its wall-clock column); a dense and a weighting problem under each test switch that selects a kernel form; every
golden of tests/test_gpu_ip.py's IP_CASES with n <= 2049 at its own options and length (between them they reach the info
tokens skipH, resetH, LFail, LMxItr, LNoImprv, iNK, LMnStp, cmpEq); and driver_branches(), small configurations that
reach three of the four tokens no golden reaches (dampH, DQN, SLP; no small configuration tried reached LSkip, HISTORY
R27.2) and the periodic work at the head of an iteration.  Every interior-point record also lists its phase names in
order of first appearance.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sparse_digest import without_time  # noqa: E402

BASE = {"abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01}
MPC = {"barrier_strategy": "mehrotra_predictor_corrector"}
SEQ_LIN = {"sequential_linear_method": True}
WEIGHTING = (51, 7, 3, 3, 51)


def spec(name, problem, n, c, qn="bfgs", m=5, iters=10, extra=None, wt=None, linear=False):
    opts = dict(BASE, qn_type=qn, qn_subspace_size=m, max_major_iters=iters)
    opts.update(extra or {})
    return dict(name=name, problem=problem, n=n, c=c, opts=opts, wt=wt, linear=linear)


def boundaries():
    # L-BFGS(m) brings 2 m panel columns once m updates are stored, L-SR1(m) one per update
    return [
        spec("lsr1_12_columns", "convex", 513, 3, "sr1", 12, 14),
        spec("lsr1_13_columns", "convex", 513, 3, "sr1", 13, 14),
        spec("gram_panel_80", "convex", 701, 69, iters=8),
        spec("gram_panel_81", "convex", 701, 70, iters=8),
        spec("mpc_panel_1", "convex", 257, 1, iters=14, extra=dict(MPC, **SEQ_LIN)),
        spec("mpc_panel_15", "quadratic", 769, 5, iters=14, extra=MPC),
        spec("mpc_panel_16", "quadratic", 769, 6, iters=14, extra=MPC),
        spec("panel_96", "convex", 901, 86, iters=8),
        spec("panel_97", "convex", 901, 87, iters=8),
        spec("no_dense_constraint", "quadratic", 1025, 0, iters=10),
        spec("no_dense_constraint_lsr1", "convex", 511, 0, "sr1", 4, 8),
        spec("seq_lin", "convex", 1001, 3, iters=12, extra=SEQ_LIN),
        spec("seq_lin_mpc", "convex", 1001, 3, iters=14, extra=dict(MPC, **SEQ_LIN)),
        spec("fixed_lbfgs", "quadratic", 1024, 4, m=4, iters=12, extra={"use_quasi_newton_update": False}),
        spec("linear_constraints", "convex", 999, 7, "sr1", 6, 8, linear=True),
        spec("linear_constraints_lbfgs", "quadratic", 640, 7, iters=12, linear=True),
    ]


def driver_branches():
    """(name, golden whose case it starts from, options added) -- branches of optimize() that no golden takes"""
    fixed = {"use_quasi_newton_update": 0}
    return [
        # a fixed L-BFGS whose line search fails (one or two trial points, the clamp goldens' design_precision): the
        # next step keeps only the diagonal of the approximation (DQN)
        ("fixed_lbfgs_clamp_quadratic_line1", "ip_quadratic_clamp_n200_c2", dict(fixed, max_line_iters=1)),
        ("fixed_lbfgs_clamp_convex_line2", "ip_convex_clamp_n300_c3", dict(fixed, max_line_iters=2)),
        # ... and with no approximation at all (diagonal Hessian) it is a sequential linear step (SLP)
        ("no_qn_diag_hessian_clamp_quadratic_line1", "ip_quadratic_clamp_n200_c2",
         dict(fixed, max_line_iters=1, qn_type="none", use_diag_hessian=1)),
        # damped BFGS update (dampH)
        ("damped_convex_badbounds7", "ip_convex_badbounds7_n300_c3", {"qn_update_type": "damped_update"}),
        ("damped_convex_nolower", "ip_convex_nolower_n200_c2", {"qn_update_type": "damped_update"}),
        # the periodic work at the head of an iteration
        ("hessian_reset_freq_4", "ip_convex_n300_c5_bfgs", {"hessian_reset_freq": 4, "max_major_iters": 14}),
        ("gradient_verification_3", "ip_quadratic_n257_c3_bfgs", {"gradient_verification_frequency": 3,
                                                                  "max_major_iters": 8}),
        ("step_verification_3", "ip_quadratic_n257_c3_bfgs", {"step_verification_frequency": 3,
                                                              "max_major_iters": 8}),
        ("step_verification_3_mpc", "ip_quadratic_mpc_n300_c3", {"step_verification_frequency": 3,
                                                                 "max_major_iters": 8}),
    ]


# (switch of core.hpp, its number, the value that leaves the default form, options under which it is reached)
SWITCHES = [("SW_EXPLICIT_DOTS", 20, 1, {}), ("SW_NO_RECOMPUTE", 21, 1, {}), ("SW_NO_RECOMPUTE_RHS", 22, 1, {}),
            ("SW_NO_FUSED_MERIT", 23, 1, {}), ("SW_NO_LEAN_STEP", 24, 1, {}), ("SW_NO_RECOMPUTE_DT", 25, 1, {}),
            ("SW_NO_FUSED_UPDATE", 26, 1, {}), ("SW_MPC_FUSE", 14, 0, MPC), ("SW_SPEC_DT", 16, 0, SEQ_LIN)]


def helpers(ctx, brief, brief_keys=("config", "switch", "iteration_counters", "deltas")):
    """(counters, delta, emit) of a digest over `ctx` (shared with tools/tr_digest.py)"""

    def emit(**rec):
        line = json.dumps(rec, sort_keys=True)
        if brief:
            keep = {k: rec[k] for k in brief_keys if k in rec}
            line = json.dumps(dict(keep, sha256_of_line=hashlib.sha256(line.encode()).hexdigest()), sort_keys=True)
        print(line, flush=True)

    def counters():
        syncs, launches = ctx.counters()
        return dict(ctx.sync_counters(), syncs=syncs, launches=launches, batched=ctx.batched_reductions(),
                    bytes=ctx.algorithmic_bytes()[0])

    def delta(before):
        after = counters()
        return {k: after[k] - before[k] for k in sorted(after)}

    return counters, delta, emit


def main():
    import numpy as np

    import paropt_amd as pa
    import sparse_forms_helpers as H
    from paropt_amd import lib as L
    from test_gpu_ip import IP_CASES, ON_RECORD, SWEEP, build_gpu, golden_case

    ctx = pa.Context(0)

    counters, delta, emit = helpers(ctx, "--brief" in sys.argv[1:])

    def solve_and_emit(ip, name, **tags):
        before = counters()
        ip.optimize()
        d = delta(before)
        x, z, zl, zu = ip.getOptimizedPoint()
        vecs = [("x", x), ("zl", zl), ("zu", zu)]
        sparse = ip.getOptimizedSparse()
        if sparse is not None:
            vecs += list(zip(("zw", "sw", "tw", "zsw", "ztw"), sparse))
        emit(config=name, history=ip.getHistory(), z=np.asarray(z).tolist(), deltas=d,
             iteration_counters=list(ip.getIterationCounters()), phases=list(ip.getPhaseTimes()),
             sha256={k: H.sha(v.to_numpy()) for k, v in vecs if v is not None}, **tags)

    def run_ip(s, **tags):
        prob = pa.SeparableProblem(ctx, s["problem"], s["n"], s["c"])
        if s["wt"]:
            prob.setWeighting(*s["wt"])
        if s["linear"]:
            prob.setLinearConstraints(True)
        solve_and_emit(pa.InteriorPoint(prob, dict(s["opts"], write_output_frequency=0)), s["name"], **tags)

    def run_golden(name, case):
        prob, ip = build_gpu(ctx, case)
        solve_and_emit(ip, name)

    for name in IP_CASES:
        case = golden_case(name)
        if case["args"]["n"] <= 2049:
            run_golden("golden_" + name, case)
    for name, golden, extra in driver_branches():
        run_golden(name, golden_case(golden, **extra))
    for i, (problem, n, c, qn, m, extra, wt) in enumerate(SWEEP):
        run_ip(spec("sweep_%02d" % i, problem, n, c, qn, m, 8 if qn == "sr1" else 14, extra, wt))
    for s in boundaries():
        run_ip(s)
    for name, rec in sorted(ON_RECORD.items()):
        if "ip" in rec:
            run_ip(dict(rec["ip"], name=name, linear=False))

    def run_tr(name, problem, n, c, opts, eig=None):
        tr = pa.TrustRegion(pa.SeparableProblem(ctx, problem, n, c), dict(opts))
        if eig:
            tr.setEigenModelSynthetic(*eig)
        before = counters()
        tr.optimize()
        d = delta(before)
        x, z = tr.getOptimizedPoint()[:2]
        emit(config=name, history=without_time(tr.getHistory()), z=np.asarray(z).tolist(), deltas=d,
             sha256={"x": H.sha(x.to_numpy())})

    run_tr("tr_quadratic", "quadratic", 1001, 3, {"tr_max_iterations": 4, "qn_subspace_size": 4})
    run_tr("tr_eigenvalue", "quadratic", 1001, 4, {"tr_max_iterations": 4, "qn_subspace_size": 10,
                                                    "max_major_iters": 200}, eig=(10, 0, 0, 2.0))
    for name, rec in sorted(ON_RECORD.items()):
        if "tr" in rec:
            run_tr(name, **rec["tr"])

    for sw, number, value, extra in SWITCHES:
        for s in (spec("dense", "convex", 1025, 7, "sr1", 6, 12, extra),
                  spec("weighting", "convex", 513, 2, "bfgs", 5, 12, extra, WEIGHTING)):
            L.lib.po_debug_set_switch(number, value)  # (read when the solver is constructed)
            try:
                run_ip(s, switch="%s=%d" % (sw, value))
            finally:
                L.lib.po_debug_set_switch(number, -1)
    ctx.close()


if __name__ == "__main__":
    main()
