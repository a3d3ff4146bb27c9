"""
MMA with its two sub-solvers on one MI355X: the built-in `convex` problem at (n = 10 M, c = 8) and (n = 50 M, c = 32).
In ONE process the interior-point sub-solver (the reference's way) and the dual sub-solver alternate, three rounds of a
few MMA iterations each; then one evaluation of the dual is timed beside the trivial kernel of its stream mix
(po_bench_mma_dual).  One JSON line per run, appended to profiles/r09_bench_mma.jsonl (--out), whatever comes out.

    python tools/bench_mma.py [--shapes 10000000x8,50000000x32] [--mma-iters 4] [--rounds 3] [--out FILE]

--globalization conservative: the dual sub-solver without and with the conservative inner loop alternate instead (ms
per MMA iteration and per inner raise, evaluations per solve), and the dual pass is timed beside its rho form and the
trivial kernel of the rho form's mix, 2m + 7 in (po_bench_mma_dual_rho; profiles/r10_bench_gcmma.jsonl).  --problem
picks the built-in problem of the whole runs.  --small: instead, whole runs to the stop test on small problems
(--shapes 300x3,200x2, dual tolerance 1e-9, at most --mma-iters iterations, default there 120) with and without the
inner loop: iterations, raises, cap hits, rises of fobj (the `convex_small` lines).

--nw NW [--nwcon W]: weighting constraints (W groups of NW consecutive variables, default n / NW) stay in the dual
(mma_dual_sparse_constraints = groups): whole MMA iterations with the interior-point sub-solver and with the grouped
dual alternate, then on the subproblem the last run left the grouped evaluation (po_mma_dual_group_eval) and the plain
evaluation of the same shape without groups (po_mma_dual_eval, panel form) alternate, wall time and algorithmic bytes
per call (both calls allocate their work vectors: the same m + 1 of n; the grouped one m + 1 of w besides).  Appended
to profiles/r12_bench_mma_groups.jsonl.

--nw NW [--nwcon W] --globalization conservative: the grouped dual without and with the conservative inner loop
(mma_gcmma_sparse_constraints = groups) alternate instead: ms per MMA iteration, raises, cap hits of the inner loop and
of the root searches, dual evaluations per solve.  Then on the last subproblem the grouped evaluation without and with
rho (po_mma_dual_group_eval / _rho; the rho form once with rho = 0, which is the same point and the same searches as
the plain form, so that it prices the form alone, and once with the run's rho) alternate, and the point of a trial
(po_mma_gcmma_group_point: the group solve and the read-only sums pass) is timed beside them.  Appended to profiles/r14_bench_mma_gcmma_groups.jsonl.

--linearized: mma_use_constraint_linearization = 1.  Whole MMA iterations with the interior-point sub-solver and with
the dual of the linearised subproblem (mma_dual_linearized_constraints = newton) alternate; then the linear pass
(po_bench_mma_dual_linear: root searches started warm, from the point of the call before, and cold, from the expansion
point) and the rational pass (po_bench_mma_dual) alternate at the same (n, m): ms, GB/s over the algorithmic m + 9
(m + 10 in the panel form) streams and the fraction of 8 TB/s.  Appended to profiles/r16_bench_mma_linear.jsonl.

--dual-only: the whole runs that alternate with the interior-point sub-solver (the default, --nw, --linearized) leave it
out: what a comparison of two builds of the dual's host code needs, at a hundredth of the time.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
M_F = 8


def run_mma(pa, ctx, n, c, solver, iters, globalization="none", problem="convex", linearized=False):
    prob = pa.SeparableProblem(ctx, problem, n, c, 0)
    opts = {"mma_subproblem_solver": solver, "mma_max_iterations": iters, "mma_l1_tol": 0.0,
            "mma_linfty_tol": 0.0, "write_output_frequency": 0, "mma_globalization": globalization}
    if linearized:
        opts.update(mma_use_constraint_linearization=1, mma_dual_linearized_constraints="newton")
    mma = pa.MMA(prob, opts)
    stamps = []
    # (the callback follows the reductions of the table row, which the host has waited for: nothing is in flight)
    mma.setIterationCallback(lambda k: stamps.append(time.perf_counter()))
    mma.optimize()
    st = mma.getState()
    its = len(stamps) - 1  # MMA iterations between the first and the last table row
    ms = (stamps[-1] - stamps[0]) / max(1, its) * 1e3
    out = dict(solver=solver, mma_iterations=its, ms_per_mma_iteration=ms,
               subproblem_evaluations_per_mma_iteration=st["subproblem_iter"] / max(1, its), fobj=st["fobj"],
               vectors=pa.live_objects()[0], GB=pa.live_objects()[1] * 1e-9)
    if solver == "dual":
        out["dual_stats"] = ds = mma.getDualStats()
        out["evaluations_per_solve"] = ds["evaluations"] / max(1, ds["solves"])
        gs = mma.getGlobalizationStats()
        out.update(globalization=globalization, inner_total=gs["inner_total"], inner_max=gs["inner_max"],
                   cap_hits=gs["cap_hits"], rho=gs["rho"].tolist())
        if linearized:
            out["linear_stats"] = mma.getDualLinearStats()
    return out


def linear_pass_lines(pa, ctx, n, c, reps, rounds):
    """The linear pass (warm and cold starts of the root searches) and the rational pass, alternating in one process."""
    lines = []
    for form in ([1, 2] if c <= M_F else [2]):
        for rnd in range(rounds):
            warm, cold, gram_l, ceil_l, steps = pa.bench_mma_dual_linear(ctx, n, c, form, reps)
            rat_ms, gram_r, ceil_r = pa.bench_mma_dual(ctx, n, c, form, reps)
            streams = c + 9 + (1 if form == 2 else 0)
            gb = 8.0 * streams * n * 1e-9
            gb_r = 8.0 * (2 * c + 6 + (c + 1 if form == 2 else 0)) * n * 1e-9
            r = dict(kind="dual_linear_pass", n=n, c=c, form=form, round=rnd,
                     mix="%d in / %d out" % (c + 8, 2 if form == 2 else 1), alg_GB=gb, warm_ms=warm, cold_ms=cold,
                     gram_ms=gram_l, trivial_ms=ceil_l, max_root_steps_warm_cold=steps,
                     warm_GBps=gb / (warm * 1e-3), cold_GBps=gb / (cold * 1e-3),
                     warm_frac_hbm_8TBps=gb / (warm * 1e-3) / HBM_PEAK_GBPS,
                     cold_frac_hbm_8TBps=gb / (cold * 1e-3) / HBM_PEAK_GBPS, warm_frac_of_trivial=ceil_l / warm,
                     rational_alg_GB=gb_r, rational_ms=rat_ms, rational_gram_ms=gram_r, rational_trivial_ms=ceil_r,
                     rational_frac_hbm_8TBps=gb_r / (rat_ms * 1e-3) / HBM_PEAK_GBPS,
                     warm_over_rational=(warm + gram_l) / (rat_ms + gram_r),
                     cold_over_rational=(cold + gram_l) / (rat_ms + gram_r))
            lines.append(r)
            print(json.dumps(r), flush=True)
    return lines


def group_lines(pa, ctx, n, c, nwcon, nw, iters, rounds, reps, solvers):
    """Whole runs (interior point / grouped dual, alternating), then the two evaluations on the last subproblem."""
    lines = []
    mma = None
    for rnd in range(rounds):
        for solver in solvers:
            mma = None  # (one solver's vectors at a time)
            prob = pa.SeparableProblem(ctx, "convex", n, c, 0).setWeighting(nwcon, nw, 0, 0)
            mma = pa.MMA(prob, {"mma_subproblem_solver": solver, "mma_dual_sparse_constraints": "groups",
                                "mma_max_iterations": iters, "mma_l1_tol": 0.0, "mma_linfty_tol": 0.0,
                                "write_output_frequency": 0})
            stamps = []
            mma.setIterationCallback(lambda k: stamps.append(time.perf_counter()))
            mma.optimize()
            st = mma.getState()
            its = len(stamps) - 1
            r = dict(kind="mma_groups", n=n, c=c, nwcon=nwcon, nw=nw, round=rnd, solver=solver, mma_iterations=its,
                     ms_per_mma_iteration=(stamps[-1] - stamps[0]) / max(1, its) * 1e3,
                     subproblem_evaluations_per_mma_iteration=st["subproblem_iter"] / max(1, its), fobj=st["fobj"],
                     vectors=pa.live_objects()[0], GB=pa.live_objects()[1] * 1e-9)
            if solver == "dual":
                r.update(dual_stats=mma.getDualStats(), group_stats=mma.getDualGroupStats())
            lines.append(r)
            print(json.dumps(r), flush=True)
    # the evaluations on the subproblem of the last (dual) run, at its multipliers
    import numpy as np

    s = mma.getSubproblem()
    lo, up = mma.getAsymptotes()
    lam = mma.getOptimizedPoint()[1]
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    zw = pa.PVec(ctx, nwcon)
    cvec = pa.PVec(ctx, nwcon).from_numpy(np.ones(nwcon))  # cw = 1 - sum x is linear: psi is the constraint itself
    head = (ctx, lo, up, s["alpha"], s["beta"], s["p0"], s["q0"], s["p"], s["q"], s["b"], lam)

    def timed(fn):
        ctx.synchronize()
        b0 = ctx.algorithmic_bytes()[0]
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, ctx.algorithmic_bytes()[0] - b0, out

    plain, grouped, stats = [], [], None
    for _ in range(reps + 1):  # (the first pair warms up)
        ms_p, by_p, _ = timed(lambda: pa.mma_dual_eval(*head, form=2))
        ms_g, by_g, out = timed(lambda: pa.mma_dual_group_eval(*head, nwcon, nw, 0, 0, -1.0, cvec, nwcon, 1000.0, pt, zw))
        plain.append(ms_p)
        grouped.append(ms_g)
        stats = out[3]
    r = dict(kind="dual_group_eval", n=n, c=c, nwcon=nwcon, nw=nw, plain_ms=plain[1:], grouped_ms=grouped[1:],
             plain_streams=by_p / (8.0 * n), grouped_streams=by_g / (8.0 * n),
             plain_frac_hbm_8TBps=by_p * 1e-9 / (min(plain[1:]) * 1e-3) / HBM_PEAK_GBPS,
             grouped_frac_hbm_8TBps=by_g * 1e-9 / (min(grouped[1:]) * 1e-3) / HBM_PEAK_GBPS,
             grouped_over_plain=min(grouped[1:]) / min(plain[1:]), predicted_by_bytes=by_g / by_p,
             inner_mean=stats["steps"] / max(1, nwcon), inner_max=stats["max_inner"], group_stats=stats)
    lines.append(r)
    print(json.dumps(r), flush=True)
    return lines


def gcmma_group_lines(pa, ctx, n, c, nwcon, nw, iters, rounds, reps, problem):
    """Whole runs of the grouped dual (none / conservative, alternating), then the evaluations on the last subproblem."""
    import numpy as np

    lines = []
    mma = None
    for rnd in range(rounds):
        for glob in ("none", "conservative"):
            mma = None  # (one solver's vectors at a time)
            prob = pa.SeparableProblem(ctx, problem, n, c, 0).setWeighting(nwcon, nw, 0, 0)
            mma = pa.MMA(prob, {"mma_subproblem_solver": "dual", "mma_dual_sparse_constraints": "groups",
                                "mma_globalization": glob, "mma_gcmma_sparse_constraints": "groups",
                                "mma_max_iterations": iters, "mma_l1_tol": 0.0, "mma_linfty_tol": 0.0,
                                "write_output_frequency": 0})
            stamps, root_caps = [], []
            mma.setIterationCallback(lambda k: (stamps.append(time.perf_counter()),
                                                root_caps.append(mma.getDualGroupStats()["cap_hits"])))
            mma.optimize()
            st, ds, gs = mma.getState(), mma.getDualStats(), mma.getGlobalizationStats()
            its = len(stamps) - 1
            r = dict(kind="mma_gcmma_groups", problem=problem, n=n, c=c, nwcon=nwcon, nw=nw, round=rnd,
                     globalization=glob, mma_iterations=its,
                     ms_per_mma_iteration=(stamps[-1] - stamps[0]) / max(1, its) * 1e3, fobj=st["fobj"],
                     evaluations_per_solve=ds["evaluations"] / max(1, ds["solves"]), dual_stats=ds,
                     inner_total=gs["inner_total"], inner_max=gs["inner_max"], cap_hits=gs["cap_hits"],
                     root_search_cap_hits=sum(root_caps[1:]), rho=gs["rho"].tolist(),
                     group_stats=mma.getDualGroupStats(), vectors=pa.live_objects()[0], GB=pa.live_objects()[1] * 1e-9)
            lines.append(r)
            print(json.dumps(r), flush=True)
    # the evaluations on the subproblem of the last (conservative) run, at its multipliers and its rho; the expansion
    # point of that subproblem is gone, the accepted point stands in for it
    s = mma.getSubproblem()
    lo, up = mma.getAsymptotes()
    xk, lam = mma.getOptimizedPoint()[0], mma.getOptimizedPoint()[1]
    rho = mma.getGlobalizationStats()["rho"]
    pt = [pa.PVec(ctx, n) for _ in range(3)]
    zw = pa.PVec(ctx, nwcon)
    cvec = pa.PVec(ctx, nwcon).from_numpy(np.ones(nwcon))  # cw = 1 - sum x is linear: psi is the constraint itself
    sub = (ctx, lo, up, s["alpha"], s["beta"], s["p0"], s["q0"], s["p"], s["q"])
    groups = (nwcon, nw, 0, 0, -1.0, cvec, nwcon, 1000.0)

    def timed(fn):
        ctx.synchronize()
        b0 = ctx.algorithmic_bytes()[0]
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, ctx.algorithmic_bytes()[0] - b0, out

    plain, rho_zero, with_rho, point = [], [], [], []
    zero = np.zeros(c + 1)
    for _ in range(reps + 1):  # (the first round warms up)
        ms_p, by_p, out_p = timed(lambda: pa.mma_dual_group_eval(*sub, s["b"], lam, *groups, pt, zw))
        ms_z, by_z, out_z = timed(lambda: pa.mma_dual_group_eval(*sub, s["b"], lam, *groups, pt, zw, xk=xk, rho=zero))
        ms_r, by_r, out_r = timed(lambda: pa.mma_dual_group_eval(*sub, s["b"], lam, *groups, pt, zw, xk=xk, rho=rho))
        ms_t, by_t, out_t = timed(lambda: pa.mma_gcmma_group_point(*sub, lam, *groups, xk, rho, pt, zw))
        plain.append(ms_p)
        rho_zero.append(ms_z)
        with_rho.append(ms_r)
        point.append(ms_t)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    r = dict(kind="dual_group_eval_rho", problem=problem, n=n, c=c, nwcon=nwcon, nw=nw, plain_ms=plain[1:],
             rho_zero_ms=rho_zero[1:], rho_ms=with_rho[1:], point_ms=point[1:], plain_streams=by_p / (8.0 * n),
             rho_streams=by_r / (8.0 * n), point_streams=by_t / (8.0 * n),
             rho_zero_over_plain=med(rho_zero[1:]) / med(plain[1:]), predicted_by_bytes=by_z / by_p,
             spread_plain=(max(plain[1:]) - min(plain[1:])) / min(plain[1:]),
             spread_rho_zero=(max(rho_zero[1:]) - min(rho_zero[1:])) / min(rho_zero[1:]),
             same_point=bool(out_z[3] == out_p[3] and out_z[0] == out_p[0]),
             plain_stats=out_p[3], rho_stats=out_r[3], point_stats=out_t[1])
    lines.append(r)
    print(json.dumps(r), flush=True)
    return lines


def small_run_lines(pa, ctx, n, c, iters, problem):
    """Whole runs to the stop test with and without the conservative inner loop."""
    lines = []
    for glob in ("none", "conservative"):
        mma = pa.MMA(pa.SeparableProblem(ctx, problem, n, c, 0),
                     {"mma_subproblem_solver": "dual", "mma_dual_tol": 1e-9, "mma_max_iterations": iters,
                      "mma_globalization": glob})
        rows, inner = [], []

        def cb(k):
            rows.append(mma.getLastRow())
            inner.append(mma.getGlobalizationStats()["inner_last"])

        mma.setIterationCallback(cb)
        mma.optimize()
        gs = mma.getGlobalizationStats()
        rises = sum(1 for k in range(1, len(rows)) if rows[k][0] > rows[k - 1][0] + 1e-7 * max(1.0, abs(rows[k][0])))
        r = dict(kind="%s_small" % problem, n=n, c=c, globalization=glob, mma_iterations=len(rows) - 1,
                 last_row=rows[-1], inner_total=gs["inner_total"], inner_max=gs["inner_max"], cap_hits=gs["cap_hits"],
                 inner_per_iteration_first20=inner[1:21], fobj_every_20=[rows[k][0] for k in range(0, len(rows), 20)],
                 rises=rises)
        lines.append(r)
        print(json.dumps(r), flush=True)
    return lines


def rho_pass_lines(pa, ctx, n, c, reps):
    """The dual pass, its rho form and the trivial kernel of the rho form's mix, alternating in one call."""
    lines = []
    for form in ([1, 2] if c <= M_F else [2]):
        plain, rho, gram_ms, ceil_ms = pa.bench_mma_dual_rho(ctx, n, c, form, reps)
        r = dict(kind="dual_rho_pass", n=n, c=c, form=form, mix_rho="%d in / %d out" % (2 * c + 7, c + 1 if form == 2 else 0),
                 plain_ms=plain, rho_ms=rho, gram_ms=gram_ms, trivial_rho_mix_ms=ceil_ms,
                 rho_over_plain=[rho[0] / plain[0], rho[1] / plain[1]], predicted_by_bytes=(2 * c + 7) / (2 * c + 6),
                 spread_plain=abs(plain[0] - plain[1]) / min(plain), spread_rho=abs(rho[0] - rho[1]) / min(rho),
                 rho_frac_of_trivial=ceil_ms / min(rho))
        lines.append(r)
        print(json.dumps(r), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--mma-iters", type=int, default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--globalization", choices=("none", "conservative"), default="none")
    ap.add_argument("--problem", default="convex")
    ap.add_argument("--out", default=None)
    ap.add_argument("--nw", type=int, default=0)
    ap.add_argument("--nwcon", type=int, default=0)
    ap.add_argument("--linearized", action="store_true")
    ap.add_argument("--dual-only", action="store_true")
    a = ap.parse_args()
    solvers = ("dual",) if a.dual_only else ("interior_point", "dual")
    if a.small:
        a.globalization = "conservative"
    if a.shapes is None:
        a.shapes = "300x3,200x2" if a.small else "10000000x8,50000000x32"
    if a.mma_iters is None:
        a.mma_iters = 120 if a.small else 4
    if a.out is None and a.linearized:
        a.out = os.path.join(ROOT, "profiles", "r16_bench_mma_linear.jsonl")
    if a.out is None and a.nw > 0:
        a.out = os.path.join(ROOT, "profiles", "r14_bench_mma_gcmma_groups.jsonl" if a.globalization == "conservative"
                             else "r12_bench_mma_groups.jsonl")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r10_bench_gcmma.jsonl" if a.globalization == "conservative"
                             else "r09_bench_mma.jsonl")
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    for shape in a.shapes.split(","):
        n, c = (int(v) for v in shape.split("x"))
        if a.nw > 0 and a.globalization == "conservative":
            lines += gcmma_group_lines(pa, ctx, n, c, a.nwcon or n // a.nw, a.nw, a.mma_iters, a.rounds, a.reps,
                                       a.problem)
            continue
        if a.nw > 0:
            lines += group_lines(pa, ctx, n, c, a.nwcon or n // a.nw, a.nw, a.mma_iters, a.rounds, a.reps, solvers)
            continue
        if a.small:
            lines += small_run_lines(pa, ctx, n, c, a.mma_iters, a.problem)
            continue
        if a.linearized:
            for rnd in range(a.rounds):
                for solver in solvers:
                    r = run_mma(pa, ctx, n, c, solver, a.mma_iters, problem=a.problem, linearized=True)
                    r.update(kind="mma_linearized", problem=a.problem, n=n, c=c, round=rnd)
                    lines.append(r)
                    print(json.dumps(r), flush=True)
            lines += linear_pass_lines(pa, ctx, n, c, a.reps, 2)
            continue
        for rnd in range(a.rounds):
            if a.globalization == "conservative":
                for glob in ("none", "conservative"):
                    r = run_mma(pa, ctx, n, c, "dual", a.mma_iters, glob, a.problem)
                    r.update(kind="mma_gcmma", problem=a.problem, n=n, c=c, round=rnd)
                    if glob == "conservative":  # what a raise costs beyond the plain iteration of the same round
                        r["ms_per_inner_raise"] = ((r["ms_per_mma_iteration"] - lines[-1]["ms_per_mma_iteration"])
                                                   * r["mma_iterations"] / max(1, r["inner_total"]))
                    lines.append(r)
                    print(json.dumps(r), flush=True)
                continue
            for solver in solvers:
                r = run_mma(pa, ctx, n, c, solver, a.mma_iters)
                r.update(kind="mma", n=n, c=c, round=rnd)
                lines.append(r)
                print(json.dumps(r), flush=True)
        if a.globalization == "conservative":
            lines += rho_pass_lines(pa, ctx, n, c, a.reps)
            continue
        for form in ([1, 2] if c <= M_F else [2]):
            pass_ms, gram_ms, ceil_ms = pa.bench_mma_dual(ctx, n, c, form, a.reps)
            streams_in, streams_out = 2 * c + 6, (c + 1 if form == 2 else 0)
            gb = 8.0 * (streams_in + streams_out) * n * 1e-9
            r = dict(kind="dual_pass", n=n, c=c, form=form, mix="%d in / %d out" % (streams_in, streams_out),
                     alg_GB=gb, pass_ms=pass_ms, gram_ms=gram_ms, trivial_ms=ceil_ms,
                     pass_GBps=gb / (pass_ms * 1e-3), frac_hbm_8TBps=gb / (pass_ms * 1e-3) / HBM_PEAK_GBPS,
                     trivial_GBps=gb / (ceil_ms * 1e-3), frac_of_trivial=ceil_ms / pass_ms)
            lines.append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
