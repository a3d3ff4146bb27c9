"""
The CSR sparse constraints on their two factor engines, sparse_factor="rows" (the default, the level-scheduled row
Cholesky) and sparse_factor="multifrontal" (the engine of ParOptSparseCholesky), in one process, alternating, three
repeats each.  The baseline is the row engine: the same problem, the same process, the other setting.

On the grid pattern of tools/bench_sparse_chol.py (one constraint per edge of an nx x nx grid of variables) timed are
    pa.quasidef_factor, pa.quasidef_apply,
    pa.quasidef_gram at nv = 21 and nv = 73 (the panel widths of bench.py's config 3 with L-SR1(10) and L-BFGS(20)),
        with the correction vector,
    interior-point iterations per second on a convex objective over that pattern (sum (x - xt)^2, one dense linear
        constraint, cw = b - A x >= 0, L-BFGS(10); the callbacks are host numpy through scipy.sparse and cost both
        engines the same),
and on the chain pattern of tools/bench_csr.py at its default size (fronts of order 3) factor, apply and the
interior-point iterations per second of that tool's run.  One JSON line per pattern.

--pack 0 8 16 ... runs the multifrontal engine once per cap on its packed groups of tiny fronts (debug switch 38, set
before each problem is created and reset after): the engines are then "rows", "multifrontal:cap0", "multifrontal:cap8",
...  Cap 0 is the engine without packing -- a workgroup per front -- and is the baseline of the other caps, in the same
process, alternating.

    python tools/bench_csr_multifrontal.py [--sizes 150 300] [--chain-nglobal 4000000] [--repeats 3] [--inner 3]
                                           [--steps 15] [--warmup 5] [--pack 0 8 16 32 64]
                                           [--out profiles/r19_bench_chol_packing.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENGINES = ("rows", "multifrontal")  # (--pack: one "multifrontal:cap<k>" per value instead of the second, engines_of)
SW_CHOL_PACK = 38  # core.hpp DbgSwitch


def create(label, build):
    """the problem of engine `label`, analysed under its cap"""
    import paropt_amd as pa
    from paropt_amd.lib import lib

    kind, _, cap = label.partition(":cap")
    if cap:
        lib.po_debug_set_switch(SW_CHOL_PACK, int(cap))
    try:
        prob = build(kind)
        pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()  # uploads the Jacobian entries
    finally:
        lib.po_debug_set_switch(SW_CHOL_PACK, -1)
    return prob

IP_OPTS = {"qn_type": "bfgs", "qn_subspace_size": 10, "abs_res_tol": 1e-30, "abs_step_tol": 0.0,
           "starting_point_strategy": "affine_step", "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0,
           "write_output_frequency": 0}


def engines_of(a):
    return ("rows",) + tuple("multifrontal:cap%d" % cap for cap in a.pack) if a.pack else ENGINES


def time_ratios(rec, key, engines):
    """rows / engine of every repeat: a list under the name this tool always wrote, or with --pack one list per cap"""
    name = key.replace("_ms", "_ratio_rows_over")
    if engines == ENGINES:
        rec[name + "_multifrontal"] = [a / b for a, b in zip(rec[key]["rows"], rec[key]["multifrontal"])]
    else:
        rec[name] = {e: [a / b for a, b in zip(rec[key]["rows"], rec[key][e])] for e in engines[1:]}


def rate_ratios(rec, engines):
    rates = rec["ip_iterations_per_s"]
    if engines == ENGINES:
        rec["ip_ratio_multifrontal_over_rows"] = [m / r for r, m in zip(rates["rows"], rates["multifrontal"])]
    else:
        rec["ip_ratio_over_rows"] = {e: [m / r for r, m in zip(rates["rows"], rates[e])] for e in engines[1:]}


def timed(ctx, fn, inner):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / inner


def iterations_per_second(pa, ctx, prob, warmup, steps):
    ip = pa.InteriorPoint(prob, dict(IP_OPTS, max_major_iters=warmup + steps))
    marks = {}

    def cb(k):
        if k in (warmup, warmup + steps):
            ctx.synchronize()
            marks[k] = time.perf_counter()

    ip.setIterationCallback(cb)
    ip.optimize()
    ctx.synchronize()
    niter = ip.getIterationCounters()[0]
    done = min(niter, warmup + steps) - warmup
    dt = marks.get(warmup + steps, time.perf_counter()) - marks[warmup]
    return done / dt, done, ip.getObjective()[0]


def vec(pa, ctx, arr):
    return pa.PVec(ctx, len(arr)).from_numpy(np.asarray(arr, dtype=float))


def solver_times(pa, ctx, probs, n, w, rng, repeats, inner, widths, rec):
    """factor / apply / gram of every problem, alternating; checks that the engines solve the same system"""
    engines = tuple(probs)
    dinv, cdiag = rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 1.0, w)
    x, d, c = vec(pa, ctx, np.full(n, 0.5)), vec(pa, ctx, dinv), vec(pa, ctx, cdiag)
    bx, bw = vec(pa, ctx, rng.standard_normal(n)), vec(pa, ctx, rng.standard_normal(w))
    out = {}
    for e in engines:
        yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
        pa.quasidef_factor(probs[e], x, d, c)
        pa.quasidef_apply(probs[e], x, d, c, bx, bw, yx, yw)
        out[e] = (yx, yw)
        rec["factor_info_" + e] = pa.quasidef_factor_info(probs[e])
    ref = out["rows"][1].to_numpy()
    rec["solutions_max_abs_diff"] = max(float(np.abs(out[e][1].to_numpy() - ref).max()) for e in engines[1:])
    mf = [out[e][1].to_numpy() for e in engines[1:]]
    if len(mf) > 1:
        rec["multifrontal_solutions_bit_equal"] = all(np.array_equal(mf[0], y) for y in mf)
    rec["solution_max_abs"] = float(np.abs(ref).max())
    panels = {nv: [pa.PVec(ctx, n).fill_hash(0, 20 + j, 0, 2.0, -1.0 + 0.01 * j) for j in range(nv)] for nv in widths}
    alphas = {nv: rng.standard_normal(nv) for nv in widths}
    for e in engines:
        for nv in widths:
            pa.quasidef_gram(probs[e], x, d, c, panels[nv], alpha=alphas[nv])  # (warm: the work vectors grow once)
    keys = ["quasidef_factor_ms", "quasidef_apply_ms"] + ["quasidef_gram_nv%d_ms" % nv for nv in widths]
    for k in keys:
        rec[k] = {e: [] for e in engines}
    for _ in range(repeats):
        for e in engines:
            p = probs[e]
            yx, yw = out[e]
            rec["quasidef_factor_ms"][e].append(timed(ctx, lambda: pa.quasidef_factor(p, x, d, c), inner))
            rec["quasidef_apply_ms"][e].append(timed(ctx, lambda: pa.quasidef_apply(p, x, d, c, bx, bw, yx, yw), inner))
            for nv in widths:
                rec["quasidef_gram_nv%d_ms" % nv][e].append(
                    timed(ctx, lambda: pa.quasidef_gram(p, x, d, c, panels[nv], alpha=alphas[nv]), inner))
        print("# repeat done", {k: {e: round(rec[k][e][-1], 3) for e in engines} for k in keys}, flush=True)
    for k in keys:
        time_ratios(rec, k, engines)


def run_grid(ctx, nx, a):
    import scipy.sparse as sp

    import paropt_amd as pa
    from csr_helpers import grid_pattern

    n = nx * nx
    rowp, cols = grid_pattern(nx, nx)
    w = len(rowp) - 1
    rng = np.random.default_rng(0)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    A = sp.csr_matrix((data, cols, rowp), shape=(w, n))
    xt = rng.uniform(0.2, 0.8, size=n)
    b = A @ rng.uniform(0.3, 0.6, size=n) + 0.05  # cw = b - A x >= 0 is feasible
    a0 = rng.uniform(0.5, 1.0, size=n)

    def problem(kind):
        class P(pa.Problem):
            def __init__(self):
                super().__init__(ctx, n, 1, 1, nwcon=w, nwinequality=w, rowp=rowp, cols=cols, sparse_factor=kind)

            def getVarsAndBounds(self, x, lb, ub):
                x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

            def evalSparseObjCon(self, x, sparse):
                sparse[:] = b - A @ x
                return 0, float(np.sum((x - xt) ** 2)), np.array([0.45 * np.sum(a0) - a0 @ x])

            def evalSparseObjConGradient(self, x, g, Ac, d):
                g[:] = 2.0 * (x - xt)
                Ac[0][:] = -a0
                d[:] = -data
                return 0

        return P()

    engines = engines_of(a)
    rec = {"pattern": "grid %dx%d" % (nx, nx), "n": n, "w": w, "repeats": a.repeats, "inner": a.inner}
    probs = {}
    for e in engines:
        t0 = time.perf_counter()
        probs[e] = create(e, problem)
        rec["setup_s_" + e] = time.perf_counter() - t0
    solver_times(pa, ctx, probs, n, w, rng, a.repeats, a.inner, (21, 73), rec)
    rec["ip_iterations_per_s"] = {e: [] for e in engines}
    rec["ip_workload"] = "sum (x - xt)^2, 1 dense linear constraint, cw = b - A x >= 0, L-BFGS(10), host callbacks"
    for _ in range(a.repeats):
        for e in engines:
            rate, done, fobj = iterations_per_second(pa, ctx, probs[e], a.warmup, a.steps)
            rec["ip_iterations_per_s"][e].append(rate)
            rec.setdefault("ip_steps", {})[e] = done
            rec.setdefault("ip_fobj", {})[e] = fobj
        print("# ip repeat done", {e: round(rec["ip_iterations_per_s"][e][-1], 3) for e in engines}, flush=True)
    rate_ratios(rec, engines)
    return rec


def run_chain(ctx, a):
    import paropt_amd as pa

    n = a.chain_nglobal
    engines = engines_of(a)
    rec = {"pattern": "chain span 2 stride 1 (tools/bench_csr.py)", "n": n, "repeats": a.repeats, "inner": a.inner}
    probs = {}

    def problem(kind):
        return pa.SeparableProblem(ctx, "convex", n, 4, 0).setChain(2, 1, sparse_factor=kind)

    for e in engines:
        t0 = time.perf_counter()
        probs[e] = create(e, problem)
        rec["setup_s_" + e] = time.perf_counter() - t0
        print("# chain set up", e, round(rec["setup_s_" + e], 2), "s", flush=True)
    w = probs["rows"].nwcon
    rec["w"] = w
    rec["ip_iterations_per_s"] = {e: [] for e in engines}
    rec["ip_workload"] = "convex n=%d c=4 chain span=2 stride=1 (w=%d) L-BFGS(10), built in" % (n, w)
    for _ in range(a.repeats):
        for e in engines:
            rate, done, fobj = iterations_per_second(pa, ctx, probs[e], a.warmup, a.steps)
            rec["ip_iterations_per_s"][e].append(rate)
            rec.setdefault("ip_steps", {})[e] = done
            rec.setdefault("ip_fobj", {})[e] = fobj
        print("# ip repeat done", {e: round(rec["ip_iterations_per_s"][e][-1], 3) for e in engines}, flush=True)
    rate_ratios(rec, engines)
    # (the Jacobian entries are those of the last evaluation of each run: the same point on both engines)
    solver_times(pa, ctx, probs, n, w, np.random.default_rng(0), a.repeats, a.inner, (21,), rec)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[150, 300])
    ap.add_argument("--chain-nglobal", type=int, default=4_000_000, help="0: skip the chain pattern")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pack", type=int, nargs="*", default=None,
                    help="caps of the packed groups to run the multifrontal engine with (0: no packing)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing the file")
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    for nx in a.sizes:
        lines.append(json.dumps(run_grid(ctx, nx, a)))
        print(lines[-1], flush=True)
    if a.chain_nglobal > 0:
        lines.append(json.dumps(run_chain(ctx, a)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
