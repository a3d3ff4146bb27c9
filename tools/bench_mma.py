"""
MMA with its two sub-solvers on one MI355X: the built-in `convex` problem at (n = 10 M, c = 8) and (n = 50 M, c = 32).
In ONE process the interior-point sub-solver (the reference's way) and the dual sub-solver alternate, three rounds of a
few MMA iterations each; then one evaluation of the dual is timed beside the trivial kernel of its stream mix
(po_bench_mma_dual).  One JSON line per run, appended to profiles/r09_bench_mma.jsonl (--out), whatever comes out.

    python tools/bench_mma.py [--shapes 10000000x8,50000000x32] [--mma-iters 4] [--rounds 3] [--out FILE]
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


def run_mma(pa, ctx, n, c, solver, iters):
    prob = pa.SeparableProblem(ctx, "convex", n, c, 0)
    mma = pa.MMA(prob, {"mma_subproblem_solver": solver, "mma_max_iterations": iters, "mma_l1_tol": 0.0,
                        "mma_linfty_tol": 0.0, "write_output_frequency": 0})
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
        out["dual_stats"] = mma.getDualStats()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x8,50000000x32")
    ap.add_argument("--mma-iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bench_mma.jsonl"))
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    for shape in a.shapes.split(","):
        n, c = (int(v) for v in shape.split("x"))
        for rnd in range(a.rounds):
            for solver in ("interior_point", "dual"):
                r = run_mma(pa, ctx, n, c, solver, a.mma_iters)
                r.update(kind="mma", n=n, c=c, round=rnd)
                lines.append(r)
                print(json.dumps(r), flush=True)
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
