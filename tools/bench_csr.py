"""
The CSR form of the sparse constraints at scale: convex workload with n variables,
c dense constraints and the rank-local overlapping chain constraints cw_i = 1 - sum_{k<span} x[i*stride+k]^2
(examples/rosenbrock/sparse_rosenbrock.cpp generalised), i.e. a sparse SPD Schur complement with w ~ n/stride
rows that is assembled, factored and solved on the GPU every interior-point iteration.  No CPU reference leg:
the reference's sparse Cholesky needs METIS, which this image lacks.  Prints one JSON line.

    python tools/bench_csr.py [--nglobal 4000000] [--ncon 4] [--span 2] [--stride 1] [--steps 20] [--warmup 5]
                              [--dense-columns R]

--dense-columns R: R further variables that enter EVERY sparse constraint (cw_i -= sum_j xd_j^2, the shape of an
epigraph variable): their columns of the Jacobian are dense, leave the factored matrix and come back by a low-rank
update.  The chain itself keeps its n variables, so R = 0 is the run of record.

--quasidef user: the same run with a USER quasi-definite solver attached (createQuasiDefMat) that only forwards factor
and apply to the library's own solver of a twin problem with the same pattern and entries.  The solve itself then
costs what it costs the library; the difference to the plain run is the hook: one apply per panel column and the
cross product instead of the half solve.  Reports the share of the measured time spent inside the user's applies.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ForwardingSolver:
    """factor / apply forwarded to po_quasidef_* of a twin problem (same chain pattern; the entries -2 x of the chain
    constraints are copied from the solved problem's device array at every factor).  Times are host wall time with a
    stream synchronisation after each call, so that the work is attributed to the call that issued it."""

    def __init__(self, pa, ctx, a):
        self.pa, self.ctx = pa, ctx
        self.twin = pa.SeparableProblem(ctx, a.problem, a.n, a.ncon, 0).setChain(a.span, a.stride)
        self.main = None
        self.t_apply = self.t_factor = 0.0
        self.napply = 0
        self.held = None

    def factor(self, x, dinv, cdiag):
        t0 = time.perf_counter()
        _, _, src = self.main.getSparseJacobianData(device=True)
        _, _, dst = self.twin.getSparseJacobianData(device=True)
        dst.copy_(src)
        self.held = (x, dinv, cdiag)  # borrowed until the next factor
        self.pa.quasidef_factor(self.twin, *self.held)
        self.ctx.synchronize()
        self.t_factor += time.perf_counter() - t0
        return 0

    def apply(self, bx, bw, yx, yw):
        t0 = time.perf_counter()
        self.pa.quasidef_apply(self.twin, *self.held, bx, bw, yx, yw)
        self.ctx.synchronize()
        self.t_apply += time.perf_counter() - t0
        self.napply += 1
        return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nglobal", dest="n", type=int, default=4_000_000)
    ap.add_argument("--ncon", type=int, default=4)
    ap.add_argument("--problem", default="convex")
    ap.add_argument("--span", type=int, default=2)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--qn-size", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quasidef", choices=("library", "user"), default="library")
    ap.add_argument("--dense-columns", dest="dense", type=int, default=0)
    a = ap.parse_args()
    if a.dense and a.quasidef == "user":
        ap.error("--dense-columns measures the library's solver")
    import paropt_amd as pa

    ctx = pa.Context(0)
    t0 = time.perf_counter()
    prob = pa.SeparableProblem(ctx, a.problem, a.n + a.dense, a.ncon, 0).setChain(a.span, a.stride,
                                                                                 dense_vars=a.dense)
    t_sym = time.perf_counter() - t0
    fwd = None
    if a.quasidef == "user":
        fwd = ForwardingSolver(pa, ctx, a)
        fwd.main = prob
        prob.setQuasiDefMat(fwd, device="pvec")
    opts = {"qn_type": "bfgs", "qn_subspace_size": a.qn_size, "abs_res_tol": 1e-30, "abs_step_tol": 0.0,
            "starting_point_strategy": "affine_step", "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0,
            "max_major_iters": a.warmup + a.steps, "write_output_frequency": 0}
    ip = pa.InteriorPoint(prob, opts)
    marks = {}

    def cb(k):
        if k in (a.warmup, a.warmup + a.steps):
            ctx.synchronize()
            marks[k] = time.perf_counter()
            marks["counters", k] = ctx.counters()
            if fwd is not None:
                marks["apply", k] = (fwd.t_apply, fwd.napply, fwd.t_factor)

    ip.setIterationCallback(cb)
    ip.optimize()
    ctx.synchronize()
    niter = ip.getIterationCounters()[0]
    t1 = marks.get(a.warmup + a.steps, time.perf_counter())
    steps = min(niter, a.warmup + a.steps) - a.warmup
    dt = t1 - marks[a.warmup]
    extra = {}
    if a.dense:
        extra = {"dense_columns": prob.dense_columns}
    (s0, l0), (s1, l1) = marks["counters", a.warmup], marks.get(("counters", a.warmup + a.steps), ctx.counters())
    if fwd is not None:
        (ta0, na0, tf0), (ta1, na1, tf1) = marks["apply", a.warmup], marks.get(("apply", a.warmup + a.steps),
                                                                           (fwd.t_apply, fwd.napply, fwd.t_factor))
        extra = {"quasidef": "user (forwarding to the library's solver of a twin problem)",
                 "user_applies_per_step": (na1 - na0) / steps, "share_in_user_applies": (ta1 - ta0) / dt,
                 "share_in_user_factor": (tf1 - tf0) / dt}
    print(json.dumps({
        **extra,
        "metric": "interior-point iterations/s (CSR sparse constraints)", "value": steps / dt,
        "unit": "IP iterations/s", "n_gpus": 1, "steps": steps, "warmup": a.warmup, "ms_per_step": 1e3 * dt / steps,
        "dtype": "f64", "data": "synthetic", "launches_per_step": (l1 - l0) / steps,
        "host_syncs_per_step": (s1 - s0) / steps,
        "config": {"workload": "%s n=%d c=%d chain span=%d stride=%d (w=%d) L-BFGS(%d)" % (
            a.problem, a.n + a.dense, a.ncon, a.span, a.stride, prob.nwcon, a.qn_size) + (
                " + %d dense columns" % a.dense if a.dense else "")},
        "fobj": ip.getObjective()[0], "symbolic_seconds": t_sym, "factor_info": pa.quasidef_factor_info(prob),
    }))


if __name__ == "__main__":
    main()
