"""The metric's workload (config 3: random_convex, n = 50 M, m = 32 dense constraints, L-SR1(10)) through the four
problem boundaries, in one process and alternating:

    builtin         the library's SeparableProblem("convex")
    facade          examples/random_convex_amd.cpp, the C++ user twin (deferred reductions)
    torch_host      examples/random_convex_torch.py, host results (the reference's semantics)
    torch_deferred  the same, device results with deferred reductions
    numpy           paropt_amd.Problem with numpy callbacks on host copies (for scale; fewer steps, last)

Each run is one optimize() of W + K iterations on fresh objects; the K iterations after the warm-up are timed.  One
JSON line per run: it/s, library launches and host synchronisations per iteration (the torch twin's own host
synchronisations counted in), getPhaseTimes() and the library-side time per iteration (step time minus the stream time
of the problem's callbacks, "user_eval").

    python tools/bench_torch_problem.py [--n 50000000] [--ncon 32] [--steps 20] [--warmup 12] [--rounds 3]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import paropt_amd as pa  # noqa: E402
from random_convex_torch import EPS, RandomConvexTorch  # noqa: E402

USER_LIB = os.path.join(ROOT, "examples", "librandom_convex_user.so")


class RandomConvexNumpy(pa.Problem):
    """The same problem with numpy callbacks: x downloaded, g and every A[j] through host mirrors."""

    def __init__(self, ctx, n, ncon, seed=0):
        super().__init__(ctx, n, ncon, ncon)
        self.b2 = pa.PVec(ctx, n).fill_hash(seed, 2, 0).to_numpy() ** 2
        self.a = np.stack([pa.PVec(ctx, n).fill_hash(seed, 100 + j, 0).to_numpy() for j in range(ncon)])
        self.x0 = pa.PVec(ctx, n).fill_hash(seed, 3, 0, 0.9, 0.05).to_numpy()
        self.beta = 0.25 * self.a.sum(axis=1)
        self.host_syncs = 0

    def getVarsAndBounds(self, x, lb, ub):
        x[:], lb[:], ub[:] = self.x0, 0.0, 1.0

    def evalObjCon(self, x):
        return 0, float(np.sum(self.b2 / (x + EPS))), self.beta - self.a @ x

    def evalObjConGradient(self, x, g, A):
        d = x + EPS
        g[:] = -self.b2 / (d * d)
        if A is not None:
            for j in range(self.ncon):
                np.negative(self.a[j], out=A[j])
        return 0


def make(ctx, kind, n, ncon):
    if kind == "builtin":
        return pa.SeparableProblem(ctx, "convex", n, ncon)
    if kind == "facade":
        return pa.UserLibraryProblem(ctx, USER_LIB, n, ncon).setDeferredReductions(True)
    if kind == "torch_host":
        return RandomConvexTorch(ctx, n, ncon)
    if kind == "torch_deferred":
        return RandomConvexTorch(ctx, n, ncon, device_results=True).setDeferredReductions(True)
    return RandomConvexNumpy(ctx, n, ncon)


def run_once(ctx, kind, a, W, K):
    prob = make(ctx, kind, a.n, a.ncon)
    opts = {"qn_type": "sr1", "qn_subspace_size": a.qn_size, "abs_res_tol": 1e-30, "start_affine_multiplier_min": 0.01,
            "max_major_iters": W + K, "write_output_frequency": 0}
    ip = pa.InteriorPoint(prob, opts)
    ip.setCallbackTiming(True)
    stamp = {}

    def cb(k):
        if k == W:
            ctx.synchronize()
            torch.cuda.synchronize()
            stamp["c0"] = ctx.counters()
            stamp["own0"] = getattr(prob, "host_syncs", 0)
            stamp["t0"] = time.perf_counter()

    ip.setIterationCallback(cb)
    ctx.synchronize()
    ip.optimize()
    ctx.synchronize()
    elapsed = time.perf_counter() - stamp["t0"]
    red, lau = ctx.counters()
    own = getattr(prob, "host_syncs", 0) - stamp["own0"]
    niter = ip.getIterationCounters()[0]
    assert niter == W + K, (niter, W, K)
    phases = ip.getPhaseTimes()
    step_ms = 1e3 * elapsed / K
    user_ms = 1e3 * phases.get("user_eval", 0.0) / niter
    out = {"problem": kind, "n": a.n, "ncon": a.ncon, "qn": "sr1(%d)" % a.qn_size, "warmup": W, "steps": K,
           "it_per_s": K / elapsed, "ms_per_step": step_ms, "user_eval_ms_per_iter": user_ms,
           "library_ms_per_iter": step_ms - user_ms,
           "host_syncs_per_iter": (red - stamp["c0"][0] + own) / K, "own_host_syncs_per_iter": own / K,
           "launches_per_iter": (lau - stamp["c0"][1]) / K, "phases_s": phases,
           "counters": list(ip.getIterationCounters()), "fobj": ip.getObjective()[0]}
    ip.setIterationCallback(lambda k: None)
    del ip, prob
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--ncon", type=int, default=32)
    ap.add_argument("--qn-size", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--numpy-steps", type=int, default=3, help="timed steps of the numpy run (0: skip it)")
    a = ap.parse_args()
    W = max(a.warmup, a.qn_size + 2)  # the timed window starts with the quasi-Newton memory full (as bench.py)
    ctx = pa.Context(0)
    kinds = ["builtin", "facade", "torch_host", "torch_deferred"]
    for r in range(a.rounds):
        for kind in kinds:
            out = run_once(ctx, kind, a, W, a.steps)
            out["round"] = r
            print(json.dumps(out), flush=True)
    if a.numpy_steps > 0:
        out = run_once(ctx, "numpy", a, W, a.numpy_steps)
        out["round"] = 0
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
