"""What a quasi-Newton approximation behind the PUBLIC interface costs: the built-in ParOptLBFGS against the user-written
class of examples/user_quasi_newton_amd.cpp (its own HIP kernels, attached through setQuasiNewton), alternating in ONE
process, on

    c2        config 2:        quadratic, n = 10 M, m = 8,  L-BFGS(20)
    c3_bfgs   config 3's data: convex,    n = 50 M, m = 32, L-BFGS(20)

Each run is one optimize() of W + K iterations on fresh objects, W = max(warmup, qn + 2), so that the timed window
starts with the memory full; host clock around a device synchronise.  One JSON line per run, then one summary line per
size with the stream ceiling of the same run (read-only dot of two vectors, bytes / time) and the PREDICTED slowdown:
the doubles per variable and iteration that the user path streams beyond the built-in, counted from the code --

    built-in update:  Z^T s comes from the step's panel products and the pair enters by buffer swap: s.s, s.y (2 reads of
                      s, 1 of y) and y.y (1 read)                                              =  4 streams
    user update:      s, y and the k = 2 * qn columns read once, s and y written to the spare   =  k + 4 streams
    extra                                                                                       =  k     streams

-- times 8 bytes over the ceiling.  No CPU fallback: the tool fails without a GPU.

    python tools/bench_user_qn.py [--sizes c2,c3_bfgs] [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import ctypes as C
import gc
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import paropt_amd as pa  # noqa: E402
import paropt_amd.lib as L  # noqa: E402

SIZES = {"c2": ("quadratic", 10_000_000, 8, 20), "c3_bfgs": ("convex", 50_000_000, 32, 20)}
USER_LIB = os.path.join(ROOT, "examples", "libuser_quasi_newton.so")


def user_library():
    if not os.path.exists(USER_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "libuser_quasi_newton.so"])
    lib = C.CDLL(USER_LIB)
    lib.user_qn_create.restype = C.c_void_p
    lib.user_qn_create.argtypes = [L.po_ctx, C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(L.po_qn)]
    lib.user_qn_calls.restype = None
    lib.user_qn_calls.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    lib.user_qn_destroy.restype = None
    lib.user_qn_destroy.argtypes = [C.c_void_p]
    return lib


def run_once(ctx, ulib, size, kind, W, K):
    problem, n, ncon, qn = SIZES[size]
    prob = pa.SeparableProblem(ctx, problem, n, ncon)
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": qn, "abs_res_tol": 1e-30,
                                 "start_affine_multiplier_min": 0.01, "max_major_iters": W + K,
                                 "write_output_frequency": 0})
    obj, h = None, L.po_qn()
    if kind == "user":
        obj = ulib.user_qn_create(ctx.handle, n, qn, 0, 0, C.byref(h))
        L.check(L.lib.po_ip_set_quasi_newton(ip._h, h))
    stamp = {}

    def cb(k):
        if k == W:
            ctx.synchronize()
            stamp["c0"] = ctx.counters()
            stamp["t0"] = time.perf_counter()

    ip.setIterationCallback(cb)
    ctx.synchronize()
    ip.optimize()
    ctx.synchronize()
    elapsed = time.perf_counter() - stamp["t0"]
    red, lau = ctx.counters()
    niter = ip.getIterationCounters()[0]
    assert niter == W + K, (niter, W, K)
    out = {"size": size, "qn_class": kind, "problem": problem, "n": n, "ncon": ncon, "qn": "bfgs(%d)" % qn,
           "warmup": W, "steps": K, "ms_per_step": 1e3 * elapsed / K, "it_per_s": K / elapsed,
           "host_syncs_per_iter": (red - stamp["c0"][0]) / K, "library_launches_per_iter": (lau - stamp["c0"][1]) / K,
           "counters": list(ip.getIterationCounters()), "fobj": ip.getObjective()[0]}
    if obj:
        calls = (C.c_long * 6)()
        ulib.user_qn_calls(obj, calls)
        out["user_calls"] = dict(zip(("reset", "update", "mult", "multAdd", "getCompactMat", "getMaxSize"), calls))
        L.check(L.lib.po_ip_set_quasi_newton(ip._h, None))
    ip.setIterationCallback(lambda k: None)
    del ip
    if obj:
        ulib.user_qn_destroy(obj)
    del prob
    gc.collect()
    return out


def stream_ceiling(ctx, n):
    """bytes / s of a read-only pass over two n-vectors (the reduction kernels' own stream)"""
    x, y = pa.PVec(ctx, n).fill_hash(0, 1), pa.PVec(ctx, n).fill_hash(0, 2)
    pa.bench_stream(x, y, 0, 3)
    ms = pa.bench_stream(x, y, 0, 10)
    return 16.0 * n / (1e-3 * ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="c2,c3_bfgs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ctx = pa.Context(0)  # raises without a GPU
    ulib = user_library()
    for size in a.sizes.split(","):
        problem, n, ncon, qn = SIZES[size]
        W = max(a.warmup, qn + 2)
        run_once(ctx, ulib, size, "builtin", W, 2)  # first-use costs (allocator, code objects) stay out of round 0
        ms = {"builtin": [], "user": []}
        for r in range(max(a.rounds, 3)):
            for kind in ("builtin", "user"):
                out = run_once(ctx, ulib, size, kind, W, a.steps)
                out["round"] = r
                ms[kind].append(out["ms_per_step"])
                print(json.dumps(out), flush=True)
        ceiling = stream_ceiling(ctx, n)
        extra = 2 * qn
        b, u = sorted(ms["builtin"]), sorted(ms["user"])
        med = lambda v: v[len(v) // 2]  # noqa: E731
        print(json.dumps({"size": size, "summary": True, "stream_ceiling_GBps": ceiling / 1e9,
                          "extra_doubles_per_variable_and_iteration": extra,
                          "predicted_extra_ms_per_step": 1e3 * 8.0 * extra * n / ceiling,
                          "measured_extra_ms_per_step": med(u) - med(b),
                          "builtin_ms_per_step": b, "user_ms_per_step": u,
                          "builtin_spread_ms": b[-1] - b[0]}), flush=True)


if __name__ == "__main__":
    main()
