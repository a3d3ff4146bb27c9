"""What a Hessian-vector product by differences of the Lagrangian's gradient costs (InteriorPoint.setHvecFiniteDifference)
at config 3's shape: convex, n = 50 M, m = 32 dense constraints -- and for the same problem with its constraints declared
linear (setLinearConstraints: the Jacobian pairs drop out, the product is the gradient pair alone).

Per case (forward and central form): ms per product -- host clock around `reps` po_ip_eval_hvec calls that end in a device
synchronise, after one warm-up call that allocates the scratch -- split into

    user      stream time of the problem's evalObjCon + evalObjConGradient at the perturbed points (HIP events around the
              callbacks, the phase "hvec_user_eval"; the built-in problem's kernels stand in for a user's)
    library   the rest: the step-size pass, the perturbed point, the combine pass, launch and synchronisation overhead

and, from po_bench_vec_api in the SAME process, the two new kernels beside the trivial kernel of their stream mix: the
combine pass (2 m + 2 = 66 input streams and one output stream at m = 32: 67 x 0.4 GB = 26.8 GB per product) and the
step-size pass.  One JSON document, written to --out as well.  No CPU fallback: the tool fails without a GPU.

    python tools/bench_hvec_fd.py [--n 50000000] [--c 32] [--reps 10] [--out profiles/hvec_fd_c3.json] [--no-kernels]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import paropt_amd as pa  # noqa: E402


def product_case(ctx, n, c, linear, central, reps):
    prob = pa.SeparableProblem(ctx, "convex", n, c)
    if linear:
        prob.setLinearConstraints(True)
    ip = pa.InteriorPoint(prob, {"qn_type": "sr1", "qn_subspace_size": 10, "abs_res_tol": 1e-30,
                                 "start_affine_multiplier_min": 0.01, "max_major_iters": 3,
                                 "write_output_frequency": 0})
    ip.optimize()  # an interior iterate with a live gradient and Jacobian
    ip.setCallbackTiming(True)
    ip.setHvecFiniteDifference("always", central=central)
    px = pa.PVec(ctx, prob.nvars).fill_hash(0, 77, prob.offset, 2.0, -1.0)
    hv = pa.PVec(ctx, prob.nvars)
    z = np.linspace(0.5, 1.5, c)
    v0 = pa.live_objects()
    ip.evalHvec(z, None, px, hv)  # warm-up: allocates the scratch
    v1 = pa.live_objects()
    ctx.synchronize()
    user0 = ip.getPhaseTimes().get("hvec_user_eval", 0.0)
    b0 = ctx.algorithmic_bytes()
    r0, l0 = ctx.counters()
    t0 = time.perf_counter()
    for _ in range(reps):
        ip.evalHvec(z, None, px, hv)
    ctx.synchronize()
    total = (time.perf_counter() - t0) / reps
    user = (ip.getPhaseTimes().get("hvec_user_eval", 0.0) - user0) / reps
    b1 = ctx.algorithmic_bytes()
    r1, l1 = ctx.counters()
    products, evals = ip.getHvecFiniteDifferenceCount()
    lib_bytes = ((b1[0] - b0[0]) - (b1[1] - b0[1])) / reps
    return {"linear_constraints": linear, "form": "central" if central else "forward",
            "ms_per_product": 1e3 * total, "ms_user_callbacks": 1e3 * user, "ms_library": 1e3 * (total - user),
            "evaluations_per_product": evals // max(products, 1), "step": ip.getHvecFiniteDifferenceStep(),
            "scratch_vectors": v1[0] - v0[0], "scratch_GB": (v1[1] - v0[1]) * 1e-9,
            "library_alg_GB_per_product": lib_bytes * 1e-9,
            "library_GBps": lib_bytes / max(total - user, 1e-12) * 1e-9,
            "launches_per_product": (l1 - l0) / reps, "host_syncs_per_product": (r1 - r0) / reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--c", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hvec_fd_c3.json"))
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel rows of po_bench_vec_api")
    a = ap.parse_args()
    ctx = pa.Context(0)
    out = {"what": "Hessian-vector product by differences, convex n = %d, m = %d; host clock around %d products ending in "
                   "a device synchronise; user = HIP-event time of the problem's callbacks" % (a.n, a.c, a.reps),
           "n": a.n, "c": a.c, "reps": a.reps, "products": [], "kernels": []}
    for linear in (False, True):
        for central in (False, True):
            row = product_case(ctx, a.n, a.c, linear, central, a.reps)
            out["products"].append(row)
            print(json.dumps(row), flush=True)
    if not a.no_kernels:
        # the calibration rows are fixed at 32 constraint pairs: the ceiling is the trivial kernel of the same mix
        for r in pa.bench_vec_api(ctx, a.n, a.reps):
            if r["op"].startswith("hvec_fd_"):
                out["kernels"].append(r)
                print(json.dumps(r), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps({"written": a.out, "cases": len(out["products"]), "kernel_rows": len(out["kernels"])}))


if __name__ == "__main__":
    main()
