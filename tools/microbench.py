#!/usr/bin/env python3
"""Micro-benchmarks on one GPU: every hot kernel of an interior-point iteration in isolation
(po_bench_kernels), as JSON lines with GB/s against the HBM roofline."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def xgram_rows(pa, ctx, reps, tag):
    """Wall time of the whole call (launches, final stage, host sync: what a caller outside a batch pays), median and
    range over `reps` alternating rounds; fraction of 8 TB/s on the 16 m w bytes the product has to read."""
    import time

    import numpy as np

    for w in (1_000_000, 4_000_000, 20_000_000):
        for m in (12, 25, 43):
            U = [pa.PVec(ctx, w).fill_hash(0, 100 + j, 0, 2.0, -1.0) for j in range(m)]
            Z = [pa.PVec(ctx, w).fill_hash(0, 300 + j, 0, 2.0, -0.5) for j in range(m)]
            ones = pa.PVec(ctx, w)
            ones.set(1.0)
            forms = {
                "a_xgram": lambda: pa.xgram(U, Z),
                "b_wgram_stacked": lambda: pa.wgram(ones, U + Z)[:m, m:],
                "c_mdot": lambda: np.stack([np.array(Z[j].mdot(U)) for j in range(m)], axis=1),
                # the SAME call as (b) at another place in the round: what two readings of one kernel differ by here
                "b_wgram_stacked_again": lambda: pa.wgram(ones, U + Z)[:m, m:],
            }
            ref = forms["c_mdot"]()
            times = {k: [] for k in forms}
            for f in forms.values():  # warm-up (first launch of an instantiation sets its attributes)
                f()
            for _ in range(reps):
                for k, f in forms.items():
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    out = f()
                    times[k].append(1e3 * (time.perf_counter() - t0))
                    assert np.abs(out - ref).max() <= 1e-13 * w * 10, k
            for k, t in times.items():
                med = float(np.median(t))
                print(json.dumps({"bench": "xgram", "form": k, "w": w, "m": m, "ms": med, "ms_min": min(t),
                                  "ms_max": max(t), "frac_of_8TBs": 16.0 * m * w / (med * 1e-3) / 8e12,
                                  "reps": reps, "tag": tag}), flush=True)
            del U, Z, ones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--c", type=int, default=32, help="dense constraints")
    ap.add_argument("--k", type=int, default=10, help="quasi-Newton panel columns (<= 12)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", type=str, default="")
    ap.add_argument("--vec-api", action="store_true",
                    help="roofline rows of the ParOptVec operations and ParOptQuasiNewton::mult (with the ceiling of "
                         "each stream mix) instead of the iteration kernels")
    ap.add_argument("--xgram", action="store_true",
                    help="the two-panel Gram X = U^T Z in three forms of the same product, alternating in one process: "
                         "(a) xgram, (b) wgram on the stacked panel [U | Z] with unit weights, (c) m mdot calls, (b) again; "
                         "w in {1 M, 4 M, 20 M} x m in {12, 25, 43}")
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    if a.xgram:
        return xgram_rows(pa, ctx, a.reps, a.tag)
    if a.vec_api:
        for r in pa.bench_vec_api(ctx, a.n, a.reps):
            r.update(n=a.n, tag=a.tag)
            print(json.dumps(r), flush=True)
        return
    for r in pa.bench_kernels(ctx, a.n, a.c, a.k, a.reps):
        r.update(n=a.n, c=a.c, k=a.k, tag=a.tag)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
