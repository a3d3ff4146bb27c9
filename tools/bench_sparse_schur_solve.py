"""
Factoring and solving with the Schur complement on the device (pa.SparseCholesky.factor_schur and what follows it)
beside the PLAIN handle on the same matrix in the same elimination order, in one process, alternating, three repeats
each, one JSON line per pattern (and one per further panel width):

    partial_factor_ms      set_values_device + factor() of the handle with the Schur set
    schur_factor_ms        factor_schur(): the copy of S and its dense factorization, ns^3 / 3 flops
    schur_solve_ms         schur_solve_tensor of nrhs right-hand sides, {"1": [...], "32": [...]}
    solve_ms               the whole solve_tensor on the Schur handle, the same nrhs
    plain_factor_ms / plain_solve_ms   the plain handle (order "natural" with the Schur handle's perm): the same
                           elimination order with the set as ordinary supernodes, swept a front a workgroup
    l2_bytes               the bytes of L2 one forward and one backward dense sweep read: 2 * 8 * ns (ns + 1) / 2
    sweep_GBps / sweep_frac_hbm_8TBps   l2_bytes / schur_solve_ms, beside the 8 TB/s the project measures against
    torch_cholesky_ms / torch_cholesky_solve_ms   "the caller's own solve" on schur_device's output with
                           torch.linalg.cholesky / torch.cholesky_solve (of -S where S is negative definite); null where
                           this build of torch cannot do it
    solve_speedup          plain_solve_ms / solve_ms per nrhs, from the medians

Patterns: the nx x nx five-point grid with one grid line as the set (default 300: ns = 300) and the KKT matrix of
tools/bench_sparse_schur.py (20 000 blocks of order 4, 256 constraints) -- the patterns of record -- and 7-point 3-D
grids m^3 with the middle plane as the set (default m = 32 and 64: ns = 1024 and 4096).  --widths re-creates the Schur
handle with other panel widths W (debug switch 39) and times its solves alone.

    python tools/bench_sparse_schur_solve.py [--grid 300] [--kkt 20000 4 256] [--grid3 32 64] [--widths 64 256]
        [--repeats 3] [--inner 5] [--out file.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparse_schur import grid_line, kkt_blocks  # noqa: E402

SW_CHOL_SCHUR_W = 39  # core.hpp DbgSwitch
HBM_PEAK_GBPS = 8000.0
NRHS = (1, 32)


def grid3_plane(m):
    import scipy.sparse as sp

    T = sp.diags([-np.ones(m - 1), np.full(m, 2.25), -np.ones(m - 1)], [-1, 0, 1])
    I = sp.eye(m)
    G = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsc()
    G.sort_indices()
    return "7-point grid %d^3, the middle plane" % m, G, (m // 2) * m * m + np.arange(m * m), "llt"


def median(v):
    return float(np.median(v))


def run(ctx, name, M, schur, kind, repeats, inner, width=None):
    import torch

    import paropt_amd as pa
    from paropt_amd.lib import lib

    n = M.shape[0]
    dev = torch.device("cuda", ctx.device())
    lib.po_debug_set_switch(SW_CHOL_SCHUR_W, -1 if width is None else int(width))
    try:
        t0 = time.perf_counter()
        part = pa.SparseCholesky(ctx, n, M.indptr, M.indices, factorization=kind, schur=schur)
        t_setup = time.perf_counter() - t0
    finally:
        lib.po_debug_set_switch(SW_CHOL_SCHUR_W, -1)
    plain = None
    if width is None:
        plain = pa.SparseCholesky(ctx, n, M.indptr, M.indices, order="natural", perm=part.perm, factorization=kind)
    vals = torch.from_numpy(np.ascontiguousarray(M.data)).to(dev)
    ns = part.num_schur
    rng = np.random.default_rng(1)
    rhs = {r: torch.from_numpy(rng.standard_normal((r, n))).to(dev) for r in NRHS}
    rhs2 = {r: torch.from_numpy(rng.standard_normal((r, ns))).to(dev) for r in NRHS}
    work = {r: rhs[r].clone() for r in NRHS}
    work2 = {r: rhs2[r].clone() for r in NRHS}

    def timed(fn, count=inner):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    def factor(c):
        c.set_values_device(vals)
        assert c.factor() == 0

    def schur_factor():
        assert part.factor_schur() == 0

    def schur_solve(r):
        work2[r].copy_(rhs2[r])
        part.schur_solve_tensor(work2[r])

    def solve(c, r):
        work[r].copy_(rhs[r])
        c.solve_tensor(work[r])

    info = part.schur_solve_info()
    l2_bytes = 2 * 8 * ns * (ns + 1) // 2
    rec = {"pattern": name, "n": n, "ns": ns, "factorization": kind, "panel_width": info["panel_width"],
           "launches": info["launches"], "setup_s": t_setup, "l2_bytes": l2_bytes, "inner": inner}
    factor(part)
    schur_factor()
    rec["factor_bytes"] = part.schur_solve_info()["factor_bytes"]
    if plain is not None:
        factor(plain)
        # the two routes solve the same system: the largest difference of the solutions over the largest entry
        solve(part, 1)
        x = work[1].clone()
        solve(plain, 1)
        rec["max_rel_difference_to_plain"] = float((x - work[1]).abs().max() / work[1].abs().max())
    for r in NRHS:  # warm
        schur_solve(r)
        solve(part, r)
        if plain is not None:
            solve(plain, r)
    keys = ["schur_solve_ms", "solve_ms"] + (["plain_solve_ms"] if plain is not None else [])
    rec.update({k: {str(r): [] for r in NRHS} for k in keys})
    if plain is not None:
        rec.update({"partial_factor_ms": [], "plain_factor_ms": [], "schur_factor_ms": []})
    for _ in range(repeats):
        if plain is not None:
            rec["partial_factor_ms"].append(timed(lambda: factor(part), 1))
            rec["schur_factor_ms"].append(timed(schur_factor, 1))
            rec["plain_factor_ms"].append(timed(lambda: factor(plain), 1))
        for r in NRHS:
            rec["schur_solve_ms"][str(r)].append(timed(lambda: schur_solve(r)))
            rec["solve_ms"][str(r)].append(timed(lambda: solve(part, r)))
            if plain is not None:
                rec["plain_solve_ms"][str(r)].append(timed(lambda: solve(plain, r)))
    rec["sweep_GBps"] = {str(r): l2_bytes * 1e-9 / (median(rec["schur_solve_ms"][str(r)]) * 1e-3) for r in NRHS}
    rec["sweep_frac_hbm_8TBps"] = {k: v / HBM_PEAK_GBPS for k, v in rec["sweep_GBps"].items()}
    if plain is not None:
        rec["solve_speedup"] = {str(r): median(rec["plain_solve_ms"][str(r)]) / median(rec["solve_ms"][str(r)])
                                for r in NRHS}
        rec["torch_cholesky_ms"] = rec["torch_cholesky_solve_ms"] = None
        try:  # "the caller's own solve" on the output of schur_device
            S = torch.zeros((ns, ns), dtype=torch.float64, device=dev)
            part.schur_device(S, ns)
            sign = -1.0 if kind == "ldlt" else 1.0
            holder = {}

            def t_factor():
                holder["L"] = torch.linalg.cholesky(sign * S)

            def t_solve():
                holder["x"] = torch.cholesky_solve(sign * rhs2[1].T, holder["L"])

            t_factor()
            t_solve()
            torch.cuda.synchronize(dev)
            rec["torch_cholesky_ms"] = [timed(lambda: (t_factor(), torch.cuda.synchronize(dev)), 1)
                                        for _ in range(repeats)]
            rec["torch_cholesky_solve_ms"] = [timed(lambda: (t_solve(), torch.cuda.synchronize(dev)))
                                              for _ in range(repeats)]
        except Exception as e:  # (no dense solver behind this build of torch)
            rec["torch_error"] = str(e)[:200]
        plain.close()
    part.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300, help="grid side; 0: skip the pattern")
    ap.add_argument("--kkt", type=int, nargs=3, default=[20000, 4, 256], metavar=("BLOCKS", "ORDER", "CONSTRAINTS"),
                    help="BLOCKS 0: skip the pattern")
    ap.add_argument("--grid3", type=int, nargs="*", default=[32, 64], help="sides m of the 3-D grids")
    ap.add_argument("--widths", type=int, nargs="*", default=[], help="further panel widths W to time the solves with")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_bench_sparse_schur_solve.jsonl"))
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    patterns = ([grid_line(a.grid)] if a.grid > 0 else []) + ([kkt_blocks(*a.kkt)] if a.kkt[0] > 0 else [])
    patterns += [grid3_plane(m) for m in a.grid3]
    for name, M, schur, kind in patterns:
        for width in [None] + list(a.widths):
            lines.append(json.dumps(run(ctx, name, M, schur, kind, a.repeats, a.inner, width)))
            print(lines[-1], flush=True)
            if a.out:  # (after every record: a run that is cut short keeps what it has)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
