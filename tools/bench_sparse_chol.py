"""
The multifrontal SparseCholesky against the interior point's row factor on the same matrix: for the grid pattern of
tools/bench_csr_factor.py, S = C + Aw D^-1 Aw^T is built on the host (scipy) and, in one process, alternating, three
repeats each, timed are
    pa.quasidef_factor / pa.quasidef_apply             (CsrSparse, the engine of the interior point)
    SparseCholesky.set_values_device + factor / solve_tensor   on the same S
One JSON line per size.

    python tools/bench_sparse_chol.py [--sizes 150 300] [--repeats 3] [--inner 3] [--out file.jsonl]

--factorization ldlt runs SparseCholesky in its L S L^T mode (the signed kernels and the sign pass of the solve): on the
same SPD S above, and on the --packing matrices with the diagonal negated at every odd-coloured unknown (red/black:
symmetric quasi-definite, half the pivots negative).  Its lines carry "factorization": "ldlt"; without the flag the
output is what it was.

--refine GRID_NX: on the 5-point grid with the red/black diagonal negated, in L S L^T mode with the matrix kept, timed in
one process, alternating, for 1 and 32 right-hand sides: the plain solve, the product y = A x alone (with the GB/s of
the bytes it must move: rowp, col, vidx, the compact values, the two panels), the refined solve stopped after its
first residual pass (max_steps = 0) and after exactly one correction (max_steps = 1, tol = 0); one refinement step
costs the difference of the last two.  One JSON line per number of right-hand sides.
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


def run(ctx, nx, repeats, inner, factorization="llt"):
    import scipy.sparse as sp
    import torch

    import paropt_amd as pa
    from csr_helpers import grid_pattern

    n = nx * nx
    rowp, cols = grid_pattern(nx, nx)
    w = len(rowp) - 1
    rng = np.random.default_rng(0)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))

    class P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=w, nwinequality=w, rowp=rowp, cols=cols)

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = 1.0
            return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x) / n])

        def evalSparseObjConGradient(self, x, g, A, d):
            g[:] = 2.0 * x
            A[0][:] = -1.0 / n
            d[:] = data
            return 0

    prob = P()
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()  # uploads the Jacobian entries

    def vec(arr):
        v = pa.PVec(ctx, len(arr))
        v.from_numpy(arr)
        return v

    dinv, cdiag = rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 1.0, w)
    x, d, c = vec(np.full(n, 0.5)), vec(dinv), vec(cdiag)
    bx, bw = vec(np.zeros(n)), vec(rng.standard_normal(w))
    yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
    Aw = sp.csr_matrix((data, cols, rowp), shape=(w, n))
    S = (sp.diags(cdiag) + Aw @ sp.diags(dinv) @ Aw.T).tocsc()
    S.sort_indices()
    t0 = time.perf_counter()
    chol = pa.SparseCholesky(ctx, w, S.indptr, S.indices)
    if factorization != "llt":
        chol.set_factorization(factorization)
    t_setup = time.perf_counter() - t0
    dev = torch.device("cuda", ctx.device())
    svals = torch.from_numpy(np.ascontiguousarray(S.data)).to(dev)
    rhs = torch.from_numpy(bw.to_numpy().copy()).to(dev)
    work = rhs.clone()
    # warm both engines, and check that they solve the same system
    pa.quasidef_factor(prob, x, d, c)
    pa.quasidef_apply(prob, x, d, c, bx, bw, yx, yw)
    chol.set_values_device(svals)
    assert chol.factor() == 0
    chol.solve_tensor(work)
    ctx.synchronize()
    # [D Aw^T; Aw -C] [yx; -yw] = [0; bw]  =>  yx = D^-1 Aw^T yw and S yw = bw
    diff = float(np.abs(work.cpu().numpy() - yw.to_numpy()).max())
    scale = float(np.abs(yw.to_numpy()).max())

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / inner

    def chol_factor():
        chol.set_values_device(svals)
        chol.factor()

    def chol_solve():
        work.copy_(rhs)
        chol.solve_tensor(work)

    rec = {"pattern": "grid %dx%d" % (nx, nx), "n": w, "nnzS": int(S.nnz), "nnzL_multifrontal": chol.nnzL,
           "nnzL_row": pa.CsrSymbolic(n, rowp, cols).nnzL, "snodes": chol.num_snodes, "levels": chol.nlevels,
           "max_snode": chol.max_snode, "max_front": chol.max_front, "work_bytes": chol.work_bytes,
           "setup_s": t_setup, "solutions_max_abs_diff": diff, "solution_max_abs": scale,
           "quasidef_factor_ms": [], "chol_factor_ms": [], "quasidef_apply_ms": [], "chol_solve_ms": []}
    for _ in range(repeats):
        rec["quasidef_factor_ms"].append(timed(lambda: pa.quasidef_factor(prob, x, d, c)))
        rec["chol_factor_ms"].append(timed(chol_factor))
        rec["quasidef_apply_ms"].append(timed(lambda: pa.quasidef_apply(prob, x, d, c, bx, bw, yx, yw)))
        rec["chol_solve_ms"].append(timed(chol_solve))
    if factorization != "llt":
        rec["factorization"] = factorization
        rec["inertia"] = chol.inertia()
    rec["factor_ratio_row_over_multifrontal"] = [a / b for a, b in zip(rec["quasidef_factor_ms"], rec["chol_factor_ms"])]
    rec["solve_ratio_row_over_multifrontal"] = [a / b for a, b in zip(rec["quasidef_apply_ms"], rec["chol_solve_ms"])]
    return rec


def run_packing(ctx, name, n, colp, rows, vals, repeats, inner, cap=16, factorization="llt"):
    """the public class with its packed groups of tiny fronts switched off (cap 0: a workgroup per front) and with
    groups of at most `cap` fronts, alternating: factor and a solve of one right-hand side"""
    import torch

    import paropt_amd as pa
    from paropt_amd.lib import lib

    dev = torch.device("cuda", ctx.device())
    svals = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
    rhs = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).to(dev)
    work = rhs.clone()
    chol = {}
    packed = "cap%d" % cap
    for key, value in (("cap0", 0), (packed, cap)):
        lib.po_debug_set_switch(38, value)  # core.hpp SW_CHOL_PACK, read by the analysis
        try:
            chol[key] = pa.SparseCholesky(ctx, n, colp, rows)
            if factorization != "llt":
                chol[key].set_factorization(factorization)
        finally:
            lib.po_debug_set_switch(38, -1)

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / inner

    def factor(c):
        c.set_values_device(svals)
        assert c.factor() == 0

    def solve(c):
        work.copy_(rhs)
        c.solve_tensor(work)

    sols = {}
    for key, c in chol.items():
        factor(c)
        solve(c)
        sols[key] = work.cpu().numpy().copy()
    p = chol[packed].packing()
    rec = {"pattern": name, "n": n, "snodes": chol[packed].num_snodes, "levels": chol[packed].nlevels,
           "cap": p["cap"], "groups": p["num_groups"], "factor_levels": p["factor_levels"],
           "kernel_forms": chol[packed].kernel_forms(),
           "bit_equal": bool(np.array_equal(sols["cap0"], sols[packed])),
           "chol_factor_ms": {k: [] for k in chol}, "chol_solve_ms": {k: [] for k in chol}}
    if factorization != "llt":
        rec["factorization"] = factorization
        rec["inertia"] = {k: c.inertia() for k, c in chol.items()}
    for _ in range(repeats):
        for key, c in chol.items():
            rec["chol_factor_ms"][key].append(timed(lambda: factor(c)))
            rec["chol_solve_ms"][key].append(timed(lambda: solve(c)))
    return rec


def run_refine(ctx, nx, repeats, inner):
    import torch

    import paropt_amd as pa

    name, n, colp, rows, vals = list(packing_patterns(8, nx, quasi_definite=True))[1]
    dev = torch.device("cuda", ctx.device())
    chol = pa.SparseCholesky(ctx, n, colp, rows, factorization="ldlt", keep_matrix=True)
    chol.set_values_device(torch.from_numpy(np.ascontiguousarray(vals)).to(dev))
    assert chol.factor() == 0
    rowp, col, vidx, nd = chol.matrix_arrays()
    matrix_bytes = 4 * (len(rowp) + len(col) + len(vidx)) + 8 * nd

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / inner

    for nrhs in (1, 32):
        rhs = torch.from_numpy(np.random.default_rng(nrhs).standard_normal((nrhs, n))).to(dev)
        work, out = rhs.clone(), torch.zeros_like(rhs)
        stats = {}

        def solve():
            work.copy_(rhs)
            chol.solve_tensor(work)

        def product():
            chol.matvec_tensor(rhs, out)

        def refined(max_steps):
            work.copy_(rhs)
            stats[max_steps] = chol.solve_refined_tensor(work, max_steps=max_steps, tol=0.0)[1]

        fns = (("solve_ms", solve), ("product_ms", product), ("refined_0_steps_ms", lambda: refined(0)),
               ("refined_1_step_ms", lambda: refined(1)))
        for _, fn in fns:
            fn()  # warm
        product_bytes = matrix_bytes + 2 * 8 * n * nrhs
        rec = {"pattern": name, "n": n, "nnzA": int(rowp[-1]), "longest_row": int(np.diff(rowp).max()), "nrhs": nrhs,
               "factorization": "ldlt", "levels": chol.nlevels, "product_bytes": product_bytes,
               "eta0": float(stats[1]["eta0"].max()), "eta_after_one_step": float(stats[1]["eta"].max())}
        rec.update({k: [] for k, _ in fns})
        for _ in range(repeats):
            for k, fn in fns:
                rec[k].append(timed(fn))
        rec["product_GBps"] = [1e-6 * product_bytes / t for t in rec["product_ms"]]
        rec["one_step_ms"] = [b - a for a, b in zip(rec["refined_0_steps_ms"], rec["refined_1_step_ms"])]
        rec["one_step_over_solve"] = [a / b for a, b in zip(rec["one_step_ms"], rec["solve_ms"])]
        yield rec


def packing_patterns(tridiag_n, nx, quasi_definite=False):
    import scipy.sparse as sp

    T = sp.diags([-np.ones(tridiag_n - 1), np.full(tridiag_n, 2.5), -np.ones(tridiag_n - 1)], [-1, 0, 1]).tocsc()
    G = sp.kron(sp.eye(nx), sp.diags([-np.ones(nx - 1), np.full(nx, 2.25), -np.ones(nx - 1)], [-1, 0, 1]))
    G = (G + sp.kron(sp.diags([-np.ones(nx - 1), np.full(nx, 2.25), -np.ones(nx - 1)], [-1, 0, 1]), sp.eye(nx))).tocsc()
    for name, M in (("tridiagonal n=%d" % tridiag_n, T), ("5-point grid %dx%d" % (nx, nx), G)):
        if quasi_definite:  # negate the diagonal at the odd colour of the red/black colouring
            k = np.arange(M.shape[0])
            odd = (k % 2 == 1) if M is T else ((k // nx + k % nx) % 2 == 1)
            M = (M - 2.0 * sp.diags(np.where(odd, M.diagonal(), 0.0))).tocsc()
        M.sort_indices()
        yield name, M.shape[0], M.indptr, M.indices, M.data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packing", type=int, nargs=2, default=None, metavar=("TRIDIAG_N", "GRID_NX"),
                    help="also one line each for a tridiagonal and a 5-point grid matrix on the public class, "
                         "packed groups off against groups of at most 16 fronts")
    ap.add_argument("--sizes", type=int, nargs="*", default=[150, 300])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--factorization", choices=("llt", "ldlt"), default="llt")
    ap.add_argument("--refine", type=int, default=None, metavar="GRID_NX",
                    help="only the refined solve beside the plain one and the product (see above)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    if a.refine:
        a.sizes = []
        for rec in run_refine(ctx, a.refine, a.repeats, a.inner):
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    for nx in a.sizes:
        lines.append(json.dumps(run(ctx, nx, a.repeats, a.inner, factorization=a.factorization)))
        print(lines[-1], flush=True)
    if a.packing:
        for name, n, colp, rows, vals in packing_patterns(*a.packing, quasi_definite=a.factorization == "ldlt"):
            lines.append(json.dumps(run_packing(ctx, name, n, colp, rows, vals, a.repeats, a.inner,
                                                factorization=a.factorization)))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
