"""
The partial factorization of pa.SparseCholesky (a Schur set) beside the plain handle on the same matrix, in one process,
three repeats each, one JSON line per pattern:

    partial_factor_ms      set_values_device + factor() of the handle with the Schur set
    get_schur_ms           schur_device() into a device buffer
    condense_expand_ms     condense_tensor + expand_tensor of one right-hand side
    plain_factor_ms / plain_solve_ms   the plain handle in the SAME elimination order (order "natural" with the Schur
                           handle's perm), so the two differ by the last front alone
    fan_in                 children of the Schur supernode
    gather_ms / chunked_ms the Schur front's assembly ALONE: the table-driven gather launch, and the same sums by
                           chol_assemble_kernel over a chunk list of that front (po_sparse_chol_schur_assembly_probe;
                           `--probe-reps` launches a sample, the front's values are scrap afterwards)

Patterns: the nx x nx five-point grid with one grid line as the Schur set (default 300: ns = 300), and a KKT matrix
[[E, B^T], [B, -I]] with E block-diagonal (default 20 000 blocks of order 4) and 256 constraints that each touch every
block, reduced onto the constraints: the fan-in is the number of blocks.

    python tools/bench_sparse_schur.py [--grid 300] [--kkt 20000 4 256] [--repeats 3] [--inner 3] [--out file.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_line(nx):
    import scipy.sparse as sp

    T = sp.diags([-np.ones(nx - 1), np.full(nx, 2.25), -np.ones(nx - 1)], [-1, 0, 1])
    G = (sp.kron(sp.eye(nx), T) + sp.kron(T, sp.eye(nx))).tocsc()
    G.sort_indices()
    return "5-point grid %dx%d, one grid line" % (nx, nx), G, (nx // 2) * nx + np.arange(nx), "llt"


def kkt_blocks(nblocks, order, ncon):
    import scipy.sparse as sp

    rng = np.random.default_rng(0)
    nE = nblocks * order
    G = rng.standard_normal((nblocks, order, order))
    E = G @ G.transpose(0, 2, 1) / order + np.eye(order)
    B = sp.csr_matrix(rng.uniform(0.1, 1.0, size=(ncon, nE)) / np.sqrt(nE))
    Eb = sp.bsr_matrix((E, np.arange(nblocks), np.arange(nblocks + 1)), shape=(nE, nE))
    K = sp.bmat([[Eb, B.T], [B, -sp.eye(ncon)]]).tocsc()
    K.sort_indices()
    name = "KKT, E = %d blocks of order %d, %d constraints on every block" % (nblocks, order, ncon)
    return name, K, nE + np.arange(ncon), "ldlt"


def run(ctx, name, M, schur, kind, repeats, inner, probe_reps):
    import torch

    import paropt_amd as pa
    from paropt_amd.lib import check, lib

    n = M.shape[0]
    dev = torch.device("cuda", ctx.device())
    t0 = time.perf_counter()
    part = pa.SparseCholesky(ctx, n, M.indptr, M.indices, factorization=kind, schur=schur)
    t_setup = time.perf_counter() - t0
    plain = pa.SparseCholesky(ctx, n, M.indptr, M.indices, order="natural", perm=part.perm, factorization=kind)
    vals = torch.from_numpy(np.ascontiguousarray(M.data)).to(dev)
    ns = part.num_schur
    rhs = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).to(dev)
    work = rhs.clone()
    Sbuf = torch.zeros((ns, ns), dtype=torch.float64, device=dev)

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

    def get_schur():
        part.schur_device(Sbuf, ns)

    def condense_expand():
        work.copy_(rhs)
        part.condense_tensor(work)
        part.expand_tensor(work)  # (the Schur entries hold g, not x2: the time is the same)

    def plain_solve():
        work.copy_(rhs)
        plain.solve_tensor(work)

    def probe(chunked):
        check(lib.po_sparse_chol_schur_assembly_probe(part.handle, chunked, probe_reps))

    info = part.schur_info()
    rec = {"pattern": name, "n": n, "ns": ns, "factorization": kind, "fan_in": info["children"],
           "gather_entries": info["gather_entries"], "snodes": part.num_snodes, "levels": part.nlevels,
           "nnzL": part.nnzL, "work_bytes": part.work_bytes, "setup_s": t_setup, "kernel_forms": part.kernel_forms(),
           "probe_reps": probe_reps}
    # the two assemblies give the same bits: once each on freshly set values
    fronts = []
    for chunked in (0, 1):
        part.set_values_device(vals)
        assert part.factor() == 0
        check(lib.po_sparse_chol_schur_assembly_probe(part.handle, chunked, 1))
        ctx.synchronize()
        part.schur_device(Sbuf, ns)
        fronts.append(Sbuf.cpu().numpy().copy())  # S with the children's updates added once more
    rec["assemblies_bit_equal"] = bool(np.array_equal(fronts[0], fronts[1]))
    for fn in (lambda: factor(part), lambda: factor(plain), get_schur, condense_expand, plain_solve):
        fn()  # warm
    keys = ("partial_factor_ms", "plain_factor_ms", "get_schur_ms", "condense_expand_ms", "plain_solve_ms", "gather_ms",
            "chunked_ms")
    rec.update({k: [] for k in keys})
    for _ in range(repeats):
        rec["partial_factor_ms"].append(timed(lambda: factor(part)))
        rec["plain_factor_ms"].append(timed(lambda: factor(plain)))
        rec["get_schur_ms"].append(timed(get_schur))
        rec["condense_expand_ms"].append(timed(condense_expand))
        rec["plain_solve_ms"].append(timed(plain_solve))
        rec["gather_ms"].append(timed(lambda: probe(0), 1) / probe_reps)
        rec["chunked_ms"].append(timed(lambda: probe(1), 1) / probe_reps)
    rec["chunked_over_gather"] = [a / b for a, b in zip(rec["chunked_ms"], rec["gather_ms"])]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300, help="grid side; 0: skip the pattern")
    ap.add_argument("--kkt", type=int, nargs=3, default=[20000, 4, 256], metavar=("BLOCKS", "ORDER", "CONSTRAINTS"),
                    help="BLOCKS 0: skip the pattern")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--probe-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_bench_sparse_schur.jsonl"))
    a = ap.parse_args()
    import paropt_amd as pa

    ctx = pa.Context(0)
    lines = []
    patterns = ([grid_line(a.grid)] if a.grid > 0 else []) + ([kkt_blocks(*a.kkt)] if a.kkt[0] > 0 else [])
    for name, M, schur, kind in patterns:
        lines.append(json.dumps(run(ctx, name, M, schur, kind, a.repeats, a.inner, a.probe_reps)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
