"""
Digest of the sparse-constraint path, one JSON line per configuration, for every form of the quasi-definite solver
(paropt_amd/csrc/quasidef.hpp) and for the three problems that wrap a user's problem.  Two libraries compute the same
thing bit for bit exactly when their outputs are byte-identical:

    PAROPT_AMD_LIB=<one libparopt_amd.so> python tools/sparse_digest.py > a.jsonl
    PAROPT_AMD_LIB=<another>              python tools/sparse_digest.py > b.jsonl
    cmp a.jsonl b.jsonl

Per form (tests/sparse_forms_helpers.py has the problems): SHA-256 of (yx, yw) of po_quasidef_factor +
po_quasidef_apply on fixed inputs, quasidef_factor_info, and a six-iteration InteriorPoint.optimize(): its history
and SHA-256 of x, zl, zu, the five sparse blocks, z.  The kernel launches of each step are recorded as well: equal bits
do not tell a fused form from the unfused sequence it replaces, the launch count does.  The grouped and CSR problems
also run four iterations under TrustRegion (quadratic subproblem; the steering problem rides along; the table without
its wall-clock column), MMA with the interior-point sub-solver and MMA with mma_dual_sparse_constraints = groups.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def without_time(history):
    """the trust-region table without its wall-clock column (ten characters ending where the header's time(s) ends)"""
    lines = history.splitlines()
    end = max((ln.find("time(s)") for ln in lines), default=-1) + len("time(s)")
    if end < len("time(s)"):
        return history
    return "\n".join(ln[:end - 10] + ln[end:] if len(ln) >= end else ln for ln in lines)


def main():
    import numpy as np

    import paropt_amd as pa
    import sparse_forms_helpers as H
    from test_gpu_quasidef_user import BlockSolver, DenseSolver, DiagonalSolver

    ctx = pa.Context(0)

    def diagonal(p):
        return DiagonalSolver(H.po.SepProblem("convex", H.N, 2, nwcon=60, nw=H.NW).sparse_jacobian_dense())

    forms = [
        ("grouped", lambda: H.grouped(ctx), None),
        ("grouped_skip1", lambda: H.grouped(ctx, 1), None),
        ("csr_groups", lambda: H.csr_groups(ctx), None),
        ("csr_groups_skip1", lambda: H.csr_groups(ctx, 1), None),
        ("csr_fallback", lambda: H.csr_groups(ctx, differ_after=3), None),
        ("csr", lambda: H.csr_chain(ctx), None),
        ("scalar", lambda: H.scalar(ctx), None),
        ("block2", lambda: H.block(ctx, 2), None),
        ("block3", lambda: H.block(ctx, 3), None),
        ("user_on_grouped", lambda: H.grouped(ctx), diagonal),
        ("user_on_csr", lambda: H.csr_chain(ctx), DenseSolver),
        ("user_on_block3", lambda: H.block(ctx, 3), lambda p: BlockSolver(H.block_jacobian(3), 3)),
    ]

    def make(build, solver):
        p = build()
        if solver:
            p.setQuasiDefMat(solver(p))
        return p

    def emit(**rec):
        print(json.dumps(rec, sort_keys=True), flush=True)

    for name, build, solver in forms:
        p = H.upload_entries(make(build, solver))
        launches = []
        yx, yw = H.factor_and_apply(ctx, p, launches=launches)
        yx0, yw0 = H.factor_and_apply(ctx, p, with_bw=False)
        rec = dict(form=name, apply={"yx": H.sha(np.frombuffer(yx)), "yw": H.sha(np.frombuffer(yw)),
                                     "yx_no_bw": H.sha(np.frombuffer(yx0)), "yw_no_bw": H.sha(np.frombuffer(yw0))},
                   info=pa.quasidef_factor_info(p), launches_factor_apply=launches)
        p = make(build, solver)
        ip = pa.InteriorPoint(p, H.IP_OPTS)
        n0 = ctx.counters()[1]
        ip.optimize()
        rec["launches_optimize"] = ctx.counters()[1] - n0
        x, z, zl, zu = ip.getOptimizedPoint()
        vecs = [("x", x), ("zl", zl), ("zu", zu)] + list(zip(("zw", "sw", "tw", "zsw", "ztw"), ip.getOptimizedSparse()))
        rec.update(history=ip.getHistory(), z=np.asarray(z).tolist(), info_after=pa.quasidef_factor_info(p),
                   sha256={k: H.sha(v.to_numpy()) for k, v in vecs})
        emit(**rec)

    wrapped = [("grouped", lambda: H.grouped(ctx)), ("grouped_skip1", lambda: H.grouped(ctx, 1)),
               ("csr_groups", lambda: H.csr_groups(ctx)), ("csr", lambda: H.csr_chain(ctx))]
    for name, build in wrapped:
        tr = pa.TrustRegion(build(), {"tr_max_iterations": 4, "qn_subspace_size": 4})
        n0 = ctx.counters()[1]
        tr.optimize()
        launches = ctx.counters()[1] - n0
        x, z, zw = tr.getOptimizedPoint()[:3]
        emit(form=name, wrapper="tr", history=without_time(tr.getHistory()), z=np.asarray(z).tolist(),
             launches=launches, sha256={"x": H.sha(x.to_numpy()), "zw": H.sha(zw.to_numpy())})
        runs = [("mma", {})]
        if name != "csr":  # the dual takes sparse constraints in the grouped form only
            runs.append(("mma_dual_groups", {"mma_subproblem_solver": "dual", "mma_dual_sparse_constraints": "groups"}))
        for wrapper, options in runs:
            mma = pa.MMA(build(), dict(options, mma_max_iterations=4))
            n0 = ctx.counters()[1]
            mma.optimize()
            launches = ctx.counters()[1] - n0
            x, z, zw, zl, zu = mma.getOptimizedPoint()
            emit(form=name, wrapper=wrapper, history=mma.getHistory(), z=np.asarray(z).tolist(), launches=launches,
                 sha256={k: H.sha(v.to_numpy()) for k, v in (("x", x), ("zw", zw), ("zl", zl), ("zu", zu))})
    ctx.close()


if __name__ == "__main__":
    main()
