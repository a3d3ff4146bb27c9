"""
Digest of MMA.optimize() on a fixed list of small built-in problems, one JSON line per configuration: the full
iteration history, SHA-256 of the bytes of x, zl, zu, L, U, and z, getState(), getDualStats(), getGlobalizationStats()
as they are.  Two libraries compute the same thing bit for bit exactly when their outputs are byte-identical:

    PAROPT_AMD_LIB=<one libparopt_amd.so> python tools/mma_digest.py > a.jsonl
    PAROPT_AMD_LIB=<another>              python tools/mma_digest.py > b.jsonl
    cmp a.jsonl b.jsonl

Every configuration is a SeparableProblem at seed 0 with mma_max_iterations = 6.  The list covers the three ways a
subproblem is solved and, for the dual, every path of its pass: n = 1, an odd tail, the last fused width (c = 8), the
first panel width (c = 9) and the first width past the register-hold capacity (c = 33).
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DUAL = {"mma_subproblem_solver": "dual"}
GCMMA = {"mma_subproblem_solver": "dual", "mma_globalization": "conservative"}
CONFIGS = [
    ("convex", 200, 2, {}),
    ("convex", 200, 2, {"mma_use_constraint_linearization": 1}),
    ("convex", 1, 1, DUAL),
    ("convex", 511, 3, DUAL),
    ("convex", 513, 8, DUAL),
    ("convex", 513, 9, DUAL),
    ("convex", 4097, 33, DUAL),
    ("quadratic", 200, 2, GCMMA),
    ("convex", 513, 9, GCMMA),
    ("convex", 4097, 33, GCMMA),
]


def _plain(d):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}


def digest(pa, ctx, kind, n, c, options):
    mma = pa.MMA(pa.SeparableProblem(ctx, kind, n, c, 0), dict(options, mma_max_iterations=6))
    mma.optimize()
    x, z, _, zl, zu = mma.getOptimizedPoint()
    lo, up = mma.getAsymptotes()
    sha = {name: hashlib.sha256(v.to_numpy().tobytes()).hexdigest()
           for name, v in (("x", x), ("zl", zl), ("zu", zu), ("L", lo), ("U", up))}
    return dict(problem=kind, n=n, c=c, options=options, history=mma.getHistory(), sha256=sha, z=z.tolist(),
                state=_plain(mma.getState()), dual_stats=_plain(mma.getDualStats()),
                globalization_stats=_plain(mma.getGlobalizationStats()))


def main():
    import paropt_amd as pa

    ctx = pa.Context(0)
    for kind, n, c, options in CONFIGS:
        print(json.dumps(digest(pa, ctx, kind, n, c, options), sort_keys=True), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
