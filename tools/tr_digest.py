"""
Digest of the trust-region layer, one JSON line per configuration: the iteration table without its wall-clock column,
the last table line of the steering ([0]) and QP ([1]) solve of every iteration, z, SHA-256 of x (and zw), getState(),
and what optimize() added to the context's counters -- kernel launches, host-synchronising reductions, polled
completions / collectives, batched reductions, algorithmic bytes.  Two libraries compute the same thing bit for bit, with
the same launches and host round trips, exactly when their outputs are byte-identical:

    PAROPT_AMD_LIB=<one libparopt_amd.so> python tools/tr_digest.py > a.jsonl
    PAROPT_AMD_LIB=<another>              python tools/tr_digest.py > b.jsonl
    cmp a.jsonl b.jsonl

--brief prints, per configuration, the counter deltas and the SHA-256 of the full line instead of the line itself (the
form kept under profiles/): equal files still mean equal full outputs.

Configurations (tests/test_gpu_tr.py has the builders; imported, not copied): every golden case of TR_CASES cut to
MAX_ITERATIONS trust-region iterations -- penalty and filter method, fixed and adaptive gamma, the three steering
objectives and both steering constraints, weighting and CSR constraints, the eigenvalue model with and without a
quasi-Newton part --; qn_type = none; a problem with one dense equality; the 100-column panel of
test_trust_region_with_a_panel_wider_than_one_launch; the object-level assembly with
optimize(ip); the user-written subproblem in Python (CallbackSubproblem, live mirrors, the borrowed model); an
eigenvalue model filled through getArray from a Python callback (release_mirror); the three paths of TR_ON_RECORD.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ip_digest import helpers  # noqa: E402
from sparse_digest import without_time  # noqa: E402

MAX_ITERATIONS = 8


def main():
    import numpy as np

    import paropt_amd as pa
    import sparse_forms_helpers as H
    import test_gpu_tr as T
    from conftest import load_golden
    from test_gpu_mma_dual_linear import equality_problem
    from tr_helpers import TR_REFERENCE_IRREPRODUCIBLE, eig_model, tr_options_from_case

    ctx = pa.Context(0)
    counters, delta, emit = helpers(ctx, "--brief" in sys.argv[1:], ("config", "deltas"))

    def run(name, tr, ip=None, x_of=None):
        lines = []  # [steering, QP] of every iteration (the steering solve of iteration i runs before callback i)

        def cb(i):
            steer, qp = tr.getLastSolveLines()
            if i > 0:
                lines[-1][1] = qp
            lines.append([steer, ""])

        tr.setIterationCallback(cb)
        before = counters()
        tr.optimize(ip)
        d = delta(before)
        if lines:
            lines[-1][1] = tr.getLastSolveLines()[1]
        st = tr.getState()
        state = {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else v) for k, v in sorted(st.items())}
        if ip is None:
            x, z, zw = tr.getOptimizedPoint()
        else:
            x, z, zw = x_of(), ip.getOptimizedPoint()[1], None
        sha = {"x": H.sha(x.to_numpy())}
        if zw is not None and len(zw) > 0:
            sha["zw"] = H.sha(zw.to_numpy())
        emit(config=name, history=without_time(tr.getHistory()), solve_lines=lines, z=np.asarray(z).tolist(),
             sha256=sha, state=state, deltas=d)

    def cut(name):
        g, case = load_golden(name)
        rows = TR_REFERENCE_IRREPRODUCIBLE.get(name, {}).get("rows", MAX_ITERATIONS)
        case["args"]["tr.tr_max_iterations"] = min(rows, MAX_ITERATIONS)
        return case

    for name in T.TR_CASES:
        run(name, T.make_gpu_tr(ctx, cut(name))[1])

    short = {"tr_max_iterations": 6, "qn_subspace_size": 5}
    run("qn_none", pa.TrustRegion(pa.SeparableProblem(ctx, "quadratic", 200, 3), dict(short, qn_type="none")))
    run("dense_equality", pa.TrustRegion(equality_problem(ctx), short))
    run("panel_100_columns", pa.TrustRegion(pa.SeparableProblem(ctx, "quadratic", 400, 70),
                                            {"tr_init_size": 0.1, "tr_max_iterations": 4, "qn_subspace_size": 15}))
    for name in ("tr_eig_quadratic_n200_c2_N4", "tr_rand_eig_quadratic_n257_c3_N5_subcon", "tr_quadratic_n200_c3_bfgs",
                 "tr_convex_n200_c2_w40"):
        tr, ip, sub = T.make_gpu_tr_objects(ctx, cut(name))
        run("objects_" + name, tr, ip, lambda: sub.getLinearModel()[0])

    case = cut("tr_quadratic_n200_c3_bfgs")
    a = case["args"]
    opts, tropts = tr_options_from_case(case)
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"])
    sub = T._user_quadratic_subproblem(pa, prob, pa.LBFGS(ctx, prob.nvars, opts["qn_subspace_size"]))
    run("user_written_subproblem", pa.TrustRegion(sub, tropts), pa.InteriorPoint(sub, opts), lambda: sub.xk)

    case = cut("tr_eig_quadratic_n200_c2_N4")
    run("eigen_model_from_python", T.make_gpu_tr(ctx, case, python_eig_callback=True)[1])
    # ... and written through getArray views that the callback leaves live: uploaded when it returns
    a = case["args"]
    opts, tropts = tr_options_from_case(case)
    prob = pa.SeparableProblem(ctx, a["problem"], a["n"], a["c"])
    Hm, M, Minv = eig_model(a.get("seed", 0), a["eig_N"], a["eig_curv"], prob.nvars, prob.offset)

    def fill(x, e):
        for i in range(a["eig_N"]):
            e.hvecs[i].getArray()[:] = Hm[i] / np.linalg.norm(Hm[i])
        e.M[:, :] = M
        e.Minv[:, :] = Minv

    tr = pa.TrustRegion(prob, dict(opts, **tropts))
    tr.setEigenModel(a["eig_N"], a["eig_index"], fill)
    run("eigen_model_through_get_array", tr)

    for name, rec in sorted(T.TR_ON_RECORD.items()):
        tr, (launches, syncs) = T.optimize_tr_on_record(ctx, rec)
        emit(config="on_record_" + name, history=without_time(tr.getHistory()),
             deltas={"launches": launches, "syncs": syncs})
    ctx.close()


if __name__ == "__main__":
    main()
