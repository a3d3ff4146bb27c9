"""The multifrontal engine under the interior point with packed groups of tiny fronts: the quasi-definite solve, the
Gram panels and a whole interior-point run are bit for bit what the unpacked kernels (cap 0) give."""
import numpy as np
import pytest

from sparse_chol_packing_helpers import csr_patterns, pack_cap, pattern_problem

pytestmark = pytest.mark.gpu

NV = (1, 21, 33, 97)


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def _vec(ctx, arr):
    import paropt_amd as pa

    return pa.PVec(ctx, len(arr)).from_numpy(np.asarray(arr, dtype=float))


def solves(ctx, name, cap):
    """factor, one apply with bw and the Gram panels of every width on a fresh problem analysed under `cap`"""
    import paropt_amd as pa

    n, rowp, cols, min_rows = csr_patterns()[name]
    w = len(rowp) - 1
    rng = np.random.default_rng(5)
    data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))
    with pack_cap(cap):
        sym = pa.CsrSymbolic(n, rowp, cols, dense_column_rows=min_rows, sparse_factor="multifrontal")
        prob, A = pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=min_rows)
    p = sym.frontal_packing()
    assert p["cap"] == cap and (p["num_groups"] > 0) == (cap > 0)
    d, c = rng.uniform(0.2, 3.0, size=n), rng.uniform(0.5, 2.0, size=w)
    x, dv, cv = _vec(ctx, np.full(n, 0.5)), _vec(ctx, d), _vec(ctx, c)
    pa.quasidef_factor(prob, x, dv, cv)
    bx, bw = rng.standard_normal(n), rng.standard_normal(w)
    yx, yw = pa.PVec(ctx, n), pa.PVec(ctx, w)
    pa.quasidef_apply(prob, x, dv, cv, _vec(ctx, bx), _vec(ctx, bw), yx, yw)
    out = {"yx": yx.to_numpy(), "yw": yw.to_numpy()}
    # and against the dense S, so that equal bits are not equal nonsense
    S = np.diag(c) + (A * d) @ A.T
    yw_ref = np.linalg.solve(S, bw - A @ (d * bx))
    np.testing.assert_allclose(out["yw"], yw_ref, rtol=0, atol=1e-10 * max(1.0, np.abs(yw_ref).max()))
    V = [pa.PVec(ctx, n).fill_hash(0, 20 + j, 0, 2.0, -1.0 + 0.01 * j) for j in range(max(NV))]
    for nv in NV:
        alpha = np.random.default_rng(nv).standard_normal(nv)
        W2, corr = pa.quasidef_gram(prob, x, dv, cv, V[:nv], alpha=alpha)
        out["W%d" % nv], out["corr%d" % nv] = np.array(W2), corr.to_numpy()
    return out, p


@pytest.mark.parametrize("name", sorted(csr_patterns()))
def test_apply_and_gram_equal_cap_0(ctx, name):
    ref, _ = solves(ctx, name, 0)
    assert all(np.isfinite(v).all() for v in ref.values())
    for cap in (2, 16):
        got, p = solves(ctx, name, cap)
        assert (p["group_root"] > p["group_first"]).any(), (name, cap)
        for key in ref:
            assert np.array_equal(got[key], ref[key]), (name, cap, key, float(np.abs(got[key] - ref[key]).max()))


def test_interior_point_run_equals_cap_0(ctx):
    import paropt_amd as pa

    opts = {"abs_res_tol": 1e-8, "starting_point_strategy": "affine_step", "barrier_strategy": "monotone",
            "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0, "qn_subspace_size": 6, "qn_type": "bfgs",
            "max_major_iters": 12}  # tests/test_gpu_csr.py, cut short
    runs = {}
    for cap in (0, 16):
        with pack_cap(cap):
            prob = pa.SeparableProblem(ctx, "convex", 500, 3).setChain(3, 2, True, sparse_factor="multifrontal")
            ip = pa.InteriorPoint(prob, opts)
            ip.optimize()
        assert "nsnodes" in pa.quasidef_factor_info(prob)
        runs[cap] = (tuple(ip.getIterationCounters()), ip.getObjective()[0], ip.getOptimizedPoint()[0].to_numpy(),
                     ip.getOptimizedSparse()[0].to_numpy())
    assert runs[0][0] == runs[16][0] and runs[0][0][0] > 0
    assert runs[0][1] == runs[16][1]
    assert np.array_equal(runs[0][2], runs[16][2]) and np.array_equal(runs[0][3], runs[16][3])
