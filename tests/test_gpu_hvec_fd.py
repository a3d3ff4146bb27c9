"""
Hessian-vector products by differences of the Lagrangian's gradient (InteriorPoint.setHvecFiniteDifference): the inexact
Newton-Krylov step (use_hvec_product) for problems that have no evalHvecProduct.

The yardsticks:
  * the SAME difference formula evaluated in numpy from the oracle's eval_obj_con_gradient (fd_hvec below), with the
    step size the device reports, agreement per element within
        64 eps (|g|_inf + sum_j |z_j| |A_j|_inf + |Aw^T zw|_inf) / h
    -- the cancellation error of a difference of two gradients of that size, divided by the step;
  * the exact product SepProblem.hvec_product: the device's error against it is at most 10 x the error the numpy
    evaluation itself has against it (floor: the bound above);
  * the oracle's interior point with hvec_product patched to that formula, for whole trajectories on the two problems
    where they are stable (rosenbrock n = 100, quadratic n = 500 c = 4 L-BFGS(6): the counters of exact and differenced
    products are equal, forward and central form alike).
"""
import json
import os
import socket
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "newton_krylov_fd_amd")
EPS = np.finfo(np.float64).eps

# the options of the Newton-Krylov runs: the Krylov step from the first iteration on
NK = {"use_hvec_product": True, "gmres_subspace_size": 15, "nk_switch_tol": 1e3, "max_gmres_rtol": 1.0}
STABLE = [("rosenbrock", 100, 2, {}), ("quadratic", 500, 4, {"qn_subspace_size": 6})]


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


# ---- the difference formula in numpy ---------------------------------------------------------------------------------
def fd_step(op, lb, ub, x, px, central, rel=None, max_bound=1e20):
    """h = min(rel (1 + |x|) / |p|, half the step to the nearest bound along p [and along -p, central form])."""
    if rel is None:
        rel = np.cbrt(EPS) if central else np.sqrt(EPS)
    s = op.comm.allreduce(np.array([np.dot(x, x), np.dot(px, px)]))
    if s[1] == 0.0:
        return 0.0
    ap = np.abs(px)
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = np.where((lb > -max_bound) & (ap > 0), (x - lb) / ap, np.inf)
        tu = np.where((ub < max_bound) & (ap > 0), (ub - x) / ap, np.inf)
    fwd = np.where(px > 0, tu, tl)
    bwd = np.where(px > 0, tl, tu)
    to_bound = min(fwd.min(), bwd.min()) if central else fwd.min()
    return min(rel * (1.0 + np.sqrt(s[0])) / np.sqrt(s[1]), 0.5 * to_bound)


def fd_hvec(op, x, z, px, zw, central, h):
    """s ((g+ - g-) - sum_j z_j (A+_j - A-_j)) - s Aw(x+)^T zw + s Aw(x-)^T zw: every pair subtracted first."""
    if h == 0.0:
        return np.zeros_like(x)
    s = 0.5 / h if central else 1.0 / h
    has_w = op.nwcon > 0 and zw is not None
    saved = (getattr(op, "_cw", None), getattr(op, "_jac", None))
    hv = np.zeros_like(x)

    def at(y, sign):
        op.eval_obj_con(y)  # values first, then the gradient: the order the solver keeps
        _, g, A = op.eval_obj_con_gradient(y)
        if has_w:
            op.add_sparse_jacobian_transpose(sign * s, zw, hv)
        return g, A

    gp, Ap = at(x + h * px, -1.0)
    gm, Am = at(x - h * px if central else x, 1.0)
    if saved[0] is not None:
        op._cw, op._jac = saved
    acc = gp - gm
    for j in range(op.c):
        acc = acc - z[j] * (Ap[j] - Am[j])
    return hv + s * acc


def cancellation_bound(op, x, z, zw, h):
    op.eval_obj_con(x)
    _, g, A = op.eval_obj_con_gradient(x)
    size = np.abs(g).max() + sum(abs(z[j]) * np.abs(A[j]).max() for j in range(op.c))
    if op.nwcon > 0 and zw is not None:
        size += np.abs(op.add_sparse_jacobian_transpose(1.0, zw, np.zeros_like(x))).max()
    return 64.0 * EPS * size / h


def oracle_run(kind, n, c, extra, fd=None):
    """The oracle's interior point with exact products (fd None) or with hvec_product patched to the formula above."""
    from oracle import paropt_oracle as po

    op = po.SepProblem(kind, n, c)
    if fd is not None:
        _, lb, ub = op.vars_and_bounds()
        op.hvec_product = lambda x, z, px, zw=None: fd_hvec(op, x, z, px, zw, fd, fd_step(op, lb, ub, x, px, fd))
    ip = po.InteriorPoint(op, dict(NK, **extra))
    ip.optimize()
    return (ip.niter, ip.neval, ip.ngeval, ip.nhvec), ip.vars.x.copy()


def device_run(ctx, prob, extra, mode=None, central=False, **more):
    import paropt_amd as pa

    ip = pa.InteriorPoint(prob, dict(NK, write_output_frequency=0, **extra, **more))
    if mode is not None:
        ip.setHvecFiniteDifference(mode, central=central)
    ip.optimize()
    return ip, ip.getIterationCounters() + (ip.getHvecCount(),), ip.getOptimizedPoint()[0].to_numpy()


def rosen_python(ctx, n, with_hvec=False):
    """The oracle's rosenbrock as a Python problem with first derivatives only (evalHvecProduct on request)."""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    op = po.SepProblem("rosenbrock", n, 2)

    class Rosen(pa.Problem):
        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = -1.0, -2.0, 1.0

        def evalObjCon(self, x):
            return op.eval_obj_con(x)

        def evalObjConGradient(self, x, g, A):
            _, gg, aa = op.eval_obj_con_gradient(x)
            g[:] = gg
            A[0][:], A[1][:] = aa[0], aa[1]
            return 0

    if with_hvec:
        def hv(self, x, z, zw, px, hvec):
            hvec[:] = op.hvec_product(x, z, px)
            return 0

        Rosen.evalHvecProduct = hv
    return Rosen(ctx, n, 2)


# ---- 1. fails today ------------------------------------------------------------------------------------------------------
def test_problem_without_hvec_product_runs_newton_krylov(ctx):
    import paropt_amd as pa

    n = 100
    # the default must not move: a problem without the product ends the run with today's error
    ip0 = pa.InteriorPoint(rosen_python(ctx, n), dict(NK, write_output_frequency=0))
    with pytest.raises(pa.ParOptAMDError, match="evalHvecProduct failed or is not provided"):
        ip0.optimize()
    assert ip0.getHvecFiniteDifferenceCount() == (0, 0)
    ref_counters, ref_x = oracle_run("rosenbrock", n, 2, {})
    for central in (False, True):
        ip, counters, x = device_run(ctx, rosen_python(ctx, n), {}, "when_missing", central, max_major_iters=200)
        print("when_missing central=%s counters %s oracle(exact) %s max|dx| %.3e" % (
            central, counters, ref_counters, np.abs(x - ref_x).max()))
        assert counters[0] < 200 and "iNK" in ip.getHistory()  # stopped by its own criterion, on Krylov steps
        assert counters == ref_counters
        np.testing.assert_allclose(x, ref_x, rtol=0, atol=1e-6)
        products, evals = ip.getHvecFiniteDifferenceCount()
        assert products == counters[3] and evals == (2 if central else 1) * products
    # a problem that HAS the product keeps using it under when_missing
    ip, counters, x = device_run(ctx, rosen_python(ctx, n, with_hvec=True), {}, "when_missing")
    assert counters == ref_counters and ip.getHvecFiniteDifferenceCount() == (0, 0)


# ---- 2. the product itself -----------------------------------------------------------------------------------------------
PRODUCT_CASES = [
    ("quadratic", 500, 4, None, None),
    ("convex", 640, 3, None, None),
    ("rosenbrock", 100, 2, None, None),
    ("rosenbrock", 101, 2, (2, 1), None),       # CSR form, overlapping nonlinear rows (odd n: the padded pair)
    ("convex", 640, 3, (3, 2), None),           # CSR form
    ("convex", 640, 3, None, (32, 20, 0, 0)),   # weighting constraints (structured form)
    ("quadratic", 480, 2, None, (40, 5, 1, 1)),
]


def _sep_pair(ctx, kind, n, c, chain, wgt):
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    prob = pa.SeparableProblem(ctx, kind, n, c)
    kw = {}
    if chain:
        prob.setChain(*chain)
        kw["chain"] = chain
    if wgt:
        prob.setWeighting(*wgt)
        kw.update(nwcon=wgt[0], nw=wgt[1], nwstart=wgt[2], nwskip=wgt[3])
    return prob, po.SepProblem(kind, n, c, **kw)


def _at_an_iterate(ctx, prob, iters=3):
    """A solver stopped after a few iterations: strictly inside the bounds, far from a stationary point."""
    import paropt_amd as pa

    ip = pa.InteriorPoint(prob, {"qn_subspace_size": 5, "max_major_iters": iters, "write_output_frequency": 0,
                                 "start_affine_multiplier_min": 0.01})
    ip.optimize()
    return ip


@pytest.mark.parametrize("kind,n,c,chain,wgt", PRODUCT_CASES)
@pytest.mark.parametrize("central", [False, True])
def test_differenced_product_against_numpy_and_exact(ctx, kind, n, c, chain, wgt, central):
    import paropt_amd as pa

    prob, op = _sep_pair(ctx, kind, n, c, chain, wgt)
    ip = _at_an_iterate(ctx, prob)
    x = ip.getOptimizedPoint()[0].to_numpy()
    lb, ub = (v.to_numpy() for v in ip.getBounds())
    rng = np.random.default_rng(7 + n + (1 if central else 0))
    px = rng.standard_normal(n)
    z = rng.uniform(0.1, 2.0, op.c)
    zw = rng.uniform(0.1, 2.0, op.nwcon) if op.nwcon else None
    vpx, vh = pa.PVec(ctx, n).from_numpy(px), pa.PVec(ctx, n)
    vzw = pa.PVec(ctx, op.nwcon).from_numpy(zw) if op.nwcon else None
    ip.setHvecFiniteDifference("always", central=central)
    dev = ip.evalHvec(z, vzw, vpx, vh).to_numpy()
    h = ip.getHvecFiniteDifferenceStep()
    h_np = fd_step(op, lb, ub, x, px, central)
    assert h > 0.0 and abs(h - h_np) <= 1e-12 * h_np, (h, h_np)
    assert np.all(x + h * px > lb) and np.all(x + h * px < ub)
    ref = fd_hvec(op, x, z, px, zw, central, h)
    bound = cancellation_bound(op, x, z, zw, h)
    exact = op.hvec_product(x, z, px, zw)
    err_a = np.abs(dev - ref).max()
    err_dev, err_np = np.abs(dev - exact).max(), np.abs(ref - exact).max()
    print("%s n=%d chain=%s wgt=%s central=%s: h %.3e |dev-numpy| %.3e bound %.3e |dev-exact| %.3e |numpy-exact| %.3e "
          "|H p| %.3e" % (kind, n, chain, wgt, central, h, err_a, bound, err_dev, err_np, np.abs(exact).max()))
    assert np.all(np.abs(dev - ref) <= bound), (err_a, bound)
    assert err_dev <= max(10.0 * err_np, bound), (err_dev, err_np, bound)
    assert ip.getHvecFiniteDifferenceCount() == (1, 2 if central else 1)


# ---- 3. the state of the iterate is restored ---------------------------------------------------------------------------
def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


@pytest.mark.parametrize("kind,n,c,chain,wgt", PRODUCT_CASES[2:6])
@pytest.mark.parametrize("central", [False, True])
def test_product_leaves_the_iterate_alone(ctx, kind, n, c, chain, wgt, central):
    import paropt_amd as pa

    prob, op = _sep_pair(ctx, kind, n, c, chain, wgt)
    ip = _at_an_iterate(ctx, prob, iters=4)
    rng = np.random.default_rng(11)
    vpx, vh1, vh2 = pa.PVec(ctx, n).from_numpy(rng.standard_normal(n)), pa.PVec(ctx, n), pa.PVec(ctx, n)
    z = rng.uniform(0.1, 2.0, op.c)
    vzw = pa.PVec(ctx, op.nwcon).from_numpy(rng.uniform(0.1, 2.0, op.nwcon)) if op.nwcon else None
    ip.setHvecFiniteDifference("always", central=central)
    snap0, ints0 = ip.snapshot(), ip.getDebugInts()
    x0 = ip.getOptimizedPoint()[0].to_numpy()
    data0 = prob.getSparseJacobianData()[2] if chain else None
    h1 = ip.evalHvec(z, vzw, vpx, vh1).to_numpy()
    h2 = ip.evalHvec(z, vzw, vpx, vh2).to_numpy()
    np.testing.assert_array_equal(h1, h2)
    _same_bits(snap0, ip.snapshot())
    _same_bits(ints0, ip.getDebugInts())
    np.testing.assert_array_equal(x0, ip.getOptimizedPoint()[0].to_numpy())
    if chain:
        np.testing.assert_array_equal(data0, prob.getSparseJacobianData()[2])
    # ... and the solver goes on from that state exactly as a solver that took no product: the next solve starts from
    # the problem's starting point, so only what the PROBLEM holds (CSR values, constraint values) could differ
    prob2, _ = _sep_pair(ctx, kind, n, c, chain, wgt)
    ip2 = _at_an_iterate(ctx, prob2, iters=4)
    ip.setHvecFiniteDifference("exact")
    ip.optimize()
    ip2.optimize()
    _same_bits(ip.snapshot(), ip2.snapshot())


def test_recognised_weighting_pattern_in_csr_form(ctx):
    """A torch problem in the CSR form whose pattern the library recognises as the grouped one: the views of the
    library's value array and constraint vector show that both hold the iterate's values again after a product."""
    import torch

    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n, c, nwcon, nw = 640, 3, 32, 20
    op = po.SepProblem("convex", n, c, nwcon=nwcon, nw=nw)
    rowp = np.arange(nwcon + 1, dtype=np.intc) * nw
    cols = ((np.arange(nwcon)[:, None] * nw) + np.arange(nw)[None, :]).astype(np.intc).ravel()
    views = {}

    def put(dst, val):
        dst.copy_(torch.from_numpy(np.array(np.broadcast_to(val, dst.shape), dtype=np.float64)))

    class P(pa.TorchProblem):
        def getVarsAndBounds(self, x, lb, ub):
            x0, l0, u0 = op.vars_and_bounds()
            put(x, x0), put(lb, l0), put(ub, u0)

        def evalSparseObjCon(self, x, sparse):
            xs = x.cpu().numpy()
            fail, f, con = op.eval_obj_con(xs)
            put(sparse, op.eval_sparse_con(xs))
            views["cw"] = sparse
            return fail, f, con

        def evalSparseObjConGradient(self, x, g, A, data):
            _, gg, aa = op.eval_obj_con_gradient(x.cpu().numpy())
            put(g, gg)
            for j in range(c):
                put(A[j], aa[j])
            data[:] = -1.0
            views["data"] = data
            return 0

    prob = P(ctx, n, c, c, nwcon=nwcon, nwinequality=nwcon, rowp=rowp, cols=cols)
    ip = _at_an_iterate(ctx, prob, iters=4)
    x = ip.getOptimizedPoint()[0].to_numpy()
    rng = np.random.default_rng(5)
    px, z, zw = rng.standard_normal(n), rng.uniform(0.1, 2.0, c), rng.uniform(0.1, 2.0, nwcon)
    vpx, vzw = pa.PVec(ctx, n).from_numpy(px), pa.PVec(ctx, nwcon).from_numpy(zw)
    for central in (False, True):
        ip.setHvecFiniteDifference("always", central=central)
        ctx.synchronize()
        cw0, data0 = views["cw"].clone(), views["data"].clone()
        snap0 = ip.snapshot()
        h1 = ip.evalHvec(z, vzw, vpx, pa.PVec(ctx, n)).to_numpy()
        h2 = ip.evalHvec(z, vzw, vpx, pa.PVec(ctx, n)).to_numpy()
        ctx.synchronize()
        np.testing.assert_array_equal(h1, h2)
        assert torch.equal(views["cw"], cw0) and torch.equal(views["data"], data0)
        _same_bits(snap0, ip.snapshot())
        h = ip.getHvecFiniteDifferenceStep()
        ref = fd_hvec(op, x, z, px, zw, central, h)
        assert np.all(np.abs(h1 - ref) <= cancellation_bound(op, x, z, zw, h))


# ---- 4. trajectories where they are stable -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,c,extra", STABLE)
@pytest.mark.parametrize("central", [False, True])
def test_trajectory_follows_the_patched_oracle(ctx, tmp_path, kind, n, c, extra, central):
    import paropt_amd as pa
    from paropt_amd import ParOpt

    ref_counters, ref_x = oracle_run(kind, n, c, extra, fd=central)
    exact_counters, _ = oracle_run(kind, n, c, extra)
    outfile = str(tmp_path / "paropt.out")
    ip, counters, x = device_run(ctx, pa.SeparableProblem(ctx, kind, n, c), extra, "always", central,
                                 output_file=outfile)
    _, builtin_exact, _ = device_run(ctx, pa.SeparableProblem(ctx, kind, n, c), extra)
    print("%s central=%s: device %s oracle(same formula) %s oracle(exact) %s built-in(exact) %s max|dx| %.3e" % (
        kind, central, counters, ref_counters, exact_counters, builtin_exact, np.abs(x - ref_x).max()))
    assert counters == ref_counters
    np.testing.assert_allclose(x, ref_x, rtol=0, atol=1e-6)
    assert counters == builtin_exact == exact_counters
    products, evals = ip.getHvecFiniteDifferenceCount()
    assert products == counters[3] > 0 and evals == (2 if central else 1) * products
    names, cols = ParOpt.unpack_output(outfile)
    assert names[3] == "nhvc" and cols[3][-1] == counters[3]
    assert cols[1][-1] == counters[1] and cols[2][-1] == counters[2]  # the extra evaluations are not in neval / ngeval


@pytest.mark.parametrize("central", [False, True])
def test_flat_problem_converges(ctx, central):
    """convex n = 640, c = 3, L-BFGS(6): a flat problem on which exact and differenced runs part ways (120 against 94
    iterations in the oracle): convergence to the solver's own stop only."""
    import paropt_amd as pa

    ip, counters, x = device_run(ctx, pa.SeparableProblem(ctx, "convex", 640, 3), {"qn_subspace_size": 6}, "always",
                                 central, max_major_iters=1000)
    print("convex central=%s: counters %s" % (central, counters))
    assert counters[0] < 1000 and counters[3] > 0
    assert ip.getHvecFiniteDifferenceCount()[0] == counters[3]


# ---- 5. boundaries -------------------------------------------------------------------------------------------------------
def _rosen_torch(ctx, n, device_results):
    import torch

    import paropt_amd as pa

    class RosenTorch(pa.TorchProblem):
        def getVarsAndBounds(self, x, lb, ub):
            x.fill_(-1.0), lb.fill_(-2.0), ub.fill_(1.0)

        def evalObjCon(self, x):
            r = x[1:] - x[:-1] ** 2
            f = ((1.0 - x[:-1]) ** 2 + 100.0 * r * r).sum()
            con = torch.stack([0.25 - (x * x).sum(), 10.0 + x[::2].sum()])
            if device_results:
                return 0, f, con
            return 0, float(f), con.cpu().numpy()

        def evalObjConGradient(self, x, g, A):
            r = x[1:] - x[:-1] ** 2
            g.zero_()
            g[:-1] += -2.0 * (1.0 - x[:-1]) - 400.0 * r * x[:-1]
            g[1:] += 200.0 * r
            A[0].copy_(-2.0 * x)
            A[1].zero_()
            A[1][::2] = 1.0
            return 0

    return RosenTorch(ctx, n, 2)


@pytest.mark.parametrize("central", [False, True])
def test_torch_problem_and_facade_example(ctx, tmp_path, central):
    n = 100
    ref_counters, ref_x = oracle_run("rosenbrock", n, 2, {}, fd=central)
    for deferred in (False, True):
        prob = _rosen_torch(ctx, n, device_results=deferred)
        if deferred:
            prob.setDeferredReductions(True)
        for mode in ("when_missing", "always"):
            ip, counters, x = device_run(ctx, prob, {}, mode, central)
            assert counters == ref_counters, (deferred, mode)
            np.testing.assert_allclose(x, ref_x, rtol=0, atol=1e-6)
            assert ip.getHvecFiniteDifferenceCount() == (counters[3], (2 if central else 1) * counters[3])
    assert os.path.exists(EXAMPLE), "examples/newton_krylov_fd_amd is built by build()"
    res = subprocess.run([EXAMPLE, "nvars=%d" % n, "central=%d" % int(central)], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    d = json.loads(res.stdout.strip().splitlines()[-1])
    assert (d["niter"], d["neval"], d["ngeval"], d["nhvec"]) == ref_counters
    np.testing.assert_allclose(np.array(d["x"]), ref_x, rtol=0, atol=1e-6)
    assert d["fd_products"] == d["nhvec"] and d["fd_evaluations"] == (2 if central else 1) * d["nhvec"]
    # what the problem itself saw: the algorithm's evaluations plus the extra ones, values before gradient at each
    assert d["problem_gevals"] == d["ngeval"] + d["fd_evaluations"]
    assert d["problem_evals"] == d["neval"] + d["fd_evaluations"]
    # ... and with the switch left alone the example ends as every such problem does today
    res = subprocess.run([EXAMPLE, "nvars=%d" % n, "exact_only=1"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode != 0


@pytest.mark.parametrize("central", [False, True])
def test_linear_constraints_allocate_no_constraint_scratch(ctx, central):
    import gc

    import paropt_amd as pa
    from oracle import paropt_oracle as po

    n, c = 500, 4
    rng = np.random.default_rng(3)
    px, z = rng.standard_normal(n), rng.uniform(0.1, 2.0, c)
    prob = pa.SeparableProblem(ctx, "quadratic", n, c)
    ip = _at_an_iterate(ctx, prob)
    ip.setHvecFiniteDifference("always", central=central)
    vpx, vh = pa.PVec(ctx, n).from_numpy(px), pa.PVec(ctx, n)
    sides = 2 if central else 1
    # declared linear: the Jacobian the solver holds is kept, the product is the gradient pair alone
    prob.setLinearConstraints(True)
    gc.collect()
    v0 = pa.live_objects()[0]
    h_lin = ip.evalHvec(z, None, vpx, vh).to_numpy()
    v1 = pa.live_objects()[0]
    ip.evalHvec(z, None, vpx, vh)
    assert pa.live_objects()[0] == v1  # allocated once
    assert v1 - v0 == 1 + sides, v1 - v0  # the perturbed point and one gradient per side: no constraint scratch
    assert ip.getHvecFiniteDifferenceCount() == (2, 2 * sides)
    # the same product with the Jacobian pairs: c more vectors per side; this Jacobian does not depend on x, so its
    # pairs cancel exactly and the product is the same bits
    prob.setLinearConstraints(False)
    h_full = ip.evalHvec(z, None, vpx, vh).to_numpy()
    assert pa.live_objects()[0] - v1 == sides * c
    np.testing.assert_array_equal(h_lin, h_full)
    op = po.SepProblem("quadratic", n, c)
    x, h = ip.getOptimizedPoint()[0].to_numpy(), ip.getHvecFiniteDifferenceStep()
    assert np.all(np.abs(h_lin - fd_hvec(op, x, z, px, None, central, h)) <= cancellation_bound(op, x, z, None, h))


# ---- 6. two ranks on one GPU ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, kind, n, c, extra, central):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import paropt_amd as pa

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    prob = pa.SeparableProblem(ctx, kind, n, c)
    ip = pa.InteriorPoint(prob, dict(NK, write_output_frequency=0, **extra))
    ip.setHvecFiniteDifference("always", central=central)
    ip.optimize()
    h_run = ip.getHvecFiniteDifferenceStep()  # of the last product of the run
    counters = ip.getIterationCounters() + (ip.getHvecCount(),)
    fd = ip.getHvecFiniteDifferenceCount()
    x = ip.getOptimizedPoint()[0].to_numpy()
    vpx = pa.PVec(ctx, prob.nvars).fill_hash(0, 21, prob.offset, 2.0, -1.0)
    hv = ip.evalHvec(np.linspace(0.5, 1.5, c), None, vpx, pa.PVec(ctx, prob.nvars)).to_numpy()
    h_one = ip.getHvecFiniteDifferenceStep()
    got = [None] * world
    dist.all_gather_object(got, (prob.offset, x, hv, h_run, h_one, counters, fd))
    if rank == 0:
        q.put(sorted(got, key=lambda t: t[0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("central", [False, True])
def test_two_ranks_one_gpu(ctx, central):
    import torch.multiprocessing as mp

    import paropt_amd as pa

    kind, n, c, extra = STABLE[1]
    ip, counters, x1 = device_run(ctx, pa.SeparableProblem(ctx, kind, n, c), extra, "always", central)
    vpx = pa.PVec(ctx, n).fill_hash(0, 21, 0, 2.0, -1.0)
    hv1 = ip.evalHvec(np.linspace(0.5, 1.5, c), None, vpx, pa.PVec(ctx, n)).to_numpy()
    h1 = ip.getHvecFiniteDifferenceStep()
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    port = _free_port()
    procs = [mpctx.Process(target=_worker, args=(r, 2, port, q, kind, n, c, extra, central)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, xa, hva, hra, hoa, ca, fa), (_, xb, hvb, hrb, hob, cb, fb) = got
    print("two ranks central=%s: h of the run %r / %r, h of one product %r / %r (one rank: %r), counters %s / %s" % (
        central, hra, hrb, hoa, hob, h1, ca, counters))
    assert hra == hrb and hoa == hob and hra > 0.0 and hoa > 0.0  # the same bits on both ranks
    assert ca == cb == counters and fa == fb == (counters[3], (2 if central else 1) * counters[3])
    assert abs(hoa - h1) <= 1e-9 * h1
    np.testing.assert_allclose(np.concatenate([xa, xb]), x1, rtol=0, atol=1e-7)
    # one product at (nearly) the same point with the same direction: the sharded product is the one-rank product
    scale = max(1.0, np.abs(hv1).max())
    np.testing.assert_allclose(np.concatenate([hva, hvb]), hv1, rtol=0, atol=1e-6 * scale)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_and_zero_direction(ctx):
    import paropt_amd as pa

    n, c = 300, 2
    prob = pa.SeparableProblem(ctx, "convex", n, c)
    sub = pa.QuadraticSubproblem(prob, pa.LBFGS(ctx, n, 5))
    ip_sub = pa.InteriorPoint(sub, {"write_output_frequency": 0})
    for mode in ("when_missing", "always"):
        with pytest.raises(pa.ParOptAMDError) as e:
            ip_sub.setHvecFiniteDifference(mode)
        assert e.value.code == 2  # PO_ERR_ARG
        assert "subproblem" in str(e.value)
    ip_sub.setHvecFiniteDifference("exact")  # the default is always accepted
    ip = _at_an_iterate(ctx, pa.SeparableProblem(ctx, "convex", n, c))
    with pytest.raises(pa.ParOptAMDError) as e:
        ip.setHvecFiniteDifference(7)
    assert e.value.code == 2
    ip.setHvecFiniteDifference("always")
    z = np.ones(c)
    vh = pa.PVec(ctx, n)
    vh.set(3.0)
    zero = pa.PVec(ctx, n)
    zero.zeroEntries()
    np.testing.assert_array_equal(ip.evalHvec(z, None, zero, vh).to_numpy(), np.zeros(n))
    assert ip.getHvecFiniteDifferenceCount() == (1, 0)  # a product, and no callback
    assert ip.getHvecFiniteDifferenceStep() == 0.0
    with pytest.raises(pa.ParOptAMDError) as e:
        ip.evalHvec(z, None, vh, vh)  # px and hvec must be two vectors
    assert e.value.code == 2


# ---- 8. the default costs nothing ----------------------------------------------------------------------------------------
def test_default_mode_adds_no_launch_and_no_allocation(ctx):
    """An existing configuration (the smoke run: quadratic n = 5000, c = 4, L-BFGS(5), 12 iterations) and the
    Newton-Krylov run of the built-in rosenbrock with its exact product: host synchronisations, kernel launches and
    live vectors are the same whether the switch was never touched, set to its default, or set to a differenced mode
    that never has to act (no use_hvec_product; a problem whose own product works)."""
    import gc

    import paropt_amd as pa

    def measure(make, opts, mode):
        ip = pa.InteriorPoint(make(), dict(opts, write_output_frequency=0))
        if mode is not None:
            ip.setHvecFiniteDifference(mode)
        gc.collect()
        r0, l0 = ctx.counters()
        v0 = pa.live_objects()
        ip.optimize()
        r1, l1 = ctx.counters()
        v1 = pa.live_objects()
        return (r1 - r0, l1 - l0, v1[0] - v0[0], v1[1] - v0[1]), ip.getIterationCounters(), \
            ip.getHvecFiniteDifferenceCount()

    smoke_opts = {"qn_subspace_size": 5, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01, "max_major_iters": 12}
    base = measure(lambda: pa.SeparableProblem(ctx, "quadratic", 5000, 4), smoke_opts, None)
    for mode in ("exact", "when_missing", "always"):
        got = measure(lambda: pa.SeparableProblem(ctx, "quadratic", 5000, 4), smoke_opts, mode)
        assert got == base, (mode, got, base)
    assert base[2] == (0, 0)
    nk_base = measure(lambda: pa.SeparableProblem(ctx, "rosenbrock", 100), NK, None)
    for mode in ("exact", "when_missing"):
        got = measure(lambda: pa.SeparableProblem(ctx, "rosenbrock", 100), NK, mode)
        assert got == nk_base, (mode, got, nk_base)
    assert nk_base[2] == (0, 0)
