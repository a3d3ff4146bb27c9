"""
paropt_amd.TorchProblem: Python problems whose callbacks work on zero-copy torch views of the library's vectors.

The metric's workload written with torch ops (examples/random_convex_torch.py) must drive the solver exactly like the
built-in twin and the C++ facade twin -- integer bookkeeping bit-exact, state to round-off -- without a host mirror and,
with deferred device results, with no more host synchronisations than the C++ twin.  The other callback forms
(weighting constraints, CSR, Hessian callbacks, the trust-region driver) are checked against the same problem as a
numpy Problem; those torch problems do their arithmetic in numpy on copies of the views, so that only the plumbing
differs between the two forms.
"""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "examples", "librandom_convex_user.so")
sys.path.insert(0, os.path.join(ROOT, "examples"))


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def tokens(text):
    out = {}
    for ln in str(text).splitlines():
        parts = ln.split()
        if len(parts) >= 15 and parts[0].isdigit():
            out[int(parts[0])] = parts[15:]
    return out


def run(ctx, prob, qn, iters, **extra):
    import paropt_amd as pa

    opts = {"qn_type": qn, "qn_subspace_size": 10, "abs_res_tol": 1e-8, "start_affine_multiplier_min": 0.01,
            "max_major_iters": iters, "write_output_frequency": 0}
    opts.update(extra)
    ip = pa.InteriorPoint(prob, opts)
    snaps = []
    ip.setIterationCallback(lambda k: snaps.append(ip.snapshot()))
    gc.collect()  # (mirrors of earlier runs' objects must not be released inside this one)
    red0, lau0 = ctx.counters()
    mir0 = pa.live_host_mirrors()
    ip.optimize()
    red1, lau1 = ctx.counters()
    mir1 = pa.live_host_mirrors()
    x, z, zl, zu = ip.getOptimizedPoint()
    # host synchronisations: the library's, plus those the problem makes itself (the torch twin's host results)
    syncs = red1 - red0 + getattr(prob, "host_syncs", 0)
    return dict(ip=ip, snaps=snaps, x=x.to_numpy(), z=np.array(z), counters=ip.getIterationCounters(),
                hist=ip.getHistory(), syncs=syncs, launches=lau1 - lau0, mirrors=mir1 - mir0)


# ---- 1. the metric's workload: torch twin against the built-in and the C++ facade twin -------------------------------
@pytest.mark.parametrize("qn,n,c,iters", [("bfgs", 20011, 5, 40), ("bfgs", 100000, 32, 30), ("sr1", 100000, 32, 12)])
def test_torch_twin_matches_the_builtin(ctx, qn, n, c, iters):
    import paropt_amd as pa
    from random_convex_torch import RandomConvexTorch

    a = run(ctx, pa.SeparableProblem(ctx, "convex", n, c), qn, iters)
    b = run(ctx, RandomConvexTorch(ctx, n, c), qn, iters)
    assert a["counters"] == b["counters"]
    assert tokens(a["hist"]) == tokens(b["hist"])
    for sa, sb in zip(a["snaps"], b["snaps"]):
        np.testing.assert_array_equal(sa["counters"], sb["counters"])
        assert sa.get("qn_size", 0) == sb.get("qn_size", 0)
        for key in ("gpiv", "mfpiv", "clamped"):
            if key in sa:
                np.testing.assert_array_equal(np.asarray(sa[key]), np.asarray(sb[key]), err_msg=key)
        assert abs(sa["mu"] - sb["mu"]) <= 1e-9 * abs(sa["mu"])
        # 1e-9, not the C++ twin's 1e-10: besides the objective, torch.mv sums the constraint products in an order
        # of its own (the C++ twin takes them from the library's mdot, as the built-in does)
        assert abs(sa["fobj"] - sb["fobj"]) <= 1e-9 * max(1.0, abs(sa["fobj"]))
    np.testing.assert_allclose(b["x"], a["x"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(b["z"], a["z"], rtol=1e-6, atol=1e-6 * max(1.0, np.abs(a["z"]).max()))
    assert b["mirrors"] == 0
    # deferred device results: the same bits, fewer host synchronisations, no more than the C++ twin's
    d = run(ctx, RandomConvexTorch(ctx, n, c, device_results=True).setDeferredReductions(True), qn, iters)
    assert d["counters"] == b["counters"]
    np.testing.assert_array_equal(d["x"], b["x"])
    np.testing.assert_array_equal(d["z"], b["z"])
    assert d["syncs"] < b["syncs"], (d["syncs"], b["syncs"])
    assert d["mirrors"] == 0
    user = pa.UserLibraryProblem(ctx, USER_LIB, n, c).setDeferredReductions(True)
    u = run(ctx, user, qn, iters)
    assert u["counters"] == d["counters"]
    assert d["syncs"] / d["counters"][0] <= u["syncs"] / u["counters"][0], (d["syncs"], u["syncs"])
    user.close()


def test_device_results_without_deferral(ctx):
    """Device tensors as results with immediate reductions: the same bits as the host results."""
    from random_convex_torch import RandomConvexTorch

    n, c = 20011, 5
    b = run(ctx, RandomConvexTorch(ctx, n, c), "bfgs", 20)
    e = run(ctx, RandomConvexTorch(ctx, n, c, device_results=True), "bfgs", 20)
    assert e["counters"] == b["counters"]
    np.testing.assert_array_equal(e["x"], b["x"])
    np.testing.assert_array_equal(e["z"], b["z"])


# ---- 2. views: no host traffic, one memory, one stream -------------------------------------------------------------
def test_views_alias_hbm_and_share_the_stream(ctx):
    import torch

    import paropt_amd as pa

    n = 100003
    v = pa.PVec(ctx, n).fill_hash(0, 5, 0, 2.0, -1.0)
    w = pa.PVec(ctx, n).fill_hash(0, 6, 0, 2.0, -1.0)
    mir0 = pa.live_host_mirrors()
    t, u = v.as_tensor(), w.as_tensor()
    assert t.data_ptr() == v.device_ptr() and u.data_ptr() == w.device_ptr()
    assert t.dtype == torch.float64 and t.shape == (n,) and t.device == torch.device("cuda", ctx.device())
    assert ctx.torch_stream() is ctx.torch_stream()
    with torch.cuda.stream(ctx.torch_stream()):
        t.mul_(3.0).add_(0.5)  # a torch write ...
        expect = torch.dot(t, u)
    assert v.dot(w) == pytest.approx(float(expect), rel=1e-13)  # ... seen by the library, no synchronisation between
    v.set(0.25)  # a library write ...
    w.scale(-2.0)
    with torch.cuda.stream(ctx.torch_stream()):
        s_v, s_u = float(t.sum()), float(u.sum())  # ... seen through the views
    assert s_v == 0.25 * n
    assert pa.live_host_mirrors() == mir0  # the views made no host mirror
    np.testing.assert_allclose(s_u, w.to_numpy().sum(), rtol=1e-12)


def test_view_of_a_live_mirror_sees_the_host_edits(ctx):
    import torch

    import paropt_amd as pa

    v = pa.PVec(ctx, 1000)
    a = v.getArray()
    a[:] = np.arange(1000.0)  # live mirror: not yet on the device
    t = v.as_tensor()  # uploads and ends the live state
    with torch.cuda.stream(ctx.torch_stream()):
        np.testing.assert_array_equal(t.cpu().numpy(), np.arange(1000.0))
        t.fill_(7.0)
    assert v.l1norm() == 7000.0  # the device copy is authoritative: the old mirror is not uploaded over it


# ---- 3. lifetime -----------------------------------------------------------------------------------------------------
def test_view_keeps_the_vector_alive(ctx):
    import torch

    import paropt_amd as pa

    gc.collect()
    base = pa.live_objects()
    v = pa.PVec(ctx, 4096)
    v.set(1.5)
    t = v.as_tensor()
    t2 = v.as_tensor()
    del v
    gc.collect()
    assert pa.live_objects()[0] == base[0] + 1  # the wrapper is gone, the vector is not
    with torch.cuda.stream(ctx.torch_stream()):
        assert float(t.sum()) == 1.5 * 4096
    del t
    gc.collect()
    assert pa.live_objects()[0] == base[0] + 1
    del t2
    gc.collect()
    assert pa.live_objects() == base


def test_releasing_a_view_after_close_is_harmless():
    script = (
        "import gc, sys\n"
        "sys.path.insert(0, %r)\n"
        "import torch\n"
        "import paropt_amd as pa\n"
        "ctx = pa.Context(0)\n"
        "v = pa.PVec(ctx, 1000)\n"
        "v.set(2.0)\n"
        "t = v.as_tensor()\n"
        "with torch.cuda.stream(ctx.torch_stream()):\n"
        "    s = float(t.sum())\n"
        "ctx.close()\n"
        "del v\n"
        "gc.collect()\n"
        "del t\n"
        "gc.collect()\n"
        "print('released', s)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "released 2000.0" in r.stdout


# ---- 4. the other callback forms against the numpy Problem ------------------------------------------------------------
def _io(torchy):
    """(read, write) of a callback argument: numpy arithmetic on both forms, so only the plumbing differs."""
    if not torchy:
        return (lambda a: np.array(a, dtype=np.float64)), (lambda dst, val: dst.__setitem__(slice(None), val))
    import torch

    def put(dst, val):
        dst.copy_(torch.from_numpy(np.array(np.broadcast_to(val, dst.shape), dtype=np.float64)))

    return (lambda t: t.cpu().numpy()), put


def _weighting(ctx, base, data, Aw, B):
    get, put = _io(base.__name__ == "TorchProblem")
    n, nc, w = data.nlocal, data.c, data.nwcon

    class Weighting(base):
        def getVarsAndBounds(self, x, lb, ub):
            x0, l0, u0 = data.vars_and_bounds()
            put(x, x0), put(lb, l0), put(ub, u0)

        def evalObjCon(self, x):
            return data.eval_obj_con(get(x))

        def evalObjConGradient(self, x, g, A):
            fail, gg, AA = data.eval_obj_con_gradient(get(x))
            put(g, gg)
            for j in range(nc):
                put(A[j], AA[j])
            return fail

        def evalSparseCon(self, x, con):
            put(con, 1.0 + Aw @ get(x))

        def addSparseJacobian(self, alpha, x, px, con):
            put(con, get(con) + alpha * (Aw @ get(px)))

        def addSparseJacobianTranspose(self, alpha, x, pz, out):
            put(out, get(out) + alpha * (Aw.T @ get(pz)))

        def addSparseInnerProduct(self, alpha, x, c, A):
            S = (Aw * get(c)) @ Aw.T
            Ah = get(A).copy()
            incr = B * (B + 1) // 2
            for b in range(w // B):
                for j in range(B):
                    for i in range(j + 1):
                        Ah[b * incr + i + j * (j + 1) // 2] += alpha * S[b * B + i, b * B + j]
            put(A, Ah)

    return Weighting(ctx, n, nc, nc, nwcon=w, nwblock=B)


@pytest.mark.parametrize("B", [1, 4])
def test_weighting_constraints_match_the_numpy_problem(ctx, B):
    import paropt_amd as pa
    from oracle import paropt_oracle as po  # problem data only

    n, w, nw = 240, 60, 4
    data = po.SepProblem("convex", n, 3, nwcon=w, nw=nw, nwblock=B)
    Aw = data.sparse_jacobian_dense()
    a = run(ctx, _weighting(ctx, pa.Problem, data, Aw, B), "bfgs", 30)
    b = run(ctx, _weighting(ctx, pa.TorchProblem, data, Aw, B), "bfgs", 30)
    assert a["mirrors"] > 0 and b["mirrors"] == 0
    assert a["counters"] == b["counters"]
    assert tokens(a["hist"]) == tokens(b["hist"])
    np.testing.assert_allclose(b["x"], a["x"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b["z"], a["z"], rtol=1e-12, atol=1e-12)
    assert ("MatInfo: nblock: %d" % B) in b["hist"] or B == 1


IPW_VIA_CSR = ["ipw_convex_n400_c4_w80", "ipw_convex_n300_c2_w30_eq", "ipw_rosenbrock_n100_w5",
               "ipw_convex_n240_c3_w40_l2", "ipw_convex_n240_c3_w40_mehrotra"]


@pytest.mark.parametrize("name", IPW_VIA_CSR)
def test_csr_form_follows_the_reference_goldens(ctx, name):
    """The Jacobian values are written into the view of the library's device array (no host buffer, no copy)."""
    import paropt_amd as pa
    from conftest import ip_options_from_case, load_golden, tolerance_schedule
    from oracle import paropt_oracle as po

    g, case = load_golden(name)
    a = case["args"]
    nwineq = a.get("nwineq", a["nwcon"])
    oprob = po.SepProblem(a["problem"], a["n"], a.get("c", 2), nwcon=a["nwcon"], nw=a["nw"],
                          nwstart=a.get("nwstart", 0), nwskip=a.get("nwskip", 0), nwineq=nwineq)
    nwcon, nw = oprob.nwcon, oprob.nw
    rowp = np.arange(nwcon + 1, dtype=np.intc) * nw
    cols = (oprob.nwstart + (np.arange(nwcon)[:, None] * (nw + oprob.nwskip)) + np.arange(nw)[None, :]).astype(
        np.intc).ravel()
    get, put = _io(True)
    seen = {}

    class P(pa.TorchProblem):
        def getVarsAndBounds(self, x, lb, ub):
            x0, l0, u0 = oprob.vars_and_bounds()
            put(x, x0), put(lb, l0), put(ub, u0)

        def evalSparseObjCon(self, x, sparse):
            fail, f, con = oprob.eval_obj_con(get(x))
            put(sparse, oprob.eval_sparse_con(get(x)))
            return fail, f, con

        def evalSparseObjConGradient(self, x, g, A, data):
            _, gg, aa = oprob.eval_obj_con_gradient(get(x))
            put(g, gg)
            for j in range(oprob.c):
                put(A[j], aa[j])
            seen["data"] = (data.data_ptr(), data.device.type, tuple(data.shape))
            data[:] = -1.0
            return 0

    prob = P(ctx, oprob.nlocal, oprob.c, oprob.c, nwcon=nwcon, nwinequality=nwineq, rowp=rowp, cols=cols)
    opts = ip_options_from_case(case)
    opts["write_output_frequency"] = 0
    ip = pa.InteriorPoint(prob, opts)
    snaps = []
    ip.setIterationCallback(lambda k: snaps.append(ip.snapshot()))
    gc.collect()
    mir0 = pa.live_host_mirrors()
    ip.optimize()
    assert pa.live_host_mirrors() == mir0
    import ctypes as C
    from paropt_amd import lib as L

    rp, cl, dp, nnz = L.c_int_p(), L.c_int_p(), C.c_void_p(), C.c_int64()
    L.check(L.lib.po_problem_get_sparse_jacobian_data(prob.handle, C.byref(rp), C.byref(cl), C.byref(dp),
                                                      C.byref(nnz)))
    assert seen["data"] == (dp.value, "cuda", (nnz.value,))
    nref = 1 + max(int(k[2:5]) for k in g if k.startswith("it") and k.endswith("/mu"))
    ncmp = min(nref, len(snaps))
    assert ncmp >= nref - 1
    tol = tolerance_schedule(name)
    for k in range(ncmp):
        p = "it%03d/" % k
        s = snaps[k]
        np.testing.assert_array_equal(s["counters"], g[p + "counters"], err_msg="counters @%d" % k)
        assert abs(s["mu"] - g[p + "mu"][0]) / abs(g[p + "mu"][0]) <= tol("mu", k), k
        assert abs(s["fobj"] - g[p + "fobj"][0]) / max(1.0, abs(g[p + "fobj"][0])) <= tol("fobj", k), k
        for key in ("z", "s", "t", "zs", "zt"):
            ref = g[p + key]
            if ref.size:
                assert np.abs(s[key] - ref).max() / max(1.0, np.abs(ref).max()) <= tol("dense", k), (key, k)
        wa, wb = np.asarray(s["wnorms"]), np.asarray(g[p + "wnorms"])
        nz = wb != 0
        assert (np.abs(wa[nz] - wb[nz]) / np.abs(wb[nz])).max() <= tol("wnorms", k), k


def _rosen(ctx, base, op, n):
    get, put = _io(base.__name__ == "TorchProblem")

    class Rosen(base):
        def getVarsAndBounds(self, x, lb, ub):
            put(x, -1.0), put(lb, -2.0), put(ub, 1.0)

        def evalObjCon(self, x):
            return op.eval_obj_con(get(x))

        def evalObjConGradient(self, x, g, A):
            _, gg, aa = op.eval_obj_con_gradient(get(x))
            put(g, gg)
            put(A[0], aa[0]), put(A[1], aa[1])
            return 0

        def evalHvecProduct(self, x, z, zw, px, hvec):
            assert isinstance(z, np.ndarray) and len(z) == 2  # z stays on the host
            put(hvec, op.hvec_product(get(x), z, get(px)))
            return 0

        def evalHessianDiag(self, x, z, zw, hdiag):
            put(hdiag, op.hessian_diag(get(x), z))
            return 0

    return Rosen(ctx, n, 2)


def test_hessian_callbacks_match_the_numpy_problem(ctx):
    import paropt_amd as pa
    from conftest import ip_options_from_case, load_golden
    from oracle import paropt_oracle as po

    n = 100
    op = po.SepProblem("rosenbrock", n, 2)
    for name in ("ip_rosenbrock_hvec_n100", "ip_rosenbrock_diaghess_n100"):
        g, case = load_golden(name)
        opts = ip_options_from_case(case)
        opts["write_output_frequency"] = 0
        ip1 = pa.InteriorPoint(_rosen(ctx, pa.Problem, op, n), opts)
        ip1.optimize()
        ip2 = pa.InteriorPoint(_rosen(ctx, pa.TorchProblem, op, n), opts)
        ip2.optimize()
        assert ip2.getIterationCounters() == ip1.getIterationCounters()
        assert ip2.getHvecCount() == ip1.getHvecCount()
        np.testing.assert_array_equal(np.array(ip2.getIterationCounters()), g["final/counters"])
        np.testing.assert_allclose(ip2.getOptimizedPoint()[0].to_numpy(), ip1.getOptimizedPoint()[0].to_numpy(),
                                   rtol=0, atol=1e-12)
        if "hvec" in name:
            assert "iNK" in ip2.getHistory()


def test_trust_region_optimizer_matches_the_numpy_problem(tmp_path):
    from oracle import paropt_oracle as po
    from paropt_amd import ParOpt

    n = 60
    op = po.SepProblem("rosenbrock", n, 2)

    def make(base):
        get, put = _io(base is ParOpt.TorchProblem)

        class Rosen(base):
            def __init__(self):
                super().__init__(None, nvars=n, ncon=2)

            def getVarsAndBounds(self, x, lb, ub):
                put(x, -1.0), put(lb, -2.0), put(ub, 1.0)

            def evalObjCon(self, x):
                return op.eval_obj_con(get(x))

            def evalObjConGradient(self, x, g, A):
                _, gg, aa = op.eval_obj_con_gradient(get(x))
                put(g, gg)
                put(A[0], aa[0]), put(A[1], aa[1])
                return 0

        return Rosen()

    res = []
    for base in (ParOpt.Problem, ParOpt.TorchProblem):
        trfile = str(tmp_path / ("%s.tr" % base.__name__))
        opt = ParOpt.Optimizer(make(base), {"algorithm": "tr", "tr_init_size": 0.05, "tr_min_size": 1e-6,
                                            "tr_max_size": 10.0, "tr_eta": 0.25, "tr_adaptive_gamma_update": True,
                                            "tr_max_iterations": 40, "qn_subspace_size": 10, "output_file": None,
                                            "tr_output_file": trfile})
        opt.optimize()
        res.append((np.array(opt.getOptimizedPoint()[0][:]), ParOpt.unpack_tr_output(trfile)[1]))
    (xa, ca), (xb, cb) = res
    assert len(ca[0]) > 5
    np.testing.assert_array_equal(cb[0], ca[0])  # the integer column
    for k in range(1, len(ca) - 1):  # values to round-off (the last column is wall time)
        np.testing.assert_allclose(cb[k], ca[k], rtol=1e-9, atol=1e-14, err_msg="column %d" % k)
    np.testing.assert_allclose(xb, xa, rtol=0, atol=1e-12)


def test_callback_exception_is_reraised(ctx):
    import paropt_amd as pa

    class Boom(pa.TorchProblem):
        def getVarsAndBounds(self, x, lb, ub):
            x.fill_(0.5), lb.fill_(0.0), ub.fill_(1.0)

        def evalObjCon(self, x):
            raise RuntimeError("boom in evalObjCon")

        def evalObjConGradient(self, x, g, A):
            g.zero_()
            return 0

    ip = pa.InteriorPoint(Boom(ctx, 100, 0), {"max_major_iters": 5, "write_output_frequency": 0})
    with pytest.raises(RuntimeError, match="boom in evalObjCon"):
        ip.optimize()


def test_tensor_results_of_the_wrong_kind_are_refused(ctx):
    import torch

    import paropt_amd as pa

    class Bad(pa.TorchProblem):
        def getVarsAndBounds(self, x, lb, ub):
            x.fill_(0.5), lb.fill_(0.0), ub.fill_(1.0)

        def evalObjCon(self, x):
            return 0, x.sum().float(), torch.zeros(1, dtype=torch.float64, device=x.device)

        def evalObjConGradient(self, x, g, A):
            g.zero_()
            A[0].zero_()
            return 0

    ip = pa.InteriorPoint(Bad(ctx, 100, 1), {"max_major_iters": 5, "write_output_frequency": 0})
    with pytest.raises(TypeError, match="float64"):
        ip.optimize()


# ---- 5. two ranks on one GPU ------------------------------------------------------------------------------------------
def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, n, c, iters):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import paropt_amd as pa
    from random_convex_torch import RandomConvexTorch

    ctx = pa.Context(0)
    ctx.init_callback_from_torch()
    assert ctx.rank_size() == (rank, world)
    prob = RandomConvexTorch(ctx, n, c, device_results=True).setDeferredReductions(True)
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": 10, "abs_res_tol": 1e-8,
                                 "start_affine_multiplier_min": 0.01, "max_major_iters": iters,
                                 "write_output_frequency": 0})
    ip.optimize()
    x = ip.getOptimizedPoint()[0].to_numpy()
    xs = [None] * world
    dist.all_gather_object(xs, (prob.offset, x))
    if rank == 0:
        q.put((ip.getIterationCounters(), ip.getObjective()[0],
               np.concatenate([a for _, a in sorted(xs, key=lambda t: t[0])])))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_match_single_rank(ctx):
    import torch.multiprocessing as mp

    from random_convex_torch import RandomConvexTorch

    n, c, iters = 40003, 6, 25
    one = run(ctx, RandomConvexTorch(ctx, n, c, device_results=True).setDeferredReductions(True), "bfgs", iters)
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    port = _free_port()
    procs = [mpctx.Process(target=_worker, args=(r, 2, port, q, n, c, iters)) for r in range(2)]
    for p in procs:
        p.start()
    counters, fobj, x2 = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert counters == one["counters"]
    assert abs(fobj - one["ip"].getObjective()[0]) <= 1e-7 * max(1.0, abs(fobj))
    np.testing.assert_allclose(x2, one["x"], rtol=0, atol=1e-7)
