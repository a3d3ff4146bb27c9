"""GPU: a compact quasi-Newton approximation the USER wrote (paropt_amd.CompactQuasiNewton, po_qn_create_callbacks).

  * the reference's quasi-Newton sequences (tests/golden/qn_*.npz) with a user-side restatement behind the callback
    table, under the very assertions of test_gpu_qn.py::test_quasi_newton_golden (that function is called with the
    class names it builds replaced -- nothing is restated);
  * the reference's interior-point trajectories with a user approximation attached through setQuasiNewton, under the
    very assertions of test_gpu_ip.py::test_ip_trajectory_golden, for every golden whose options give the solver an
    approximation;
  * the trust-region object assemblies of test_gpu_tr.py with the user class in place of LBFGS / LSR1;
  * call accounting, the consistency checker, the scaled wrapper, misuse, leaks.
"""
import gc

import numpy as np
import pytest

import test_gpu_ip as TI
import test_gpu_qn as TQ
import test_gpu_tr as TT
from conftest import golden_names, ip_options_from_case, load_golden
from user_qn_helpers import OracleQN, PVecLBFGS, PVecLSR1, make_user_qn

pytestmark = pytest.mark.gpu

FLAVOURS = ("oracle", "pvec")


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def replacing_builtins(monkeypatch, flavour, as_driver):
    """paropt_amd.LBFGS / LSR1 build the user class instead (as_driver: seen through the C ABI, the way the library
    sees it); returns the list of user objects made."""
    import paropt_amd as pa

    made = []

    def factory(kind):
        def make(ctx, n, subspace=10, update_type="skip_negative_curvature"):
            q = make_user_qn(flavour, ctx, n, kind, subspace, update_type)
            made.append(q)
            return q.driver() if as_driver else q
        return make

    monkeypatch.setattr(pa, "LBFGS", factory("bfgs"))
    monkeypatch.setattr(pa, "LSR1", factory("sr1"))
    return made


def attaching(monkeypatch, flavour):
    """paropt_amd.InteriorPoint calls setQuasiNewton(user_qn) right after construction, the user class built from the
    case's qn_type, qn_subspace_size, qn_update_type and qn_diag_type."""
    import paropt_amd as pa

    made = []

    class Attaching(pa.InteriorPoint):
        def __init__(self, problem, options=None):
            super().__init__(problem, options)
            o = dict(options or {})
            kind = o.get("qn_type", "bfgs")
            if kind in ("bfgs", "sr1"):
                q = make_user_qn(flavour, problem.ctx, problem.nvars, kind, o.get("qn_subspace_size", 10),
                                 o.get("qn_update_type", "skip_negative_curvature"),
                                 o.get("qn_diag_type", "yty_over_yts"))
                made.append(q)
                self.setQuasiNewton(q)

    monkeypatch.setattr(pa, "InteriorPoint", Attaching)
    return made


# ---- 4. the reference's quasi-Newton sequences through the callback table ---------------------------------------------
@pytest.mark.parametrize("flavour,name", [(f, n) for n in golden_names("qn_") for f in FLAVOURS + ("cpp",)
                                          if f != "cpp" or "bfgs" in n])
def test_quasi_newton_golden_through_the_callback_table(ctx, name, flavour, monkeypatch):
    made = replacing_builtins(monkeypatch, flavour, as_driver=True)
    TQ.test_quasi_newton_golden(ctx, name)
    assert made and made[0].calls["update"] > 0 and made[0].calls["mult"] > 0 and made[0].calls["multAdd"] > 0


# ---- 5. the reference's interior-point trajectories with a user approximation -----------------------------------------
def _case_info(name):
    case = load_golden(name)[1]
    o = ip_options_from_case(case)
    return o.get("qn_type", "bfgs"), bool(o.get("sequential_linear_method", 0)), case["args"]["n"]


INFO = {n: _case_info(n) for n in TI.IP_CASES}  # (qn_type, sequential linear, n), each golden read once
QN_CASES = [n for n in TI.IP_CASES if INFO[n][0] in ("bfgs", "sr1")]
SMALL_QN_CASES = [n for n in QN_CASES if INFO[n][2] <= 2000]


def _seq_lin(name):
    return INFO[name][1]


def test_case_list_is_complete():
    assert len(TI.IP_CASES) == 68
    assert len(QN_CASES) == 67 and [n for n in TI.IP_CASES if n not in QN_CASES] == ["ip_quadratic_slp_noqn_n200_c2"]
    assert len(SMALL_QN_CASES) == 62
    assert sum(_seq_lin(n) for n in QN_CASES) == 3


def _trajectory(ctx, name, flavour, monkeypatch):
    made = attaching(monkeypatch, flavour)
    TI.test_ip_trajectory_golden(ctx, name)
    assert made, "no user approximation was attached"
    calls = made[0].calls
    assert calls["getCompactMat"] > 0, "the approximation was silently detached"
    if not _seq_lin(name):
        assert calls["update"] > 0, "the approximation was never updated"


@pytest.mark.parametrize("name", QN_CASES)
def test_ip_goldens_with_user_numpy_approximation(ctx, name, monkeypatch):
    _trajectory(ctx, name, "oracle", monkeypatch)


@pytest.mark.parametrize("name", SMALL_QN_CASES)
def test_ip_goldens_with_user_pvec_approximation(ctx, name, monkeypatch):
    _trajectory(ctx, name, "pvec", monkeypatch)


BFGS_CASES = [n for n in QN_CASES if INFO[n][0] == "bfgs"]


@pytest.mark.parametrize("name", BFGS_CASES)
def test_ip_goldens_with_the_cpp_example_class(ctx, name, monkeypatch):
    """examples/user_quasi_newton_amd.cpp's class (its own HIP kernels) attached through its extern "C" constructor.  It
    is an L-BFGS: the cases whose qn_type is bfgs."""
    _trajectory(ctx, name, "cpp", monkeypatch)


def test_call_accounting_is_the_same_from_cpp_and_python(ctx):
    import paropt_amd as pa

    seen = []
    for flavour in ("pvec", "cpp"):
        prob = pa.SeparableProblem(ctx, "quadratic", 1000, 8)
        ip = pa.InteriorPoint(prob, {"qn_subspace_size": 5, "max_major_iters": 25, "abs_res_tol": 1e-8,
                                     "write_output_frequency": 0, "hessian_reset_freq": 7})
        q = make_user_qn(flavour, ctx, 1000, "bfgs", 5)
        ip.setQuasiNewton(q)
        ip.optimize()
        calls = q.calls
        seen.append((ip.getIterationCounters(), {k: calls[k] for k in ("reset", "update", "getCompactMat", "mult")}))
    print("python:", seen[0], "C++:", seen[1])
    assert seen[0] == seen[1] and seen[0][1]["reset"] > 0 and seen[0][1]["update"] > 0


# ---- 6. trust region and eigenvalue model -----------------------------------------------------------------------------
TR_OBJECT_CASES = ["tr_eig_quadratic_n200_c2_N4", "tr_rand_eig_quadratic_n257_c3_N5_subcon",
                   "tr_quadratic_n200_c3_bfgs", "tr_convex_n200_c2_w40"]


@pytest.mark.parametrize("name", TR_OBJECT_CASES)
def test_tr_objects_with_user_approximation(ctx, name, monkeypatch):
    """The existing test itself, with the user class on the device in place of LBFGS / LSR1.  Its last clause compares
    the rows BIT FOR BIT with the self-assembled driver (which keeps the built-in class): the PVec class meets it,
    because its dots go through the same reduction kernels."""
    made = replacing_builtins(monkeypatch, "pvec", as_driver=False)
    TT.test_tr_objects_assembled_like_the_reference(ctx, name)
    assert made and made[0].calls["update"] > 0 and made[0].calls["getCompactMat"] > 0


@pytest.mark.parametrize("name", TR_OBJECT_CASES)
def test_tr_objects_with_user_numpy_approximation(ctx, name, monkeypatch):
    """The numpy class sums its dots in another order than the device kernels, so the bit-for-bit clause of the existing
    test (against a run with the BUILT-IN class) cannot apply to it: measured differences of the rows are 6e-16 to
    1.4e-11 relative.  Every assertion of that test against the REFERENCE's rows is made here, through the same
    compare_tr, with the same windows and bounds."""
    made = replacing_builtins(monkeypatch, "oracle", as_driver=False)
    g, case = load_golden(name)
    tr, ip, sub, rows, final = TT.run_gpu_tr_objects(ctx, case)
    n = TT.compare_tr(g, rows, [], final, 60, check_snaps=False, inexact_rows=TT.TR_INEXACT_ROWS.get(name, set()))
    assert n >= 12
    assert final["iter_count"] == int(g["final/iter_count"][0])
    assert abs(final["fk"] - g["final/fk"][0]) <= 1e-6 * max(1.0, abs(g["final/fk"][0]))
    np.testing.assert_allclose(final["x"], g["final/x"], rtol=0, atol=1e-5 * max(1.0, np.abs(g["final/x"]).max()))
    np.testing.assert_allclose(final["z"], g["final/z"], rtol=1e-4, atol=1e-6)
    assert made and made[0].calls["update"] > 0 and made[0].calls["getCompactMat"] > 0


def _rows_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        if len(ra) == 2 and isinstance(ra[1], (list, tuple)):  # (printed columns, info tokens) of a trust-region row
            assert list(ra[1]) == list(rb[1]), (ra[1], rb[1])
            ra, rb = ra[0], rb[0]
        np.testing.assert_allclose(np.asarray(ra, dtype=float), np.asarray(rb, dtype=float), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_tr_sr1_under_the_quadratic_model_builtin_against_user(ctx, flavour, monkeypatch):
    _, case = load_golden("tr_rosenbrock_n60_sr1")
    rows0 = TT.run_gpu_tr_objects(ctx, case)[3]
    made = replacing_builtins(monkeypatch, flavour, as_driver=False)
    rows1 = TT.run_gpu_tr_objects(ctx, case)[3]
    assert made and made[0].calls["update"] > 0 and made[0].calls["getCompactMat"] > 0
    assert len(rows0) > 3
    _rows_equal(rows0, rows1)


# ---- 7. call accounting -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["affine_step", "no_start_strategy"])
def test_call_accounting(ctx, start):
    """The library asks for the compact form once at hand-over, once at the start of optimize(), once at the head of
    every KKT set-up and once after every reset / update / multiplier update it issues.  A monotone run takes one KKT
    set-up and one update per major iteration; the affine-step starting point is one more set-up.  So the user sees
    exactly 2 + [affine] + 2 * iterations + resets requests, and never a mult: the compact form is authoritative."""
    import paropt_amd as pa

    n, iters = 500, 9
    prob = pa.SeparableProblem(ctx, "quadratic", n, 3)
    ip = pa.InteriorPoint(prob, {"qn_subspace_size": 4, "max_major_iters": iters, "abs_res_tol": 1e-30,
                                 "write_output_frequency": 0, "hessian_reset_freq": 1000000,
                                 "starting_point_strategy": start})
    q = PVecLBFGS(ctx, n, 4)
    ip.setQuasiNewton(q)
    assert q.calls["getCompactMat"] == 1
    ip.optimize()
    print("calls:", start, dict(q.calls))
    assert q.calls["update"] == iters
    assert q.calls["getCompactMat"] == 2 + (start == "affine_step") + 2 * iters + q.calls["reset"]
    assert q.calls["mult"] == 0 and q.calls["multAdd"] == 0


# ---- 8. layout and the consistency checker ----------------------------------------------------------------------------
class Lopsided:
    """B = b0 I - Z d M^-1 d Z^T with a deliberately NON-symmetric M and non-unit d, in numpy (host mode)"""

    @staticmethod
    def make(ctx, n, transpose):
        import paropt_amd as pa

        rng = np.random.default_rng(5)
        k = 3
        Zn = [rng.standard_normal(n) for _ in range(k)]
        M = 4.0 * np.eye(k) + rng.standard_normal((k, k))
        d = np.array([0.5, 2.0, 1.5])
        b0 = 3.0

        class Q(pa.CompactQuasiNewton):
            def __init__(self):
                super().__init__(ctx, n, host=True)

            def reset(self):
                pass

            def update(self, x, z, zw, s, y):
                return 0

            def _bx(self, x):
                return b0 * x - sum(c * zc for c, zc in zip(d * np.linalg.solve(M, d * np.array([zc @ x for zc in Zn])), Zn))

            def mult(self, x, y):
                y[:] = self._bx(x)

            def multAdd(self, alpha, x, y):
                y += alpha * self._bx(x)

            def getCompactMat(self):
                return b0, d, (M.T if transpose else M), Zn

            def getMaxLimitedMemorySize(self):
                return k

        return Q(), (b0, d, M, Zn)


def test_layout_and_consistency_checker(ctx):
    import paropt_amd as pa

    n = 300
    q, (b0, d, M, Zn) = Lopsided.make(ctx, n, transpose=False)
    drv = q.driver()
    b, dd, MM, ZZ = drv.getCompactMat()
    assert b == b0
    np.testing.assert_array_equal(dd, d)
    np.testing.assert_array_equal(MM, M)  # row i, column j on both sides of the boundary
    for zc, zn in zip(ZZ, Zn):
        np.testing.assert_array_equal(zc.to_numpy(), zn)
    xn = np.random.default_rng(1).standard_normal(n)
    x, y = pa.PVec(ctx, n).from_numpy(xn), pa.PVec(ctx, n)
    drv.mult(x, y)
    np.testing.assert_array_equal(y.to_numpy(), q._bx(xn))  # po_qn_mult of the handle IS the user's mult
    y.from_numpy(xn)
    drv.multAdd(-0.5, x, y)
    np.testing.assert_allclose(y.to_numpy(), xn - 0.5 * q._bx(xn), rtol=1e-14, atol=1e-14)
    assert q.checkCompactForm() <= 1e-8

    qt, _ = Lopsided.make(ctx, n, transpose=True)
    probe = pa.PVec(ctx, n).fill_hash(0, 0, 0, 2.0, -1.0).to_numpy()
    Zm = np.array(Zn).T
    good = qt._bx(probe)
    swapped = b0 * probe - Zm @ (d * np.linalg.solve(M.T, d * (Zm.T @ probe)))
    want = np.abs(good - swapped).max() / np.abs(good).max()
    assert want > 1e-3
    np.testing.assert_allclose(qt.checkCompactForm(), want, rtol=1e-8)


def test_builtin_classes_satisfy_the_checker(ctx):
    import paropt_amd as pa

    n = 400
    s, y = pa.PVec(ctx, n), pa.PVec(ctx, n)
    for qn, tol in ((pa.LBFGS(ctx, n, 4), 1e-8), (pa.LSR1(ctx, n, 4), 5e-6)):
        for k in range(6):
            sn, yn = TQ.qn_pair(k, n)
            qn.update(s.from_numpy(sn), y.from_numpy(yn))
        assert qn.getCompactMat()[3]
        assert qn.checkCompactForm() <= tol
    prob = pa.SeparableProblem(ctx, "quadratic", n, 2)
    N = 3
    approx = pa.CompactEigenApprox(prob, N)
    rng = np.random.default_rng(2)
    for i in range(N):
        approx.hvecs[i].from_numpy(rng.standard_normal(n))
    A = rng.standard_normal((N, N))
    Mm = A @ A.T + N * np.eye(N)
    approx.M[:, :] = Mm
    approx.Minv[:, :] = np.linalg.inv(Mm)
    inner = pa.LBFGS(ctx, n, 4)
    inner.update(s, y)
    eq = pa.EigenQuasiNewton(inner, approx, 0)
    assert eq.checkCompactForm() <= 1e-8


# ---- 9. the scaled wrapper --------------------------------------------------------------------------------------------
def test_scaled_quasi_newton(ctx):
    import paropt_amd as pa

    n, z0 = 300, 2.5
    prob = pa.SeparableProblem(ctx, "quadratic", n, 1)
    inner = pa.LBFGS(ctx, n, 4)
    q = pa.ScaledQuasiNewton(prob, inner)
    s, y, x = pa.PVec(ctx, n), pa.PVec(ctx, n), pa.PVec(ctx, n)
    for k in range(3):
        sn, yn = TQ.qn_pair(k, n)
        assert q.update(None, np.array([z0]), None, s.from_numpy(sn), y.from_numpy(yn)) == 0
    # the inner class holds the pair (s, y / z0)
    Z = inner.getCompactMat()[3]
    np.testing.assert_array_equal(Z[2].to_numpy(), sn)
    # (y * (1 / z0) against y / z0: two roundings against one, at most 1.5 ulp apart)
    np.testing.assert_allclose(Z[5].to_numpy(), yn / z0, rtol=2 * np.finfo(float).eps, atol=0)
    xn = np.random.default_rng(3).standard_normal(n)
    x.from_numpy(xn)
    a, b = pa.PVec(ctx, n), pa.PVec(ctx, n)
    q.driver().mult(x, a)
    inner.mult(x, b)
    ref = z0 * b.to_numpy()
    assert np.abs(a.to_numpy() - ref).max() <= 4 * np.finfo(float).eps * np.abs(ref).max()
    assert q.checkCompactForm() <= 1e-8
    b0, d, M, _ = q.driver().getCompactMat()
    bi, di, Mi, _ = inner.getCompactMat()
    assert b0 == z0 * bi
    np.testing.assert_array_equal(d, np.sqrt(z0) * di)
    np.testing.assert_array_equal(M, Mi)


def test_scaled_quasi_newton_under_the_interior_point(ctx):
    """Not pinned to a reference run (the reference driver builds no scaled wrapper): the wrapper against a hand-written
    class that does the same arithmetic, row for row."""
    import paropt_amd as pa

    n = 400
    opts = {"qn_subspace_size": 4, "max_major_iters": 12, "abs_res_tol": 1e-9, "write_output_frequency": 0}

    class ByHand(PVecLBFGS):
        z0 = 1.0

        def __init__(self, ctx, n, m):
            super().__init__(ctx, n, m)
            self.y0 = pa.PVec(ctx, n)

        def update(self, x, z, zw, s, y):
            if z is not None and z[0] > 0.0:
                self.z0 = float(z[0])
            self.y0.copyValues(y)
            self.y0.scale(1.0 / self.z0)
            return super().update(x, z, zw, s, self.y0)

        def getCompactMat(self):
            b0, d, M, Z = super().getCompactMat()
            return self.z0 * b0, np.sqrt(self.z0) * np.asarray(d), M, Z

    rows = []
    for make in (lambda p: pa.ScaledQuasiNewton(p, PVecLBFGS(ctx, n, 4)), lambda p: ByHand(ctx, n, 4)):
        prob = pa.SeparableProblem(ctx, "quadratic", n, 1)
        ip = pa.InteriorPoint(prob, opts)
        q = make(prob)
        ip.setQuasiNewton(q)
        ip.optimize()
        rows.append([ln.split() for ln in ip.getHistory().splitlines() if ln[:5].strip().isdigit()])
    assert len(rows[0]) > 3 and rows[0] == rows[1]


# ---- 10. misuse -------------------------------------------------------------------------------------------------------
class Fixed:
    """a fixed approximation whose compact form the test dictates"""

    @staticmethod
    def make(ctx, n, compact, kmax=4, fail_in=None):
        import paropt_amd as pa

        class Q(pa.CompactQuasiNewton):
            def _maybe(self, where):
                if fail_in == where:
                    raise KeyError("boom in " + where)

            def reset(self):
                self._maybe("reset")

            def update(self, x, z, zw, s, y):
                self._maybe("update")
                return 0

            def mult(self, x, y):
                self._maybe("mult")
                y.copyValues(x)

            def multAdd(self, alpha, x, y):
                self._maybe("multAdd")
                y.axpy(alpha, x)

            def getCompactMat(self):
                self._maybe("getCompactMat")
                return compact()

            def getMaxLimitedMemorySize(self):
                self._maybe("getMaxLimitedMemorySize")
                return kmax

        return Q(ctx, n)


def _ip(ctx, n, c=2):
    import paropt_amd as pa

    prob = pa.SeparableProblem(ctx, "quadratic", n, c)
    return pa.InteriorPoint(prob, {"qn_subspace_size": 3, "max_major_iters": 5, "write_output_frequency": 0,
                                   "hessian_reset_freq": 2})


def test_misuse_is_a_clean_error(ctx):
    import paropt_amd as pa

    n = 200
    ident = lambda: (1.0, np.zeros(0), np.zeros((0, 0)), [])  # noqa: E731
    # a column of the wrong size
    short = pa.PVec(ctx, n - 1)
    with pytest.raises(pa.ParOptAMDError, match="column 0 of Z has the wrong size"):
        _ip(ctx, n).setQuasiNewton(Fixed.make(ctx, n, lambda: (1.0, [1.0], [[1.0]], [short])))
    # ... or from another context
    other = pa.Context(0)
    try:
        foreign = pa.PVec(other, n)
        with pytest.raises(pa.ParOptAMDError, match="column 0 of Z belongs to another context"):
            _ip(ctx, n).setQuasiNewton(Fixed.make(ctx, n, lambda: (1.0, [1.0], [[1.0]], [foreign])))
        del foreign
    finally:
        other.close()
    # more columns than getMaxLimitedMemorySize
    cols = [pa.PVec(ctx, n) for _ in range(3)]
    with pytest.raises(pa.ParOptAMDError, match="outside 0..2"):
        _ip(ctx, n).setQuasiNewton(Fixed.make(ctx, n, lambda: (1.0, np.ones(3), np.eye(3), cols), kmax=2))
    # a Python exception in each callback the solver reaches is re-raised by optimize() (or by the hand-over)
    for where in ("getCompactMat", "getMaxLimitedMemorySize"):
        with pytest.raises(KeyError, match=where):
            _ip(ctx, n).setQuasiNewton(Fixed.make(ctx, n, ident, fail_in=where))
    for where in ("update", "reset"):
        ip = _ip(ctx, n)
        ip.setQuasiNewton(Fixed.make(ctx, n, ident, fail_in=where))
        with pytest.raises(KeyError, match=where):
            ip.optimize()
    for where in ("mult", "multAdd"):
        q = Fixed.make(ctx, n, ident, fail_in=where)
        x, y = pa.PVec(ctx, n), pa.PVec(ctx, n)
        with pytest.raises(KeyError, match=where):
            getattr(q.driver(), where)(*([x, y] if where == "mult" else [1.0, x, y]))
    # the process lives and the context still works
    ip = _ip(ctx, n)
    ip.setQuasiNewton(PVecLBFGS(ctx, n, 3))
    ip.optimize()
    # no pair storage to load
    with pytest.raises(pa.ParOptAMDError):
        Fixed.make(ctx, n, ident).debugLoad()


def test_callback_returning_nonzero_through_the_c_abi(ctx):
    """A table written in C terms (ctypes): update returns 1 -> optimize() ends with PO_ERR_USER and a message."""
    import ctypes as C

    import paropt_amd as pa
    import paropt_amd.lib as L

    n = 100

    def compact(user, size, b0, d, M, Z):
        size[0], b0[0] = 0, 1.0
        return 0

    def max_size(user, size):
        size[0] = 2
        return 0

    fns = (L.QN_VOID_FN(lambda u: 0), L.QN_UPDATE_FN(lambda u, x, z, zw, s, y, rc: 1), L.QN_UPDMULT_FN(),
           L.QN_MULT_FN(lambda u, x, y: 0), L.QN_MULTADD_FN(lambda u, a, x, y: 0), L.QN_COMPACT_FN(compact),
           L.QN_SIZE_FN(max_size), L.QN_DIAG_FN())
    cb = L.QnCallbacks()
    cb.user = None
    (cb.reset, cb.update, cb.update_multipliers, cb.mult, cb.mult_add, cb.get_compact_mat, cb.get_max_size,
     cb.set_init_diagonal_type) = fns
    h = L.po_qn()
    L.check(L.lib.po_qn_create_callbacks(ctx.handle, n, C.byref(cb), C.byref(h)))
    try:
        ip = _ip(ctx, n)
        L.check(L.lib.po_ip_set_quasi_newton(ip._h, h))
        with pytest.raises(pa.ParOptAMDError, match="update failed") as e:
            ip.optimize()
        assert e.value.code == 6  # PO_ERR_USER
        L.check(L.lib.po_ip_set_quasi_newton(ip._h, None))
    finally:
        L.lib.po_qn_destroy(h)


# ---- 11. leaks --------------------------------------------------------------------------------------------------------
def test_no_leaks(ctx):
    import paropt_amd as pa

    gc.collect()
    base = pa.live_objects()
    for flavour in FLAVOURS:
        n = 300
        prob = pa.SeparableProblem(ctx, "quadratic", n, 2)
        ip = pa.InteriorPoint(prob, {"qn_subspace_size": 3, "max_major_iters": 6, "write_output_frequency": 0})
        q = make_user_qn(flavour, ctx, n, "bfgs", 3)
        ip.setQuasiNewton(q)
        ip.optimize()
        assert q.calls["update"] > 0
        ip.setQuasiNewton(None)
        del ip, q, prob
        gc.collect()
    assert pa.live_objects() == base
