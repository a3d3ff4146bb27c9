"""GPU: every kernel form of the CSR sparse Cholesky (paropt_amd/csrc/csr.{cpp,hip}) and the panel solves, stand-alone.

The patterns of tests/test_csr_kernel_forms.py sit on either side of each selector of csr_level_plan(); every case here
first asserts through CsrSymbolic.kernel_forms that the form under test is in the plan, then runs it.

  1. factor + single solve per form (po_quasidef_factor / po_quasidef_apply) against LAPACK's dense Cholesky solve of
     the same S.  Measure and bound are those of tests/test_gpu_sparse_chol.py: the normwise backward error
         eta = ||b - S y||_inf / (||S||_inf ||y||_inf + ||b||_inf)   of   S yw = bw - A (d o bx),
         eta_device <= max(16 eta_LAPACK, 64 eps) + 2 k eps,
     k the longest row of Aw: the last term bounds the device's own assembly of an entry of S (and of the right-hand
     side), a sum of at most k positive terms in another order than numpy's.  yx against d o (bx + A^T yw_device) to
     64 eps of its largest entry; two factorizations give equal bits.
  2. a non-positive pivot (c = -10 on one row) is reported by each kernel that flags one, and the next factorization
     with good values solves within the bound of 1.
  3. pa.quasidef_gram (the interior point's panel, gramSolve, Gram product, correction sequence) at the panel widths
     where the multi-right-hand-side solves change shape: W2 against U^T S^-1 U from the dense Cholesky in the scaling
     |dW_ij| / sqrt(W_ii W_jj) <= 1e-11 (TOL_MAT of tests/test_gpu_kat.py), W2 symmetric to the bit, the correction
     vector by the backward error of S (-out) = U alpha, and a column of a wide call equal to the same column of a
     narrow call bit for bit.

Every measured figure and the wall time of each case go to profiles/csr_forms_parity.json (cases that did not run in a
session keep their earlier record).  The shared(2049) cases are one workgroup doing 2049 column steps through global
memory: select them with -k shared_2049."""
import json
import os
import time

import numpy as np
import pytest

from conftest import ROOT
from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern, grid_pattern
from test_csr_kernel_forms import NEW_PATTERNS

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
TOL_MAT = 1e-11
PARITY = {}
PARITY_FILE = os.path.join(ROOT, "profiles", "csr_forms_parity.json")


def record(name, **figures):
    PARITY.setdefault(name, {}).update(figures)
    print(name, figures)


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as f:
            cases = json.load(f).get("cases", {})
    cases.update(PARITY)
    timed = {k: v["seconds"] for k, v in cases.items() if "seconds" in v}
    slowest = max(timed, key=timed.get) if timed else None
    fast = {k: v for k, v in timed.items() if "shared_2049" not in k}
    slowest_other = max(fast, key=fast.get) if fast else None
    with open(PARITY_FILE, "w") as f:
        json.dump({"eps": EPS, "bound_eta": "eta <= max(16 eta_lapack, 64 eps) + 2 k eps",
                   "bound_W": "|dW_ij| / sqrt(W_ii W_jj) <= %g" % TOL_MAT,
                   "slowest_case": [slowest, timed.get(slowest)],
                   "slowest_case_without_shared_2049": [slowest_other, fast.get(slowest_other)],
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


def _vec(ctx, arr):
    import paropt_amd as pa

    return pa.PVec(ctx, len(arr)).from_numpy(np.asarray(arr, dtype=float))


def sparse_rows_problem(ctx, n, rowp, cols, data, Asp, dense_column_rows=0):
    """test_gpu_csr.PatternProblem (fixed Jacobian entries, linear sparse constraints) evaluated through scipy.sparse,
    so that a pattern of 26 624 rows needs no dense Jacobian."""
    import paropt_amd as pa

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=len(rowp) - 1, nwinequality=len(rowp) - 1, rowp=rowp, cols=cols,
                             dense_column_rows=dense_column_rows)

        def getVarsAndBounds(self, x, lb, ub):
            x[:] = 0.5
            lb[:] = 0.0
            ub[:] = 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = 1.0 - Asp @ np.asarray(x)
            return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x)])

        def evalSparseObjConGradient(self, x, g, A, d):
            g[:] = 2.0 * x
            A[0][:] = -1.0
            d[:] = data
            return 0

    prob = _P()
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()  # one gradient evaluation uploads the entries
    return prob


class Case:
    """A problem on the device and the numpy side of the same S = C + A D A^T: image U = A (d o P), S^-1 B, L^-1 B,
    S X and ||S||_inf.  Built once per pattern and shared by the tests; the inputs are never changed."""

    def __init__(self, ctx, n, rowp, cols, dense_column_rows=0, problem=None, blocks=None):
        import scipy.sparse as sp
        from scipy.linalg import cho_factor

        self.ctx, self.n, self.w = ctx, n, len(rowp) - 1
        self.rowp, self.cols = rowp, cols
        rng = np.random.default_rng(5)
        self.data = rng.uniform(0.5, 1.5, size=int(rowp[-1]))  # positive entries: |A| D |A|^T <= S
        self.d = rng.uniform(0.2, 3.0, size=n)
        self.c = rng.uniform(0.5, 2.0, size=self.w)
        self.kmax = int(np.diff(rowp).max())
        self.Asp = sp.csr_matrix((self.data, cols, rowp), shape=(self.w, n))
        self.blocks = blocks
        if blocks:  # nb identical shapes of (rows, vars): batched, neither A nor S is built densely
            nb, br, bv = blocks
            A3 = np.zeros((nb, br, bv))
            dat = self.data.reshape(nb, 2 * bv)
            A3[:, np.arange(bv), np.arange(bv)] = dat[:, :bv]
            A3[:, bv, :] = dat[:, bv:]
            d3 = self.d.reshape(nb, 1, bv)
            self.A3 = A3
            self.S3 = (A3 * d3) @ A3.transpose(0, 2, 1)
            self.S3[:, np.arange(br), np.arange(br)] += self.c.reshape(nb, br)
            self.L3 = np.linalg.cholesky(self.S3)
            self.norm = float(np.abs(self.S3).sum(axis=2).max())
        else:
            self.A = self.Asp.toarray()
            self.S = np.diag(self.c) + (self.A * self.d) @ self.A.T
            self.chol = cho_factor(self.S, lower=True)
            self.norm = float(np.abs(self.S).sum(axis=1).max())
        self.prob = problem(self) if problem else sparse_rows_problem(ctx, n, rowp, cols, self.data, self.Asp,
                                                                      dense_column_rows)
        self.x = _vec(ctx, np.full(n, 0.5))
        self.dv, self.cv = _vec(ctx, self.d), _vec(ctx, self.c)
        self.good = False  # the device holds the factor of (d, c)
        self.sym = {}

    def image(self, P):
        return self.Asp @ (self.d[:, None] * P)

    def _b3(self, B):
        nb, br, _ = self.blocks
        return B.reshape(nb, br, -1)

    def solve(self, B):
        from scipy.linalg import cho_solve

        B2 = B.reshape(self.w, -1)
        X = np.linalg.solve(self.S3, self._b3(B2)).reshape(B2.shape) if self.blocks else cho_solve(self.chol, B2)
        return X.reshape(B.shape)

    def half(self, B):
        from scipy.linalg import solve_triangular

        if self.blocks:
            # (L^-1 B block by block through the explicit inverse of 26 x 26 factors: only the numpy-route figure)
            return (np.linalg.inv(self.L3) @ self._b3(B)).reshape(B.shape)
        return solve_triangular(np.tril(self.chol[0]), B, lower=True)

    def mul(self, X):
        X2 = X.reshape(self.w, -1)
        Y = (self.S3 @ self._b3(X2)).reshape(X2.shape) if self.blocks else self.S @ X2
        return Y.reshape(X.shape)

    def eta(self, y, b):
        return float(np.abs(b - self.mul(y)).max() / (self.norm * np.abs(y).max() + np.abs(b).max()))

    def factor(self):
        import paropt_amd as pa

        if not self.good:
            self.cv.from_numpy(self.c)
            pa.quasidef_factor(self.prob, self.x, self.dv, self.cv)
            self.good = True


def _packed_problem(case):
    """the callback form with packed 4 x 4 blocks on the rows of chain_pattern(240, 4, 4)"""
    from sparse_forms_helpers import _callbacks

    return _callbacks(case.ctx, case.n, 2, case.A, 4)


BUILDERS = dict({name: (lambda ctx, make=make: Case(ctx, *make())) for name, make in NEW_PATTERNS.items()
                 if not name.startswith("arrow_blocks")},
                grid_26_24=lambda ctx: Case(ctx, 26 * 24, *grid_pattern(26, 24)),
                arrow_blocks_1024_25=lambda ctx: Case(ctx, *NEW_PATTERNS["arrow_blocks_1024_25"](), blocks=(1024, 26, 25)),
                arrow_blocks_1023_25=lambda ctx: Case(ctx, *NEW_PATTERNS["arrow_blocks_1023_25"](), blocks=(1023, 26, 25)),
                grid_dense_columns_r2=lambda ctx: Case(ctx, *add_dense_columns(26 * 24, *grid_pattern(26, 24), 2),
                                                       dense_column_rows=600),
                packed_blocks_4=lambda ctx: Case(ctx, 240, *chain_pattern(240, 4, 4), problem=_packed_problem))
_CASES = {}


def case(ctx, name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name](ctx)
    return _CASES[name]


def symbolic(k, dense_column_rows=0):
    """the host analysis of the case's pattern, made once"""
    import paropt_amd as pa

    if dense_column_rows not in k.sym:
        k.sym[dense_column_rows] = pa.CsrSymbolic(k.n, k.rowp, k.cols, dense_column_rows=dense_column_rows)
    return k.sym[dense_column_rows]


def plan(k, nv=1, dense_column_rows=0):
    return symbolic(k, dense_column_rows).kernel_forms(nv)


def check_apply(name, k, with_bw, seed):
    """one po_quasidef_apply against the dense Cholesky solve; returns (yx, yw) of the device"""
    import paropt_amd as pa

    rng = np.random.default_rng(seed)
    bx = rng.standard_normal(k.n)
    bw = rng.standard_normal(k.w) if with_bw else None
    yx, yw = pa.PVec(k.ctx, k.n), pa.PVec(k.ctx, k.w)
    pa.quasidef_apply(k.prob, k.x, k.dv, k.cv, _vec(k.ctx, bx), _vec(k.ctx, bw) if with_bw else None, yx, yw)
    yx, yw = yx.to_numpy(), yw.to_numpy()
    rhs = (bw if with_bw else 0.0) - k.Asp @ (k.d * bx)
    e_dev, e_lap = k.eta(yw, rhs), k.eta(k.solve(rhs), rhs)
    bound = max(16.0 * e_lap, 64.0 * EPS) + 2.0 * k.kmax * EPS
    yx_ref = k.d * (bx + k.Asp.T @ yw)
    yx_err = float(np.abs(yx - yx_ref).max() / np.abs(yx_ref).max())
    record(name, **{"eta_device" + ("_bw" if with_bw else ""): e_dev, "eta_lapack" + ("_bw" if with_bw else ""): e_lap,
                    "bound": bound, "yx_err_eps" + ("_bw" if with_bw else ""): yx_err / EPS})
    assert np.isfinite(yw).all() and np.isfinite(yx).all()
    assert e_dev <= bound, (name, e_dev, e_lap, bound)
    assert yx_err <= 64.0 * EPS, (name, yx_err / EPS)
    return bx, yx, yw


# pattern -> the forms the case is about
FORMS_UNDER_TEST = {
    "arrow_2049_1": ["level:search"],
    "arrow_2047_1": ["level:table"],
    "arrow_256_16": ["front_rows:wide"],
    "arrow_255_16": ["front_rows:table"],
    "arrow_2049_16": ["front_rows:search", "front_syrk:search"],
    "arrow_2048_16": ["front_rows:wide", "front_syrk:table"],
    "arrow_2049_15": ["level:search"],
    "shared_2049": ["front_dense:global"],
}


@pytest.mark.parametrize("name", sorted(FORMS_UNDER_TEST))
def test_factor_and_single_solve_per_form(ctx, name):
    import paropt_amd as pa

    k = case(ctx, name)
    forms = plan(k)
    for f in FORMS_UNDER_TEST[name]:
        assert forms[f] > 0, (name, f, forms)
    if name == "arrow_2049_15":
        assert forms["level:search"] == 15  # long rows WITH predecessors among the long rows
    t0 = time.perf_counter()
    k.good = False
    k.factor()
    t_factor = time.perf_counter() - t0
    np.testing.assert_array_equal(k.cv.to_numpy(), k.c)  # the CSR form leaves C alone
    check_apply("factor|" + name, k, True, 11)
    bx, _, yw1 = check_apply("factor|" + name, k, False, 12)
    # repeated factorizations are bit-identical (no atomics anywhere)
    k.good = False
    k.factor()
    yx2, yw2 = pa.PVec(ctx, k.n), pa.PVec(ctx, k.w)
    pa.quasidef_apply(k.prob, k.x, k.dv, k.cv, _vec(ctx, bx), None, yx2, yw2)
    np.testing.assert_array_equal(yw2.to_numpy(), yw1)
    record("factor|" + name, seconds=time.perf_counter() - t0, seconds_first_factor=t_factor)


# (pattern, which row of the elimination order gets c = -10, the form whose kernel must flag it)
PIVOT_CASES = [("arrow_2049_1", "last", "level:search"), ("arrow_256_16", "last", "front_dense:lds"),
               ("shared_2049", "last", "front_dense:global"), ("arrow_2047_1", "first", "level:thin")]


@pytest.mark.parametrize("name,where,form", PIVOT_CASES, ids=["%s-%s" % (c[0], c[2]) for c in PIVOT_CASES])
def test_non_positive_pivot_is_reported_per_form(ctx, name, where, form):
    """The reported-error path of each kernel that flags a pivot.  The flagged row is the last one its kernel
    eliminates (or a leaf whose replaced pivot leaves the rest positive), so exactly one row is reported; D is scaled
    by 1 / (4 k) so that the row sum of A D A^T stays below 2 and c = -10 makes the pivot negative."""
    import paropt_amd as pa
    from paropt_amd.lib import ParOptAMDError

    k = case(ctx, name)
    sym = symbolic(k)
    forms = sym.kernel_forms(1)
    assert forms[form] > 0
    pos = k.w - 1 if where == "last" else 0
    level = int(np.searchsorted(sym.level_ptr, pos, side="right")) - 1
    if form.startswith("front_dense"):
        assert sym.front_of[pos] >= 0 and pos == k.w - 1  # the last row of the front (one front, last level)
    else:
        assert sym.front_of[pos] < 0
        length = sym.Lrowp[pos + 1] - sym.Lrowp[pos]
        assert (length > 2048) if form == "level:search" else (length <= 24 and level == 0)
    t0 = time.perf_counter()
    c_bad = k.c.copy()
    c_bad[sym.perm[pos]] = -10.0
    k.good = False
    with pytest.raises(ParOptAMDError, match="non-positive pivot in row %d of the permuted.*min C -1.000e\\+01" % pos):
        pa.quasidef_factor(k.prob, k.x, _vec(ctx, k.d / (4.0 * k.kmax)), _vec(ctx, c_bad))
    k.factor()  # good values again
    check_apply("pivot|%s|%s" % (name, form), k, True, 13)
    record("pivot|%s|%s" % (name, form), seconds=time.perf_counter() - t0)


def hash_panel(ctx, n, nv):
    """hash-filled columns with a different mean each (tests/test_gpu_vec.py::test_wgram_vs_numpy): device and numpy"""
    import paropt_amd as pa
    from oracle import paropt_oracle as po

    step = 0.1 if nv <= 80 else 0.01
    idx = np.arange(n, dtype=np.uint64)
    V = [pa.PVec(ctx, n).fill_hash(0, 20 + j, 0, 2.0, -1.0 + step * j) for j in range(nv)]
    P = np.stack([-1.0 + step * j + 2.0 * po.u01(0, 20 + j, idx) for j in range(nv)], axis=1)
    return V, P


def scaled_diff(W, Wref):
    dg = np.sqrt(np.abs(np.diag(Wref)))
    return float((np.abs(W - Wref) / np.outer(dg, dg)).max())


PANEL_CASES = ([("grid_26_24", nv) for nv in (1, 2, 4, 5, 17, 96, 97, 130)] +
               [("arrow_2049_16", 1), ("arrow_2049_16", 5), ("shared_2049", 1), ("shared_2049", 5),
                ("arrow_blocks_1024_25", 8), ("arrow_blocks_1024_25", 64), ("arrow_blocks_1023_25", 8),
                ("grid_dense_columns_r2", 5), ("grid_dense_columns_r2", 97), ("packed_blocks_4", 17)])


@pytest.mark.parametrize("name,nv", PANEL_CASES, ids=["%s-nv%d" % c for c in PANEL_CASES])
def test_panel_solves_stand_alone(ctx, name, nv):
    import paropt_amd as pa

    k = case(ctx, name)
    tag = "panel|%s|nv%d" % (name, nv)
    reversed_twin = False
    if name == "grid_26_24":
        f = plan(k, nv)
        assert f["level:table"] > 0 and f["front_dense:lds"] > 0 and f["trsv_fwd:thin"] > 0 and f["trsv_bwd:thin"] > 0
        split = 5 <= min(nv, 96)
        assert (f["trsv_fwd:wave_split"] > 0) == split and (f["trsv_bwd:wave_split"] > 0) == split
        assert (f["trsv_fwd:wave"] > 0) == (nv <= 4 or nv == 97) and (f["trsv_bwd:wave"] > 0) == (nv <= 4 or nv == 97)
    elif name == "arrow_2049_16":
        assert plan(k, nv)["front_rows:search"] == 1
    elif name == "shared_2049":
        assert plan(k, nv)["front_dense:global"] == 1
    elif name == "arrow_blocks_1024_25":
        f = plan(k, nv)
        if nv == 8:  # 1024 rows keep the wave form unsplit
            assert f["trsv_fwd:wave"] == 1 and f["trsv_fwd:wave_split"] == 0
        else:  # 65536 (row, right-hand side) items: thin, where a single right-hand side is a wavefront per row
            assert f["trsv_fwd:thin"] == 2 and f["trsv_fwd:wave"] == 0 and plan(k, 1)["trsv_fwd:wave"] == 1
            reversed_twin = True
    elif name == "arrow_blocks_1023_25":
        assert plan(k, nv)["trsv_fwd:wave_split"] == 1
    elif name == "grid_dense_columns_r2":
        assert k.prob.dense_columns == [k.n - 2, k.n - 1]
        assert plan(k, nv, 600)["trsv_bwd:wave_split"] > 0  # the backward multi-column sweep of solvePanel
    k.factor()
    V, P = hash_panel(ctx, k.n, nv)
    alpha = np.random.default_rng(nv).standard_normal(nv)
    t0 = time.perf_counter()
    W2, out = pa.quasidef_gram(k.prob, k.x, k.dv, k.cv, V, alpha=alpha)
    seconds = time.perf_counter() - t0
    out = out.to_numpy()
    # the Gram matrix against the dense Cholesky, and the spread of two numpy routes to the same matrix
    U = k.image(P)
    Wref = U.T @ k.solve(U)
    Y = k.half(U)
    err_dev, err_np = scaled_diff(W2, Wref), scaled_diff(Y.T @ Y, Wref)
    # the correction vector: S (-out) = U alpha
    b = U @ alpha
    e_dev, e_lap = k.eta(-out, b), k.eta(k.solve(b), b)
    bound = max(16.0 * e_lap, 64.0 * EPS) + 2.0 * k.kmax * EPS
    record(tag, W_err_device=err_dev, W_err_numpy_routes=err_np, W_err_device_eps=err_dev / EPS,
           W_err_numpy_routes_eps=err_np / EPS, eta_device=e_dev, eta_lapack=e_lap, bound=bound, seconds=seconds)
    assert np.isfinite(W2).all() and np.isfinite(out).all()
    assert err_dev <= TOL_MAT, (tag, err_dev)
    np.testing.assert_array_equal(W2, W2.T)
    assert e_dev <= bound, (tag, e_dev, e_lap, bound)
    # W2 without alpha is the same matrix
    if nv in (5, 17):
        W2b, none = pa.quasidef_gram(k.prob, k.x, k.dv, k.cv, V)
        assert none is None
        np.testing.assert_array_equal(W2b, W2)
    # a column of the wide call against the same column of a narrow call, bit for bit (alpha = e_j: -S^-1 U_j)
    if nv == 1:
        return
    for j in sorted({0, nv - 1, min(nv - 1, 96)}):
        e = np.zeros(nv)
        e[j] = 1.0
        wide = pa.quasidef_gram(k.prob, k.x, k.dv, k.cv, V, alpha=e)[1].to_numpy()
        if reversed_twin:
            # The wide call's forward sweep is the thin form (a thread sums a row in order), a single right-hand side
            # is the wave form (64 lanes and a shuffle tree): two summation orders by design, asserted above.  The
            # column is compared with itself at another position of an equally wide panel instead.
            e2 = np.zeros(nv)
            e2[nv - 1 - j] = 1.0
            narrow = pa.quasidef_gram(k.prob, k.x, k.dv, k.cv, V[::-1], alpha=e2)[1].to_numpy()
        else:
            narrow = pa.quasidef_gram(k.prob, k.x, k.dv, k.cv, [V[j]], alpha=[1.0])[1].to_numpy()
        np.testing.assert_array_equal(wide, narrow, err_msg="%s column %d" % (tag, j))
