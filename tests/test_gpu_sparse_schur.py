"""pa.SparseCholesky with a Schur set on the device: the partial factorization that leaves S = A22 - A21 A11^-1 A12,
reading S, and the two halves of the solve.

Two measures, every value of which goes to profiles/r27_sparse_schur_parity.json:
  d(S) = max|S_dev - S_ref| / max(|A22| + |A21| |A11^-1 A12|), S_ref from numpy.linalg.solve on the dense matrix, bound
         max(16 d_restate, 64 eps) with d_restate the same measure of the numpy restatement of the partial elimination
         in the handle's own order (sparse_schur_helpers.partial_nopivot) -- the factor 16 is the margin the other
         sparse-factor tests give the device over LAPACK;
  eta  = the backward error of condense, numpy.linalg.solve(S_dev, g), expand, bound max(16 eta_LAPACK, 64 eps)
         (sparse_ldlt_helpers.eta, bound_for).
Shapes: ns in {1, 8, 31, 33, 65, 130} (tiny, one wavefront, either side of the block width 32, past the 64-edge tile of
the copy kernel, more than two tiles), nrhs in (1, 3, 32, 33) (either side of a slab), packing caps (0, 2, 16)."""
import numpy as np
import pytest

from sparse_chol_helpers import csc_from_triplets, dense_from_csc, forest_triplets, mass_triplets
from sparse_chol_packing_helpers import pack_cap
from sparse_ldlt_helpers import (EPS, bordered_mass_system, bound_for, dense_csc, dense_spd, eta,
                                 grid3_quasi_definite, grid3_system)
from sparse_refine_helpers import dense_to_csc
from sparse_schur_helpers import (d_bound, d_measure, fanin_kkt, inertia_dense, record, schur_dense, write_records)

pytestmark = pytest.mark.gpu

NRHS = (1, 3, 32, 33)
CAPS = (0, 2, 16)
_SYS = {}


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()
    write_records()


def system(name):
    """name -> dict(n, colp, rows, vals, A (dense), sc (the Schur set), kind); made once and left alone"""
    if name in _SYS:
        return _SYS[name]
    kind = "llt"
    if name == "mass4_s8":
        n, R, Cc, V = mass_triplets(4)
        colp, rows, vals = csc_from_triplets(n, R, Cc, V)
        sc = np.random.default_rng(1).permutation(n)[:8]
    elif name.startswith("grid3_s"):  # scattered sets of every size of the list
        n, colp, rows, vals = grid3_system((6, 5, 4), 3)
        sc = np.random.default_rng(2).permutation(n)[:int(name[7:])]
    elif name == "grid3_plane":
        n, colp, rows, vals = grid3_system((6, 5, 4), 3)
        sc = np.arange(n).reshape(6, 5, 4)[3].ravel()
    elif name == "dense200_s130":
        n = 200
        colp, rows, vals = dense_csc(dense_spd(n, 11))
        sc = np.random.default_rng(3).permutation(n)[:130]
    elif name == "forest_in":
        n, R, Cc, V = forest_triplets()
        colp, rows, vals = csc_from_triplets(n, R, Cc, V)
        sc = 30 + np.arange(42).reshape(7, 6)[3]
    elif name == "grid3_qd":  # onto the whole negative block
        n, colp, rows, vals, odd = grid3_quasi_definite((6, 5, 4))
        sc, kind = np.nonzero(odd)[0], "ldlt"
    elif name == "bordered_mass":  # onto the constraints
        K, nm = bordered_mass_system(4)
        n = K.shape[0]
        colp, rows, vals = dense_to_csc(K)
        sc, kind = np.arange(nm, n), "ldlt"
    elif name == "fanin300":
        K, nE = fanin_kkt(300, 3, 33)
        n = K.shape[0]
        colp, rows, vals = dense_to_csc(K)
        sc, kind = np.arange(nE, n), "ldlt"
    else:
        raise KeyError(name)
    sc = [int(v) for v in sc]
    B = np.random.default_rng(17).standard_normal((33, n))
    _SYS[name] = dict(n=n, colp=colp, rows=rows, vals=vals, A=dense_from_csc(n, colp, rows, vals), sc=sc, kind=kind,
                      B=B)
    return _SYS[name]


def handle(ctx, k, cap=None, factor=True, **kw):
    import paropt_amd as pa

    with pack_cap(cap):
        s = pa.SparseCholesky(ctx, k["n"], k["colp"], k["rows"], factorization=k["kind"], schur=k["sc"], **kw)
    s.set_values(k["vals"])
    if factor:
        assert s.factor() == 0
    return s


def full_solve(s, k, B):
    """condense, numpy.linalg.solve(S_dev, g), expand: (x, g-stage array, S)"""
    S = s.schur()
    y = s.condense(B)
    z = y.copy()
    z[..., k["sc"]] = np.linalg.solve(S, y[..., k["sc"]].T).T
    return s.expand(z), y, S


LLT = ["mass4_s8", "grid3_plane", "dense200_s130", "forest_in", "grid3_s1", "grid3_s31", "grid3_s33", "grid3_s65"]
LDLT = ["grid3_qd", "bordered_mass"]


@pytest.mark.parametrize("name", LLT + LDLT)
def test_schur_complement_against_the_dense_formula(ctx, name):
    k = system(name)
    s = handle(ctx, k)
    ns, n = len(k["sc"]), k["n"]
    assert s.num_schur == ns and s.perm[n - ns:].tolist() == k["sc"]
    S = s.schur()
    assert S.shape == (ns, ns) and np.isfinite(S).all() and np.array_equal(S, S.T)  # bit for bit
    S_ref, scale, interior = schur_dense(k["A"], k["sc"])
    bound, d_restate = d_bound(k["A"], k["sc"], s.perm)
    d = d_measure(S, S_ref, scale)
    record("S|" + name, d_device=d, d_restate=d_restate, bound=bound, ns=ns, children=s.schur_info()["children"])
    assert d <= bound, (name, d, d_restate)
    pos, neg, rep = s.inertia()
    assert pos + neg + rep == n - ns and rep == 0
    if k["kind"] == "ldlt":  # inertia is additive over the partial factorization
        sp, sn, sz = inertia_dense(S)
        assert (pos + sp, neg + sn, sz) == inertia_dense(k["A"])
    else:
        assert (pos, neg) == (n - ns, 0)
    # a leading dimension above ns, on the device
    import torch

    lds = ns + 3
    t = torch.full((ns * lds,), -7.0, dtype=torch.float64, device="cuda")
    s.schur_device(t, lds)
    T = t.cpu().numpy().reshape(ns, lds)  # (column, row)
    assert np.array_equal(T[:, :ns].T, S) and (T[:, ns:] == -7.0).all()


@pytest.mark.parametrize("name", LLT + LDLT)
def test_condense_solve_expand(ctx, name):
    k = system(name)
    s = handle(ctx, k)
    A, sc, B = k["A"], k["sc"], k["B"]
    X, Y, S = full_solve(s, k, B)
    worst = 0.0
    for j in range(B.shape[0]):
        bound, e_lap = bound_for(A, B[j])
        e = eta(A, X[j], B[j])
        worst = max(worst, e / bound)
        assert e <= bound, (name, j, e, e_lap)
    # g = b2 - A21 A11^-1 b1 against the dense formula: two solves with A11, each with a relative forward error of a
    # modest multiple of cond(A11) eps
    _, _, interior = schur_dense(A, sc)
    G = B[:, sc] - (A[np.ix_(sc, interior)] @ np.linalg.solve(A[np.ix_(interior, interior)], B[:, interior].T)).T
    assert np.abs(Y[:, sc] - G).max() <= 1e3 * EPS * np.abs(G).max() * np.linalg.cond(A[np.ix_(interior, interior)])
    # x2 = 0: the interior solve
    Z = Y.copy()
    Z[:, sc] = 0.0
    X0 = s.expand(Z)
    A11 = A[np.ix_(interior, interior)]
    worst0 = 0.0
    for j in range(B.shape[0]):
        bound, e_lap = bound_for(A11, B[j, interior])
        e = eta(A11, X0[j, interior], B[j, interior])
        worst0 = max(worst0, e / bound)
        assert e <= bound, (name, j, e, e_lap)
    assert np.array_equal(X0[:, sc], Z[:, sc])
    record("solve|" + name, worst_eta_over_bound=worst, worst_interior_eta_over_bound=worst0)


@pytest.mark.parametrize("name", ["forest_in", "grid3_s33", "grid3_qd", "fanin300"])
def test_bits_do_not_depend_on_cap_nrhs_or_entry(ctx, name):
    import torch

    k = system(name)
    B, sc = k["B"], k["sc"]
    s0 = handle(ctx, k, cap=0)
    X, Y, S = full_solve(s0, k, B)
    Z = Y.copy()
    Z[:, sc] = np.linalg.solve(S, Y[:, sc].T).T
    for cap in CAPS[1:]:
        s = handle(ctx, k, cap=cap)
        assert s.packing()["cap"] == cap
        assert np.array_equal(s.schur(), S), (name, cap)
        assert np.array_equal(s.condense(B), Y) and np.array_equal(s.expand(Z), X), (name, cap)
    for nrhs in NRHS:  # a column's bits do not depend on the columns beside it
        assert np.array_equal(s0.condense(B[:nrhs]), Y[:nrhs]) and np.array_equal(s0.expand(Z[:nrhs]), X[:nrhs])
    for j in (0, 7, 32):
        assert np.array_equal(s0.condense(B[j]), Y[j]) and np.array_equal(s0.expand(Z[j]), X[j])
    # host entry against device entry
    t = torch.tensor(B, dtype=torch.float64, device="cuda")
    assert np.array_equal(s0.condense_tensor(t).cpu().numpy(), Y)
    t = torch.tensor(Z, dtype=torch.float64, device="cuda")
    assert np.array_equal(s0.expand_tensor(t).cpu().numpy(), X)
    ns = len(sc)
    t = torch.zeros((ns, ns), dtype=torch.float64, device="cuda")
    s0.schur_device(t, ns)
    assert np.array_equal(t.cpu().numpy().T, S)


@pytest.mark.parametrize("name", ["mass4_s8", "grid3_qd"])
def test_an_empty_set_is_the_plain_handle(ctx, name):
    import paropt_amd as pa

    k = system(name)
    a = pa.SparseCholesky(ctx, k["n"], k["colp"], k["rows"], factorization=k["kind"])
    b = pa.SparseCholesky(ctx, k["n"], k["colp"], k["rows"], factorization=k["kind"], schur=[])
    assert np.array_equal(a.perm, b.perm) and a.work_bytes == b.work_bytes
    assert a.kernel_forms(33) == b.kernel_forms(33)
    for s in (a, b):
        s.set_values(k["vals"])
        assert s.factor() == 0
    assert a.inertia() == b.inertia()
    assert np.array_equal(a.solve(k["B"]), b.solve(k["B"]))


def test_the_whole_matrix_as_the_set(ctx):
    import paropt_amd as pa

    n, R, Cc, V = mass_triplets(4)  # the element loop repeats entries: they add up in entry order
    colp, rows, vals = csc_from_triplets(n, R, Cc, V)
    sc = [int(v) for v in np.random.default_rng(6).permutation(n)]
    s = pa.SparseCholesky(ctx, n, colp, rows, schur=sc)
    s.set_values(vals)
    assert s.factor() == 0 and s.inertia() == (0, 0, 0)
    A = dense_from_csc(n, colp, rows, vals)
    assert np.array_equal(s.schur(), A[np.ix_(sc, sc)])
    b = np.arange(1.0, n + 1.0)
    assert np.array_equal(s.condense(b), b) and np.array_equal(s.expand(b), b)


def test_fan_in(ctx):
    k = system("fanin300")
    s = handle(ctx, k)
    info = s.schur_info()
    assert info["children"] == 300 and info["num_schur"] == 33
    assert info["gather_entries"] == 300 * 33 * 34 // 2
    assert s.kernel_forms()["schur_gather"] == 1
    S = s.schur()
    S_ref, scale, _ = schur_dense(k["A"], k["sc"])
    bound, d_restate = d_bound(k["A"], k["sc"], s.perm)
    d = d_measure(S, S_ref, scale)
    X, _, _ = full_solve(s, k, k["B"][:3])
    worst = 0.0
    for j in range(3):
        eb, e_lap = bound_for(k["A"], k["B"][j])
        e = eta(k["A"], X[j], k["B"][j])
        worst = max(worst, e / eb)
        assert e <= eb, (j, e, e_lap)
    record("fanin300", d_device=d, d_restate=d_restate, bound=bound, worst_eta_over_bound=worst,
           children=info["children"])
    assert d <= bound and np.array_equal(S, S.T)
    assert s.inertia() == (900, 0, 0) and inertia_dense(S) == (0, 33, 0)


def test_contract(ctx):
    import gc

    import paropt_amd as pa

    gc.collect()
    ctx.synchronize()
    before = pa.live_objects()
    k = system("grid3_qd")
    n, sc, A = k["n"], k["sc"], k["A"]
    s = handle(ctx, k, factor=False, keep_matrix=True)
    with pytest.raises(pa.ParOptAMDError) as e:
        s.schur()
    assert "after factor()" in str(e.value)
    with pytest.raises(pa.ParOptAMDError):
        s.condense(np.ones(n))
    assert s.factor() == 0
    S = s.schur()
    for call in (lambda: s.solve(np.ones(n)), lambda: s.solve_refined(np.ones(n))):
        with pytest.raises(pa.ParOptAMDError) as e:
            call()
        assert "solve_condense()" in str(e.value) and "solve_expand()" in str(e.value)
    with pytest.raises(pa.ParOptAMDError):  # a leading dimension below ns
        import paropt_amd.lib as L
        L.check(L.lib.po_sparse_chol_get_schur(s.handle, S.ctypes.data_as(L.c_double_p), len(sc) - 1))
    x = np.random.default_rng(5).standard_normal((3, n))
    assert np.abs(s.matvec(x) - x @ A).max() <= 64 * EPS * (np.abs(x) @ np.abs(A)).max()  # the whole A (symmetric)
    # a diagonal shift reaches A22 like any diagonal: the dense formula on the shifted matrix
    shift = np.zeros(n)
    shift[sc] = -0.25 - 0.01 * np.arange(len(sc))
    s.set_diagonal_shift(shift)
    s.set_values(k["vals"])
    with pytest.raises(pa.ParOptAMDError):  # set_values ends the validity of S
        s.schur()
    assert s.factor() == 0
    S2 = s.schur()
    off = ~np.eye(len(sc), dtype=bool)
    assert np.array_equal(S2[off], S[off])  # A11 is unchanged: only the diagonal of S moves
    S_ref, scale, _ = schur_dense(A + np.diag(shift), sc)
    bound, d_restate = d_bound(A + np.diag(shift), sc, s.perm)
    assert d_measure(S2, S_ref, scale) <= bound
    assert np.abs((S2 - S).diagonal() - shift[sc]).max() <= 4 * EPS * scale
    shift[:] = 0.125  # through A11 as well
    s.set_diagonal_shift(shift)
    s.set_values(k["vals"])
    assert s.factor() == 0
    S_ref, scale, _ = schur_dense(A + np.diag(shift), sc)
    bound, d_restate = d_bound(A + np.diag(shift), sc, s.perm)
    d = d_measure(s.schur(), S_ref, scale)
    record("shift|grid3_qd", d_device=d, d_restate=d_restate, bound=bound)
    assert d <= bound
    assert np.abs(s.matvec(x) - x @ A).max() <= 64 * EPS * (np.abs(x) @ np.abs(A)).max()  # the retained A has no shift
    s.condense(np.ones((40, n)))
    assert pa.live_objects()[1] > before[1]
    s.close()
    ctx.synchronize()
    assert pa.live_objects() == before
