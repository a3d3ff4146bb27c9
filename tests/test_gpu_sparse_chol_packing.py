"""Packed groups of tiny fronts on the device (sparse_chol.hip: chol_pack_*): whatever the cap, the factor and every
solve are bit for bit what the unpacked kernels (cap 0) give, pivot reports included; and the solutions stay within
the project's bound against LAPACK."""
import numpy as np
import pytest

from sparse_chol_helpers import dense_from_csc
from sparse_chol_packing_helpers import CAPS, EPS, eta, pack_cap, spd_system

pytestmark = pytest.mark.gpu

SHAPES = ["tridiag70", "tridiag1000", "forest", "grid12", "arrow", "clique8"]
ONLY_GROUPS_OF_ONE = ("arrow", "clique8")  # their tiny fronts sit over children that are not tiny
NRHS = (1, 3, 32, 33)
_CASES = {}


@pytest.fixture(scope="module")
def ctx():
    import paropt_amd as pa

    c = pa.Context(0)
    yield c
    c.close()


def solver(ctx, name, cap, vals=None):
    import paropt_amd as pa

    n, colp, rows, v, order = spd_system(name, 3)
    with pack_cap(cap):
        s = pa.SparseCholesky(ctx, n, colp, rows, order=order)
    assert s.packing()["cap"] == cap
    s.set_values(v if vals is None else vals)
    return s


def case(ctx, name):
    """the system, 33 right-hand sides and what cap 0 makes of them; made once per shape and left alone"""
    if name not in _CASES:
        n, colp, rows, vals, order = spd_system(name, 3)
        B = np.random.default_rng(17).standard_normal((33, n))
        s = solver(ctx, name, 0)
        assert s.factor() == 0
        assert all(v == 0 for k, v in s.kernel_forms().items() if k.startswith("pack_"))
        _CASES[name] = dict(n=n, colp=colp, rows=rows, vals=vals, B=B, ref={k: s.solve(B[:k]) for k in NRHS},
                            single=s.solve(B[0]))
    return _CASES[name]


@pytest.mark.parametrize("name", SHAPES)
def test_every_cap_gives_the_bits_of_cap_0(ctx, name):
    from scipy.linalg import cho_factor, cho_solve

    k = case(ctx, name)
    A = dense_from_csc(k["n"], k["colp"], k["rows"], k["vals"])
    xl = cho_solve(cho_factor(A, lower=True), k["B"].T).T
    multi = 0
    for cap in CAPS:
        s = solver(ctx, name, cap)
        p = s.packing()
        assert p["num_groups"] > 0 and s.kernel_forms()["pack_factor"] > 0
        multi += int((p["group_root"] > p["group_first"]).sum())
        assert s.factor() == 0
        for nrhs in NRHS:
            X = s.solve(k["B"][:nrhs])
            assert np.array_equal(X, k["ref"][nrhs]), (name, cap, nrhs, float(np.abs(X - k["ref"][nrhs]).max()))
        assert np.array_equal(s.solve(k["B"][0]), k["single"]), (name, cap)
        X = s.solve(k["B"])
        for j in range(33):
            e_dev, e_lap = eta(A, X[j], k["B"][j]), eta(A, xl[j], k["B"][j])
            assert e_dev <= max(16.0 * e_lap, 64.0 * EPS), (name, cap, j, e_dev, e_lap)
    assert (multi > 0) == (name not in ONLY_GROUPS_OF_ONE)


@pytest.mark.parametrize("name", SHAPES)
def test_bad_pivot_inside_a_group_is_reported_as_without_packing(ctx, name):
    k = case(ctx, name)
    cols = np.repeat(np.arange(k["n"]), np.diff(k["colp"]))
    ones = np.ones(k["n"])
    for cap in (2, 16):
        s = solver(ctx, name, cap)
        p = s.packing()
        size = p["group_root"] - p["group_first"] + 1
        g = int(np.argmax(size))
        f, r = int(p["group_first"][g]), int(p["group_root"][g])
        # a front in the middle of the group: neither its root nor a leaf, so it has a child inside the group and a
        # parent inside the group (in a group of fewer than three fronts, the first front)
        mid = [J for J in range(f + 1, r) if (s.snode_parent[f:J] == J).any()]
        J = mid[len(mid) // 2] if mid else f
        assert bool(mid) == (name not in ONLY_GROUPS_OF_ONE and cap >= 3), (name, cap, f, r)
        col = int(s.snode_first[J])
        bad = int(s.perm[col])
        v = k["vals"].copy()
        # (far below what the children subtract: the pivot is bad whatever they bring, and is the first bad one,
        # the columns before it in the postorder do not depend on it)
        v[(k["rows"] == bad) & (cols == bad)] = -1.0
        s.set_values(v)
        info = s.factor()
        s0 = solver(ctx, name, 0, vals=v)
        assert info == s0.factor() == 1 + col, (name, cap, info, col)
        assert np.array_equal(s.solve(ones), s0.solve(ones))
        s.set_values(k["vals"])
        assert s.factor() == 0
        assert np.array_equal(s.solve(k["B"][:3]), k["ref"][3])


@pytest.mark.parametrize("name", SHAPES)
def test_refactoring_is_deterministic(ctx, name):
    k = case(ctx, name)
    vals2 = spd_system(name, 4)[3] * 3.0
    s0 = solver(ctx, name, 0, vals=vals2)
    assert s0.factor() == 0
    ref = s0.solve(k["B"][:3])
    assert not np.array_equal(ref, k["ref"][3])
    s = solver(ctx, name, 16)
    assert s.factor() == 0
    for _ in range(2):  # the same object with other values: nothing stale in the arena or the panels
        s.set_values(vals2)
        assert s.factor() == 0
        assert np.array_equal(s.solve(k["B"][:3]), ref)
    s.set_values(k["vals"])
    assert s.factor() == 0
    assert np.array_equal(s.solve(k["B"][:3]), k["ref"][3])


def test_solve_tensor_goes_through_the_packed_sweeps(ctx):
    import torch

    k = case(ctx, "tridiag1000")
    s = solver(ctx, "tridiag1000", 16)
    assert s.factor() == 0
    t = torch.tensor(k["B"], dtype=torch.float64, device="cuda:%d" % ctx.device())
    s.solve_tensor(t)
    assert np.array_equal(t.cpu().numpy(), k["ref"][33])
