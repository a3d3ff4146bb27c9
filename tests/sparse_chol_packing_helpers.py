"""Shared by the tests of the packed groups of tiny fronts (sparse Cholesky): the debug switch that sets the cap, the
patterns, a numpy restatement of the grouping rule, and the CSR problems of the interior point's side."""
import contextlib

import numpy as np

from csr_dense_helpers import add_dense_columns
from csr_helpers import chain_pattern, dense_jacobian, grid_pattern
from sparse_chol_helpers import csc_from_triplets, forest_triplets, tridiag_triplets

SW_CHOL_PACK = 38  # core.hpp DbgSwitch
TINY = 8
CAPS = (1, 2, 16, 64)
DEFAULT_CAP = 0  # sparse_chol.hpp kCholPackMax: packing is off unless the switch sets a cap
EPS = float(np.finfo(np.float64).eps)


@contextlib.contextmanager
def pack_cap(cap):
    """the cap in force for every analysis made inside; back to the default afterwards (cap None: the default)"""
    from paropt_amd.lib import lib

    lib.po_debug_set_switch(SW_CHOL_PACK, -1 if cap is None else int(cap))
    try:
        yield
    finally:
        lib.po_debug_set_switch(SW_CHOL_PACK, -1)


def grid2_triplets(nx, ny):
    """pattern of the 5-point stencil, every entry once"""
    ids = np.arange(nx * ny).reshape(nx, ny)
    R, C = [ids.ravel()], [ids.ravel()]
    for a, b in ((ids[:-1], ids[1:]), (ids[:, :-1], ids[:, 1:])):
        R += [a.ravel(), b.ravel()]
        C += [b.ravel(), a.ravel()]
    return nx * ny, np.concatenate(R), np.concatenate(C)


def arrow_triplets():
    """A 10-clique whose vertices all touch vertex 10, plus the edges 10-11 and 11-12.  In the natural order the first
    front has s = 10, b = 1 -- not tiny -- and sits under the tiny front of vertex 10, which therefore cannot be packed
    with its subtree and runs as a group of one."""
    R, C = [], []
    for i in range(11):
        for j in range(11):
            R.append(i)
            C.append(j)
    for i, j in ((10, 11), (11, 12)):
        R += [i, j]
        C += [j, i]
    R += [11, 12]
    C += [11, 12]
    return 13, np.array(R), np.array(C)


def clique8_triplets():
    """Vertices 0 and 1, each adjacent to all of the 8-clique 2 .. 9.  In the natural order vertex 2 has two children
    and starts the supernode 2 .. 9: one front with s = 8, b = 0 -- tiny, a group of one -- over two children with
    s = 1, b = 8, which are not tiny and hand the parent all 8 rows of its front."""
    R, C = [0, 1], [0, 1]
    for v in (0, 1):
        for j in range(2, 10):
            R += [v, j]
            C += [j, v]
    for i in range(2, 10):
        for j in range(2, 10):
            R.append(i)
            C.append(j)
    return 10, np.array(R), np.array(C)


# name -> (n, R, C, order)
PATTERNS = {
    "tridiag70": lambda: tridiag_triplets(70)[:3] + ("nd",),
    "tridiag1000": lambda: tridiag_triplets(1000)[:3] + ("nd",),
    "tridiag4096": lambda: tridiag_triplets(4096)[:3] + ("nd",),
    "forest": lambda: forest_triplets()[:3] + ("nd",),
    "grid12": lambda: grid2_triplets(12, 12) + ("nd",),
    "grid40": lambda: grid2_triplets(40, 40) + ("nd",),
    "arrow": lambda: arrow_triplets() + ("natural",),
    "clique8": lambda: clique8_triplets() + ("natural",),
}


def analysis(name, cap, ctx=None):
    import paropt_amd as pa

    n, R, C, order = PATTERNS[name]()
    colp, rows = csc_from_triplets(n, R, C)
    with pack_cap(cap):
        return pa.SparseCholesky(ctx, n, colp, rows, order=order)


def spd_system(name, seed):
    """(n, colp, rows, vals, order) of a strictly diagonally dominant matrix with the pattern, entries without any
    regularity a wrong order of operations could hide behind"""
    n, R, C, order = PATTERNS[name]()
    colp, rows = csc_from_triplets(n, R, C)
    cols = np.repeat(np.arange(n), np.diff(colp))
    W = np.random.default_rng(seed).uniform(0.1, 1.0, size=(n, n))
    W = W + W.T
    off = np.zeros((n, n))
    off[rows, cols] = -W[rows, cols]
    np.fill_diagonal(off, 0.0)
    diag = np.abs(off).sum(axis=1) + 1.0 + W.diagonal()
    vals = np.where(rows == cols, diag[rows], -W[rows, cols])
    return n, colp, rows, vals, order


def groups_by_rule(snode_first, snode_parent, front_order, cap):
    """The grouping rule restated: supernodes are in postorder, so the subtree of J is [J - cnt[J] + 1, J].  J is
    packable when its order is <= TINY and all its children are; a packable J with cnt[J] <= cap is a candidate; a
    candidate whose parent is none roots a group of its subtree; every tiny front left over is a group of one.
    Returns (group_first, group_root) ascending, and the candidate flags."""
    nsn = len(snode_parent)
    cnt = np.ones(nsn, dtype=np.int64)
    packable = np.asarray(front_order) <= TINY
    for J in range(nsn):  # children come before parents
        P = snode_parent[J]
        if P >= 0:
            assert P > J
            cnt[P] += cnt[J]
            packable[P] &= packable[J]
    cand = packable & (cnt <= cap) if cap > 0 else np.zeros(nsn, dtype=bool)
    covered = np.zeros(nsn, dtype=bool)
    groups = []
    for J in range(nsn):
        P = snode_parent[J]
        if cand[J] and not (P >= 0 and cand[P]):
            groups.append((J - cnt[J] + 1, J))
            covered[J - cnt[J] + 1:J + 1] = True
    if cap > 0:
        groups += [(J, J) for J in range(nsn) if not covered[J] and front_order[J] <= TINY]
    groups.sort()
    first = np.array([g[0] for g in groups], dtype=np.intc)
    root = np.array([g[1] for g in groups], dtype=np.intc)
    return first, root, cand


def eta(A, x, b):
    """the backward error of tests/test_gpu_sparse_chol.py"""
    return float(np.abs(b - A @ x).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


# ---- the interior point's side: CSR sparse constraints on the multifrontal engine ------------------------------------
def csr_patterns():
    """name -> (n, rowp, cols, dense_column_rows): a chain of 200 sparse rows (S tridiagonal), the edges of a 10 x 10
    grid, and the chain of tests/test_gpu_csr_dense_columns.py's family with two dense columns taken out"""
    return {
        "chain200": (201,) + chain_pattern(201, 2, 1) + (0,),
        "grid10": (100,) + grid_pattern(10, 10) + (0,),
        "chain2_r2": add_dense_columns(300, *chain_pattern(300, 2, 1), 2) + (100,),
    }


def pattern_problem(ctx, n, rowp, cols, data, dense_column_rows=0):
    """a problem with fixed Jacobian entries and linear sparse constraints on the multifrontal engine, the entries
    uploaded by one gradient evaluation (tests/test_gpu_csr_multifrontal.py)"""
    import paropt_amd as pa

    A = dense_jacobian(n, rowp, cols, data)

    class _P(pa.Problem):
        def __init__(self):
            super().__init__(ctx, n, 1, 1, nwcon=len(rowp) - 1, nwinequality=len(rowp) - 1, rowp=rowp, cols=cols,
                             dense_column_rows=dense_column_rows, sparse_factor="multifrontal")

        def getVarsAndBounds(self, x, lb, ub):
            x[:], lb[:], ub[:] = 0.5, 0.0, 1.0

        def evalSparseObjCon(self, x, sparse):
            sparse[:] = 1.0 - A @ x
            return 0, float(np.sum(x * x)), np.array([1.0 - np.sum(x)])

        def evalSparseObjConGradient(self, x, g, Ac, d):
            g[:] = 2.0 * x
            Ac[0][:] = -1.0
            d[:] = data
            return 0

    prob = _P()
    pa.InteriorPoint(prob, {"max_major_iters": 0}).optimize()
    return prob, A
