"""CPU: dense columns in the one-time host analysis of the CSR sparse constraints (paropt_amd/csrc/csr.cpp).  A column
of Aw that enters (nearly) every row would make S = C + Aw D^-1 Aw^T dense; the analysis takes such columns J out
(S0 = C + As D^-1 As^T is ordered and factored) and records them for the low-rank correction S = S0 + V E V^T.
Checked here through the C ABI: the rule and its three modes, the structure of S0, a numpy restatement of the
low-rank solve on the emulated device factor, and that nothing changes where no column qualifies."""
import ctypes as C
import re

import numpy as np
import pytest

from paropt_amd import CsrSymbolic
from paropt_amd.lib import ParOptAMDError

from csr_dense_helpers import add_dense_columns, split_matrices, woodbury_solve
from csr_helpers import chain_pattern, dense_jacobian, emulate_factor
from test_csr_symbolic import CASES


def epigraph_pattern():
    """chain_pattern(40000, 2, 1) plus one variable appended to every row: about 1.6e9 pairs in Aw Aw^T"""
    rowp, cols = chain_pattern(40000, 2, 1)
    return add_dense_columns(40000, rowp, cols, 1)


def test_automatic_rule_lifts_the_refusal():
    n, rowp, cols = epigraph_pattern()
    assert n == 40001 and len(rowp) - 1 == 39999
    sym = CsrSymbolic(n, rowp, cols)  # refused before the rule existed
    assert sym.dense_cols == [40000]
    plain = CsrSymbolic(40000, *chain_pattern(40000, 2, 1))
    assert plain.dense_cols == []
    assert (sym.nnzS, sym.nnzL, sym.nlevels) == (plain.nnzS, plain.nnzL, plain.nlevels)
    assert sym.nnz == rowp[-1]
    with pytest.raises(ParOptAMDError, match="1.5e9"):
        CsrSymbolic(n, rowp, cols, dense_column_rows=-1)


def _explicit_cases():
    chain = (300, *chain_pattern(300, 2, 1))
    cases = {}
    for r in (1, 2, 9):
        cases["chain2_r%d" % r] = (add_dense_columns(*chain, r), 100, r)
    cases["dense_first_unsorted"] = (add_dense_columns(*chain, 2, first=True), 100, 2)
    cases["sixty_percent"] = (add_dense_columns(*chain, 1, fraction=0.6, seed=3), 100, 1)
    # rows whose only entry is the dense one (the rows of the empty_rows case, made longer)
    rowp = np.array([0, 0, 2, 2, 3, 3] + [3 + 2 * k for k in range(1, 41)], dtype=np.intc)
    cols = np.array([4, 1, 4] + [c for k in range(40) for c in (5 + k, 6 + k)], dtype=np.intc)
    cases["only_entry_dense"] = (add_dense_columns(50, rowp, cols, 1), 40, 1)
    return cases


EXPLICIT = _explicit_cases()


@pytest.mark.parametrize("name", sorted(EXPLICIT))
def test_explicit_rule(name):
    (n, rowp, cols), min_rows, r = EXPLICIT[name]
    w = len(rowp) - 1
    sym = CsrSymbolic(n, rowp, cols, dense_column_rows=min_rows)
    assert sym.dense_cols == list(range(n - r, n))
    if name == "sixty_percent":
        count = int(np.sum(cols == n - 1))
        assert 0.5 * w < count < 0.7 * w
    assert sorted(sym.perm.tolist()) == list(range(w)) and sym.nnz == rowp[-1]
    rng = np.random.default_rng(0)
    data = rng.uniform(-1.5, 1.5, size=int(rowp[-1]))
    A = dense_jacobian(n, rowp, cols, data)
    d = rng.uniform(0.2, 3.0, size=n)
    c = rng.uniform(0.05, 2.0, size=w)
    S, S0, V, E = split_matrices(A, d, c, sym.dense_cols)
    if name == "only_entry_dense":
        assert np.count_nonzero(np.abs(A[:, : n - r]).sum(axis=1) == 0) >= 3  # rows left empty in As
    # the structure checks of test_csr_symbolic.test_symbolic_structure, on S0
    As = A.copy()
    As[:, sym.dense_cols] = 0.0
    assert sym.nnzS == np.count_nonzero(np.tril((np.abs(As) @ np.abs(As).T) + np.eye(w)))
    for i in range(w):
        row = sym.Lcols[sym.Lrowp[i]:sym.Lrowp[i + 1]]
        assert row[-1] == i and np.all(np.diff(row) > 0)
        assert sym.parent[i] == -1 or sym.parent[i] > i
    L, Sp = emulate_factor(sym, S0)
    np.testing.assert_allclose(L @ L.T, Sp, rtol=1e-12, atol=1e-12)
    mask = np.zeros((w, w), dtype=bool)
    for i in range(w):
        mask[i, sym.Lcols[sym.Lrowp[i]:sym.Lrowp[i + 1]]] = True
    assert np.all(np.abs(np.linalg.cholesky(Sp)[~mask]) < 1e-13)
    level = np.zeros(w, dtype=int)
    for lev in range(sym.nlevels):
        level[sym.level_ptr[lev]:sym.level_ptr[lev + 1]] = lev
    ii, jj = np.nonzero(np.tril(mask, -1))
    same_front = (sym.front_of[ii] >= 0) & (sym.front_of[ii] == sym.front_of[jj])
    assert np.all((level[ii] > level[jj]) | same_front)
    # the low-rank solve built from that L against a dense solve of S
    for trial in range(2):
        b = rng.standard_normal(w)
        ref = np.linalg.solve(S, b)
        got = woodbury_solve(L, sym.perm, V, E, b)
        assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def _raw_arrays(create):
    import paropt_amd.lib as L

    h = L.po_csr_symbolic()
    L.check(create(h))
    try:
        info = (C.c_int64 * 7)()
        L.check(L.lib.po_csr_symbolic_info(h, info))
        ptrs = [L.c_int_p() for _ in range(6)]
        L.check(L.lib.po_csr_symbolic_arrays(h, *[C.byref(p) for p in ptrs]))
        dc, cnt = L.c_int_p(), C.c_int(-1)
        L.check(L.lib.po_csr_symbolic_dense_columns(h, C.byref(dc), C.byref(cnt)))
        return info, ptrs, cnt.value, h
    except Exception:
        L.lib.po_csr_symbolic_destroy(h)
        raise


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_dense_column_changes_nothing(name):
    import paropt_amd.lib as L

    n, rowp, cols = CASES[name]()
    rowp = np.ascontiguousarray(rowp, dtype=np.intc)
    cols = np.ascontiguousarray(cols, dtype=np.intc)
    w = len(rowp) - 1
    rp, cl = rowp.ctypes.data_as(L.c_int_p), cols.ctypes.data_as(L.c_int_p)
    a = _raw_arrays(lambda h: L.lib.po_csr_symbolic_create(n, w, rp, cl, C.byref(h)))
    b = _raw_arrays(lambda h: L.lib.po_csr_symbolic_create_split(n, w, rp, cl, 0, C.byref(h)))
    try:
        assert list(a[0]) == list(b[0]) and a[2] == b[2] == 0
        nnzL, nlev = int(a[0][2]), int(a[0][3])
        for k, size in enumerate((w, w, w + 1, nnzL, nlev + 1, w)):
            if size > 0:
                np.testing.assert_array_equal(np.ctypeslib.as_array(a[1][k], shape=(size,)),
                                              np.ctypeslib.as_array(b[1][k], shape=(size,)))
    finally:
        L.lib.po_csr_symbolic_destroy(a[3])
        L.lib.po_csr_symbolic_destroy(b[3])
    # the Python layer: the same fields as the rule-less constructor
    s0, s1 = CsrSymbolic(n, rowp, cols), CsrSymbolic(n, rowp, cols, dense_column_rows=-1)
    assert s0.dense_cols == s1.dense_cols == []
    for f in ("perm", "parent", "Lrowp", "Lcols", "level_ptr", "front_of"):
        np.testing.assert_array_equal(getattr(s0, f), getattr(s1, f))


def test_more_than_64_qualifying_columns_are_refused():
    rowp, cols = chain_pattern(120, 2, 1)
    n, rowp, cols = add_dense_columns(120, rowp, cols, 65)
    with pytest.raises(ParOptAMDError, match=r"\b65 columns"):
        CsrSymbolic(n, rowp, cols, dense_column_rows=100)
    n, rowp, cols = add_dense_columns(120, *chain_pattern(120, 2, 1), 64)
    assert CsrSymbolic(n, rowp, cols, dense_column_rows=100).dense_cols == list(range(120, 184))


def test_remaining_pairs_are_still_refused_with_the_count():
    # two columns in every row; a rule that catches neither leaves the pattern as dense as it was
    rowp, cols = chain_pattern(40000, 2, 1)
    n, rowp, cols = add_dense_columns(40000, rowp, cols, 1)
    with pytest.raises(ParOptAMDError, match=r"1\.5e9.*\b0 columns"):
        CsrSymbolic(n, rowp, cols, dense_column_rows=39999 + 1)


NEW_SYMBOLS = {
    "po_problem_set_sparse_dense_columns": (C.c_int, ["po_problem", C.c_int64]),
    "po_problem_sparse_dense_columns": (C.c_int, ["po_problem", "int**", "int*"]),
    "po_csr_symbolic_create_split": (C.c_int, [C.c_int64, C.c_int64, "int*", "int*", C.c_int64, "sym*"]),
    "po_csr_symbolic_dense_columns": (C.c_int, ["po_csr_symbolic", "int**", "int*"]),
}


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import os

    import paropt_amd.lib as L
    from conftest import ROOT

    named = {"po_problem": L.po_problem, "po_csr_symbolic": L.po_csr_symbolic, "int*": L.c_int_p, "int**": L.c_int_pp,
             "sym*": C.POINTER(L.po_csr_symbolic)}
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paropt_amd.h")).read(), flags=re.S)
    for name, (res, args) in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "include/paropt_amd.h does not declare %s" % name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hasattr(L.lib, name), "libparopt_amd.so does not export %s" % name
        sig = L.SIGNATURES[name]
        assert sig[0] is res and [str(t) for t in sig[1]] == [str(named.get(a, a)) for a in args], (name, sig)
