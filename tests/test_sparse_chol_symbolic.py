"""The host analysis behind pa.SparseCholesky on analysis-only handles (no device): supernodes, fill, levels and
permutations against a boolean dense Cholesky in numpy; refusals; the reference's own example program against the
compat headers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sparse_chol_helpers import (csc_from_triplets, forest_triplets, grid3_triplets, mass_triplets, symbolic_fill,
                                 tridiag_triplets)


def pattern(name):
    if name.startswith("mass"):
        n, R, Cc, _ = mass_triplets(int(name[4:]))
        # the element loop repeats entries: the clean pattern has each once
        key = np.unique(Cc.astype(np.int64) * n + R)
        R, Cc = key % n, key // n
    elif name == "grid3":
        n, R, Cc = grid3_triplets(9, 8, 7)
    elif name == "tridiag":
        n, R, Cc, _ = tridiag_triplets(200)
    elif name == "diag":
        n, R, Cc = 50, np.arange(50), np.arange(50)
    elif name == "forest":
        n, R, Cc, _ = forest_triplets()
    else:
        n = 70
        R, Cc = np.divmod(np.arange(n * n), n)
    colp, rows = csc_from_triplets(n, R, Cc)
    return n, colp, rows


NAMES = ["mass12", "mass24", "grid3", "tridiag", "diag", "forest", "dense70"]


def check_structure(s, n, colp, rows):
    assert s.size == n and s.getInfo() == (n, s.num_snodes, s.nnzL)
    assert sorted(s.perm.tolist()) == list(range(n))
    sizes = np.diff(s.snode_first)
    assert s.snode_first[0] == 0 and (sizes >= 1).all() and sizes.sum() == n
    nnzL, colcount = symbolic_fill(n, colp, rows, s.perm)
    assert s.nnzL == nnzL
    # nnzL = sum s (s + 1) / 2 + b s with b from the first column of each supernode
    below = colcount[s.snode_first[:-1]] - sizes
    assert (below >= 0).all()
    assert int((sizes * (sizes + 1) // 2 + below * sizes).sum()) == nnzL
    assert s.max_snode == sizes.max() and s.max_front == (sizes + below).max()
    kids = s.snode_parent >= 0
    assert (s.snode_parent[kids] > np.nonzero(kids)[0]).all()
    assert (s.snode_level[s.snode_parent[kids]] > s.snode_level[kids]).all()
    assert s.nlevels == s.snode_level.max() + 1
    assert ((below == 0) == ~kids).all()  # a root is a supernode with nothing below it
    assert s.work_bytes > 0 and s.block_width >= 4


@pytest.mark.parametrize("order", ["nd", "natural"])
@pytest.mark.parametrize("name", NAMES)
def test_structure(name, order):
    import paropt_amd as pa

    n, colp, rows = pattern(name)
    s = pa.SparseCholesky(None, n, colp, rows, order=order)
    check_structure(s, n, colp, rows)
    if name == "dense70":
        assert s.num_snodes == 1 and s.nnzL == 70 * 71 // 2
    if name == "diag":
        assert s.num_snodes == 50 and s.nlevels == 1 and s.nnzL == 50
    if name == "forest":
        assert (s.snode_parent < 0).sum() >= 3
    if name == "tridiag" and order == "natural":
        assert s.nnzL == 2 * 200 - 1


def test_user_perm_and_amd():
    import paropt_amd as pa

    n, colp, rows = pattern("mass12")
    perm = np.random.default_rng(3).permutation(n)
    s = pa.SparseCholesky(None, n, colp, rows, order="natural", perm=perm)
    check_structure(s, n, colp, rows)
    # the reported order is a postorder of the user's elimination tree: the same fill
    assert s.nnzL == symbolic_fill(n, colp, rows, perm)[0]
    nd = pa.SparseCholesky(None, n, colp, rows, order="nd")
    amd = pa.SparseCholesky(None, n, colp, rows, order="amd")  # accepted, gets the nested dissection
    assert np.array_equal(nd.perm, amd.perm) and nd.nnzL == amd.nnzL


@pytest.mark.parametrize("name", ["mass12", "grid3", "forest"])
def test_unsorted_and_duplicated_entries_give_the_same_analysis(name):
    import paropt_amd as pa

    n, colp, rows = pattern(name)
    clean = pa.SparseCholesky(None, n, colp, rows)
    rng = np.random.default_rng(8)
    cols = np.repeat(np.arange(n), np.diff(colp))
    extra = rng.integers(0, len(rows), size=len(rows) // 3)
    R, Cc = np.concatenate([rows, rows[extra]]), np.concatenate([cols, cols[extra]])
    shuffle = rng.permutation(len(R))
    colp2, rows2 = csc_from_triplets(n, R[shuffle], Cc[shuffle])
    messy = pa.SparseCholesky(None, n, colp2, rows2)
    for f in ("perm", "snode_first", "snode_parent", "snode_level"):
        assert np.array_equal(getattr(clean, f), getattr(messy, f)), f
    assert clean.getInfo() == messy.getInfo() and clean.max_front == messy.max_front
    # one triangle only: the pattern is symmetrised
    low = R >= Cc
    colp3, rows3 = csc_from_triplets(n, R[low], Cc[low])
    half = pa.SparseCholesky(None, n, colp3, rows3)
    assert np.array_equal(clean.perm, half.perm) and clean.nnzL == half.nnzL


def test_refusals():
    import paropt_amd as pa
    import paropt_amd.lib as L

    lib = L.lib
    n, colp, rows = pattern("tridiag")
    bad = rows.copy()
    bad[5] = n
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.SparseCholesky(None, n, colp, bad)
    assert "out of range" in str(e.value)
    bad[5] = -1
    with pytest.raises(pa.ParOptAMDError):
        pa.SparseCholesky(None, n, colp, bad)
    perm = np.arange(n)
    perm[3] = 4
    with pytest.raises(pa.ParOptAMDError) as e:
        pa.SparseCholesky(None, n, colp, rows, order="natural", perm=perm)
    assert "not a permutation" in str(e.value)
    h = L.po_sparse_chol()
    assert lib.po_sparse_chol_create(None, -1, colp.ctypes.data_as(L.c_int_p), rows.ctypes.data_as(L.c_int_p), 2, None,
                                     C.byref(h)) != 0
    assert b"out of range" in lib.po_last_error()
    assert lib.po_sparse_chol_create(None, n, colp.ctypes.data_as(L.c_int_p), rows.ctypes.data_as(L.c_int_p), 7, None,
                                     C.byref(h)) != 0
    # numeric calls on an analysis-only handle
    s = pa.SparseCholesky(None, n, colp, rows)
    vals = np.ones(len(rows))
    info = C.c_int()
    x = np.ones(n)
    for call in (lambda: lib.po_sparse_chol_set_values(s.handle, n, colp.ctypes.data_as(L.c_int_p),
                                                       rows.ctypes.data_as(L.c_int_p), vals.ctypes.data_as(L.c_double_p)),
                 lambda: lib.po_sparse_chol_set_values_device(s.handle, None),
                 lambda: lib.po_sparse_chol_factor(s.handle, C.byref(info)),
                 lambda: lib.po_sparse_chol_solve(s.handle, x.ctypes.data_as(L.c_double_p), 1, n),
                 lambda: lib.po_sparse_chol_solve_device(s.handle, None, 1, n)):
        assert call() != 0
        assert b"analysis-only" in lib.po_last_error()
    with pytest.raises(pa.ParOptAMDError):
        s.factor()
    # NULL handles: refused with a message, never dereferenced
    i8 = (C.c_int64 * 8)()
    for call in (lambda: lib.po_sparse_chol_set_values(None, n, colp.ctypes.data_as(L.c_int_p),
                                                       rows.ctypes.data_as(L.c_int_p), vals.ctypes.data_as(L.c_double_p)),
                 lambda: lib.po_sparse_chol_set_values_device(None, None),
                 lambda: lib.po_sparse_chol_factor(None, C.byref(info)),
                 lambda: lib.po_sparse_chol_solve(None, x.ctypes.data_as(L.c_double_p), 1, n),
                 lambda: lib.po_sparse_chol_solve_device(None, None, 1, n),
                 lambda: lib.po_sparse_chol_info(None, i8),
                 lambda: lib.po_sparse_chol_arrays(None, None, None, None, None)):
        assert call() != 0
        assert b"null argument" in lib.po_last_error()
    assert lib.po_sparse_chol_destroy(None) == 0


REF_EXAMPLE = "/root/reference/examples/cholesky/cholesky.cpp"


@pytest.mark.skipif(not os.path.exists(REF_EXAMPLE), reason="the reference tree is only present in the build container")
def test_reference_cholesky_example_compiles_unchanged(tmp_path):
    """The reference's examples/cholesky/cholesky.cpp -- not a copy, not edited -- compiles against
    include/paropt_compat/ (ParOptAMD.h, ParOptSparseCholesky.h, ParOptSparseUtils.h) and links."""
    exe = str(tmp_path / "cholesky_example_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include", "paropt_compat"),
                           "-I/opt/conda/include", REF_EXAMPLE, "-o", exe, "-L" + os.path.join(ROOT, "paropt_amd"),
                           "-lparopt_amd", "-Wl,-rpath," + os.path.join(ROOT, "paropt_amd"),
                           "/opt/conda/lib/libmpi.so", "-Wl,-rpath-link,/usr/lib/x86_64-linux-gnu",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/conda/lib"])
    assert os.path.exists(exe)


def test_cpp_example_builds():
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "sparse_cholesky_amd"], env=env,
                          stdout=subprocess.DEVNULL)
    import torch

    if not torch.cuda.is_available():
        res = subprocess.run([os.path.join(ROOT, "examples", "sparse_cholesky_amd"), "8"], capture_output=True, text=True)
        assert res.returncode == 2 and "no MI355X available" in res.stderr
