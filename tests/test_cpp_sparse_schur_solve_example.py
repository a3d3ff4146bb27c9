"""examples/sparse_schur_solve_amd.cpp: ParOptSparseCholesky factoring and solving with its own Schur complement
through the C++ facade -- the KKT system with a zero corner reduced onto its constraint block, a diagonal shift for the
factorization, factorSchur, and the whole solve refined against the retained matrix.  The dense restatement of the same
system (sparse_refine_helpers.zero_corner_saddle) gives the bound."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sparse_ldlt_helpers import bound_for
from sparse_refine_helpers import zero_corner_saddle

EXE = os.path.join(ROOT, "examples", "sparse_schur_solve_amd")


def build():
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "sparse_schur_solve_amd"], env=env,
                          stdout=subprocess.DEVNULL)
    return EXE


def test_example_builds_and_refuses_to_run_without_a_gpu():
    import torch

    exe = build()
    if torch.cuda.is_available():
        return  # covered by the gpu test
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 2 and "no MI355X available" in res.stderr


@pytest.mark.gpu
def test_cpp_schur_solve_example_refines_to_the_bound(tmp_path):
    exe = build()
    res = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    K, shift, nm = zero_corner_saddle(8)
    n = K.shape[0]
    bound, e_lap = bound_for(K, K @ np.ones(n))
    print("sparse_schur_solve_amd:", out, "bound", bound, "eta_lapack", e_lap)
    assert out["n"] == n and out["ns"] == n - nm
    assert out["inertia"] == [nm, 0, 0] and out["schur_inertia"] == [0, n - nm, 0]
    assert out["factor_info"] == 0 and out["schur_factor_info"] == 0
    assert out["eta0"] > bound  # the plain solve of the shifted system is not a solution of this one
    assert out["eta"] <= bound, (out["eta"], bound)
    assert 1 <= out["steps"] <= 5
