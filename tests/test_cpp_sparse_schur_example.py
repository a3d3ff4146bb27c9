"""examples/sparse_schur_amd.cpp: ParOptSparseCholesky as a partial factorization through the C++ facade -- the bordered
mass system reduced onto its constraint block, S read from the device, condense and expand around a host Cholesky of
-S.  The dense restatement of the same system (sparse_ldlt_helpers.bordered_mass_system) gives the bound."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sparse_ldlt_helpers import bordered_mass_system, bound_for

EXE = os.path.join(ROOT, "examples", "sparse_schur_amd")


def build():
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "sparse_schur_amd"], env=env,
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
def test_cpp_schur_example_solves_to_the_bound(tmp_path):
    exe = build()
    res = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    K, nm = bordered_mass_system(8)
    n = K.shape[0]
    bound, e_lap = bound_for(K, K @ np.ones(n))
    print("sparse_schur_amd:", out, "bound", bound, "eta_lapack", e_lap)
    assert out["n"] == n and out["ns"] == n - nm and out["inertia"] == [nm, 0, 0]
    assert out["factor_info"] == 0
    assert out["eta"] <= bound, (out["eta"], bound)
