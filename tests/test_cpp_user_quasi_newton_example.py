"""examples/user_quasi_newton_amd.cpp: a limited-memory BFGS written by a user as a ParOptCompactQuasiNewton subclass
with HIP kernels of its own, compiled outside the library and attached through ParOptInteriorPoint::setQuasiNewton.
Its main() solves the workload of the golden ip_quadratic_n1000_c8_bfgs20."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

EXE = os.path.join(ROOT, "examples", "user_quasi_newton_amd")


def build():
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "user_quasi_newton_amd",
                           "libuser_quasi_newton.so"], env=env, stdout=subprocess.DEVNULL)
    return EXE


def test_example_builds_and_refuses_to_run_without_a_gpu():
    import torch

    exe = build()
    if torch.cuda.is_available():
        return  # covered by the gpu test
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 2 and "no MI355X available" in res.stderr


@pytest.mark.gpu
def test_cpp_user_quasi_newton_matches_reference(tmp_path):
    exe = build()
    res = subprocess.run([exe, "n=1000", "c=8", "m=20", "iters=150"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    g, _ = load_golden("ip_quadratic_n1000_c8_bfgs20")
    np.testing.assert_array_equal(np.array([out["niter"], out["neval"], out["ngeval"]]), g["final/counters"])
    assert abs(out["fobj"] - g["final/fobj"][0]) <= 1e-6 * max(1.0, abs(g["final/fobj"][0]))
    np.testing.assert_allclose(out["xnorm"], g["final/norms"][0], rtol=1e-7)
    assert 0.0 <= out["check_compact"] <= 1e-8
    assert out["nupdate"] > 0 and out["ncompact"] > out["nupdate"] and out["nmultadd"] == 0
    assert out["nmult"] == 1  # the consistency check alone: the solver evaluates B through the compact form
    # the same solve with the Python twin attached sees the same calls
    import paropt_amd as pa
    from user_qn_helpers import PVecLBFGS

    ctx = pa.Context(0)
    prob = pa.SeparableProblem(ctx, "quadratic", 1000, 8)
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": 20, "abs_res_tol": 1e-8,
                                 "starting_point_strategy": "affine_step", "barrier_strategy": "monotone",
                                 "start_affine_multiplier_min": 0.01, "penalty_gamma": 1000.0, "max_major_iters": 150,
                                 "write_output_frequency": 0})
    q = PVecLBFGS(ctx, 1000, 20)
    ip.setQuasiNewton(q)
    ip.optimize()
    assert tuple(ip.getIterationCounters()) == (out["niter"], out["neval"], out["ngeval"])
    # (the example's consistency check at the end asks for the compact form once more)
    assert (q.calls["reset"], q.calls["update"], q.calls["getCompactMat"]) == (out["nreset"], out["nupdate"],
                                                                              out["ncompact"] - 1)
    del ip, q, prob
    ctx.close()
