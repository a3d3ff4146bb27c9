"""examples/dense_quasidef_amd.cpp: a ParOptSparseProblem whose createQuasiDefMat() returns a user-written dense
solver with HIP kernels of its own, compiled outside the library.  The reference recorded the golden of this problem
(ipcsr_rosenbrock_n100_chain2) with a user-side dense solver too."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

EXE = os.path.join(ROOT, "examples", "dense_quasidef_amd")


def build():
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "dense_quasidef_amd"], env=env,
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
def test_cpp_user_dense_solver_matches_reference(tmp_path):
    exe = build()
    res = subprocess.run([exe, "nvars=100"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    g, _ = load_golden("ipcsr_rosenbrock_n100_chain2")
    np.testing.assert_array_equal(np.array([out["niter"], out["neval"], out["ngeval"]]), g["final/counters"])
    assert abs(out["fobj"] - g["final/fobj"][0]) <= 1e-6 * max(1.0, abs(g["final/fobj"][0]))
    np.testing.assert_allclose(out["xnorm"], g["final/norms"][0], rtol=1e-7)
    np.testing.assert_allclose([out["z0"], out["z1"]], g["final/z"], rtol=1e-5, atol=1e-6)
    assert out["factor_info"] == "dense user solver: 99 x 99"  # getFactorInfo routes to the user's object
    # The facade's trampolines dispatch the three- and four-argument apply exactly: the same problem with the same
    # options and a counting Python solver attached takes the same path through the library, call for call.
    import paropt_amd as pa

    ctx = pa.Context(0)
    prob = pa.SeparableProblem(ctx, "rosenbrock", 100).setChain(2, 1)  # the example's problem, built in
    counts = {"nfactor": 0, "napply3": 0, "napply4": 0}
    prob.setQuasiDefMat(CountingSolver(prob, counts))
    ip = pa.InteriorPoint(prob, {"qn_type": "bfgs", "qn_subspace_size": 10, "abs_res_tol": 1e-6,
                                 "barrier_strategy": "monotone", "max_major_iters": 150})
    ip.optimize()
    print("C++ example:", {k: out[k] for k in counts}, "python twin:", counts)
    assert tuple(ip.getIterationCounters()) == (out["niter"], out["neval"], out["ngeval"])
    assert {k: out[k] for k in counts} == counts
    ctx.close()


class CountingSolver:
    """dense numpy solver that counts its calls"""

    def __init__(self, problem, counts):
        self.problem, self.counts = problem, counts

    def factor(self, x, dinv, cdiag):
        from csr_helpers import dense_jacobian

        self.counts["nfactor"] += 1
        rowp, cols, data = self.problem.getSparseJacobianData()
        self.A, self.d = dense_jacobian(self.problem.nvars, rowp, cols, data), np.array(dinv)
        self.L = np.linalg.cholesky(np.diag(np.array(cdiag)) + (self.A * self.d) @ self.A.T)
        return 0

    def apply(self, bx, bw, yx, yw):
        self.counts["napply3" if bw is None else "napply4"] += 1
        rhs = (0.0 if bw is None else bw) - self.A @ (self.d * bx)
        yw[:] = np.linalg.solve(self.L.T, np.linalg.solve(self.L, rhs))
        yx[:] = self.d * (bx + self.A.T @ yw)
        return 0
