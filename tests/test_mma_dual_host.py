"""CPU: the m-dimensional solver of the MMA subproblem's dual (paropt_amd/csrc/mma_dual.cpp) without a device.  The
file is compiled together with tools/mma_dual_host.cpp (its own main; W, grad W and -hess W evaluated in plain host
loops) under AddressSanitizer + UBSan and run on subproblems the oracle's MMA builds for three goldens at MMA
iterations 0, 1 and 8.  Iteration 0 is the start that breaks a plain projected Newton iteration: the point is
infeasible, every variable sits on a move limit, the dual Hessian is exactly zero and the gradient is not."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mma_dual_helpers import DUAL_GOLDENS, PENALTY_GAMMA, dual_eval, oracle_dual_mma
from mma_helpers import mma_options_from_case

TOL, MAX_EVALS = 1e-8, 200  # the defaults of mma_dual_tol / mma_dual_max_iterations
ITERATIONS = (0, 1, 8)


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("mma_dual") / "mma_dual_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "paropt_amd", "csrc", "mma_dual.cpp"),
                           os.path.join(ROOT, "tools", "mma_dual_host.cpp"), "-o", exe])
    return exe


def run_solver(exe, path, sp, lam0, gamma, tol, max_evals):
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqd", sp.n, sp.m, max_evals, tol))
        for a in (np.full(sp.m, gamma), lam0, sp.b, sp.L, sp.U, sp.alpha, sp.beta, sp.p0, sp.q0, sp.p, sp.q):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=120)
    report = out.stdout + out.stderr
    assert out.returncode == 0, report[-3000:]
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report
    lines = out.stdout.split("\n")
    status, evals, iters, pg = lines[0].split()
    lam = np.array([float(v) for v in lines[1:1 + sp.m]])
    return lam, int(status), int(evals), int(iters), float(pg)


@pytest.mark.parametrize("name", DUAL_GOLDENS)
def test_solver_matches_the_numpy_iteration(solver, tmp_path, name):
    _, case = load_golden(name)
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    trace = oracle_dual_mma(case, mopts, TOL, MAX_EVALS, max(ITERATIONS) + 1)
    for k in ITERATIONS:
        sp, lam0, lam_np, status_np, evals_np = trace[k]
        if k == 0:  # the infeasible start (on the quadratic and the Rosenbrock case with -hess W exactly zero)
            W, g, H = dual_eval(sp, lam0)
            assert (g > 0.0).any(), g
            print("%s @0: max|H| = %.3e, g = %s" % (name, np.abs(H).max(), g))
        lam, status, evals, iters, pg = run_solver(solver, str(tmp_path / ("sub%d.bin" % k)), sp, lam0,
                                                   PENALTY_GAMMA, TOL, MAX_EVALS)
        print("%s @%d: %d evaluations (numpy %d), %d steps, max|pg| = %.2e, lambda = %s" % (
            name, k, evals, evals_np, iters, pg, lam))
        assert status == 0 and status_np == 0
        assert evals <= 40, evals
        assert pg <= TOL
        assert np.all(np.abs(lam - lam_np) <= 1e-10 * np.maximum(1.0, np.abs(lam_np))), (lam, lam_np)


def test_solver_reports_giving_up(solver, tmp_path):
    """The evaluation cap ends the iteration with status 1 and the last max|pg|."""
    _, case = load_golden("mma_convex_n300_c3")
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    sp, lam0, _, _, evals_np = oracle_dual_mma(case, mopts, TOL, MAX_EVALS, 1)[0]
    assert evals_np > 3
    lam, status, evals, iters, pg = run_solver(solver, str(tmp_path / "cap.bin"), sp, lam0, PENALTY_GAMMA, TOL, 3)
    assert status == 1 and evals == 3 and pg > TOL
    assert np.all((lam >= 0.0) & (lam <= PENALTY_GAMMA))
