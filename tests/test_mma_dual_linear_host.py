"""CPU: the box form of the MMA dual solver (paropt_amd/csrc/mma_dual.cpp: lower <= lambda <= upper per component) on
the dual of the subproblem with linearised constraints, without a device.  The file is compiled together with
tools/mma_dual_linear_host.cpp (its own main; W, grad W and -hess W in plain host loops, the element roots by the
bracketed Newton iteration) under AddressSanitizer + UBSan and run on the linearised subproblems (use_true_mma = 0) the
oracle's MMA builds for three goldens at MMA iterations 0, 1 and 8 -- once with every constraint an inequality
(lambda in [0, gamma]) and once with the last one taken as an equality (lambda in [-gamma, gamma])."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mma_dual_linear_helpers import LINEAR_GOLDENS, PENALTY_GAMMA, oracle_linear_dual_mma
from mma_helpers import mma_options_from_case

TOL, MAX_EVALS = 1e-8, 200  # the defaults of mma_dual_tol / mma_dual_max_iterations
ITERATIONS = (0, 1, 8)
_NEGATIVE = {}  # golden -> an equality multiplier below zero was seen


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("mma_dual_linear") / "mma_dual_linear_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "paropt_amd", "csrc", "mma_dual.cpp"),
                           os.path.join(ROOT, "tools", "mma_dual_linear_host.cpp"), "-o", exe])
    return exe


def run_solver(exe, path, sp, lam0, gamma, tol, max_evals):
    lower, upper = sp.box(gamma)
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqd", sp.n, sp.m, max_evals, tol))
        for a in (lower, upper, lam0, sp.cons, sp.L, sp.U, sp.alpha, sp.beta, sp.p0, sp.q0, sp.xk, sp.A):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=120)
    report = out.stdout + out.stderr
    assert out.returncode == 0, report[-3000:]
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report
    lines = out.stdout.split("\n")
    status, evals, iters, pg, capped = lines[0].split()
    lam = np.array([float(v) for v in lines[1:1 + sp.m]])
    return lam, int(status), int(evals), int(iters), float(pg), int(capped)


@pytest.mark.parametrize("neq", [0, 1], ids=["inequalities", "last_is_equality"])
@pytest.mark.parametrize("name", LINEAR_GOLDENS)
def test_box_solver_matches_the_numpy_iteration(solver, tmp_path, name, neq):
    _, case = load_golden(name)
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    trace = oracle_linear_dual_mma(case, mopts, TOL, MAX_EVALS, max(ITERATIONS) + 1, neq=neq)
    if neq:
        _NEGATIVE[name] = any(t[2][-1] < 0.0 for t in trace)
    for k in ITERATIONS:
        sp, lam0, lam_np, status_np, evals_np = trace[k]
        lower, upper = sp.box(PENALTY_GAMMA)
        lam, status, evals, iters, pg, capped = run_solver(solver, str(tmp_path / ("sub%d.bin" % k)), sp, lam0,
                                                           PENALTY_GAMMA, TOL, MAX_EVALS)
        print("%s neq=%d @%d: %d evaluations (numpy %d), %d steps, max|pg| = %.2e, lambda = %s" % (
            name, neq, k, evals, evals_np, iters, pg, lam))
        assert status == 0 and status_np == 0
        assert pg <= TOL
        assert evals <= MAX_EVALS, evals
        assert capped == 0
        assert np.all(lam >= lower) and np.all(lam <= upper), lam
        assert np.all(np.abs(lam - lam_np) <= 1e-10 * np.maximum(1.0, np.abs(lam_np))), (lam, lam_np)
        if neq and lam[-1] < 0.0:
            _NEGATIVE[name] = True


def test_an_equality_multiplier_goes_negative():
    """Runs after the cases above (same module, definition order): among the equality runs a multiplier below zero
    occurs (within these nine MMA iterations on mma_convex_n200_c2_linearized: -1.24 at iteration 1)."""
    if set(_NEGATIVE) != set(LINEAR_GOLDENS):  # run alone: make the record
        for name in LINEAR_GOLDENS:
            _, case = load_golden(name)
            _, mopts = mma_options_from_case(case)
            mopts.pop("mma_max_iterations", None)
            trace = oracle_linear_dual_mma(case, mopts, TOL, MAX_EVALS, max(ITERATIONS) + 1, neq=1)
            _NEGATIVE[name] = any(t[2][-1] < 0.0 for t in trace)
    print(_NEGATIVE)
    assert any(_NEGATIVE.values()), _NEGATIVE


def test_a_start_below_the_box_is_clipped(solver, tmp_path):
    """A start below the lower end is clipped into the box first: the same solution as from the oracle's start."""
    _, case = load_golden("mma_convex_n300_c3")
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    sp, lam0, lam_np, _, _ = oracle_linear_dual_mma(case, mopts, TOL, MAX_EVALS, 1)[0]
    lam, status, evals, iters, pg, capped = run_solver(solver, str(tmp_path / "neg.bin"), sp, lam0 - 5.0,
                                                       PENALTY_GAMMA, TOL, MAX_EVALS)
    assert status == 0 and np.all(lam >= 0.0)
    assert np.all(np.abs(lam - lam_np) <= 1e-10 * np.maximum(1.0, np.abs(lam_np))), (lam, lam_np)
