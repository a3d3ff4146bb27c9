"""CPU: the conservative inner iteration of the globally convergent MMA (paropt_amd/csrc/mma_gcmma.cpp on the dual
solver of mma_dual.cpp) without a device.  Both files are compiled with tools/mma_gcmma_host.cpp (its own main, every
n-sized sum in plain host loops) under AddressSanitizer + UBSan.  The program is run on the subproblems the oracle's
MMA reaches under the numpy restatement (tests/mma_gcmma_helpers.py) for two goldens at MMA iterations 0, 1 and 8; the
problem's own functions are evaluated here, by the oracle, at every trial point the program prints.  The start values
of rho, the number of raises and the final rho must be those of the restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mma_dual_helpers import PENALTY_GAMMA
from mma_gcmma_helpers import GCMMA_DEFAULTS, GCMMA_GOLDENS, fvals, oracle_gcmma
from mma_helpers import mma_options_from_case

DUAL_TOL, MAX_EVALS = 1e-9, 200
ITERATIONS = (0, 1, 8)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("mma_gcmma") / "mma_gcmma_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "paropt_amd", "csrc", "mma_gcmma.cpp"),
                           os.path.join(ROOT, "paropt_amd", "csrc", "mma_dual.cpp"),
                           os.path.join(ROOT, "tools", "mma_gcmma_host.cpp"), "-o", exe])
    return exe


def run_program(exe, path, it, grads, evaluate, opts, n_global):
    sp = it["sp"]
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqqq", sp.n, sp.m, MAX_EVALS, opts["mma_gcmma_max_inner"], n_global))
        f.write(struct.pack("<dddd", DUAL_TOL, opts["mma_gcmma_rho_init"], opts["mma_gcmma_rho_min"],
                            opts["mma_gcmma_tol"]))
        for a in (np.full(sp.m, PENALTY_GAMMA), it["lam0"], sp.b, it["fk"], sp.L, sp.U, sp.alpha, sp.beta, sp.p0,
                  sp.q0, it["xk"], grads[0], sp.p, sp.q, np.array(grads[1:])):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.Popen([exe, path], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)
    out = {"trials": 0}
    try:
        for line in proc.stdout:
            tag, *vals = line.split()
            if tag == "x":
                out["trials"] += 1
                out["x"] = np.array([float(v) for v in vals])
                f, c = evaluate(out["x"])
                proc.stdin.write(" ".join("%.17g" % v for v in fvals(f, c)) + "\n")
                proc.stdin.flush()
            elif tag == "done":
                out["raises"], out["capped"], out["evals"] = (int(v) for v in vals)
            else:
                out[tag] = np.array([float(v) for v in vals])
        proc.stdin.close()
        err = proc.stderr.read()
        rc = proc.wait(timeout=60)
    finally:
        proc.kill()
    assert rc == 0, err[-3000:]
    assert "AddressSanitizer" not in err and "runtime error" not in err and "LeakSanitizer" not in err, err[-3000:]
    return out


@pytest.mark.parametrize("name", GCMMA_GOLDENS)
def test_inner_iteration_matches_the_restatement(program, tmp_path, name):
    _, case = load_golden(name)
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    # the restatement's run, recording at each iteration what the program needs: the gradients at the expansion point
    from oracle import mma_oracle as mo
    from mma_dual_helpers import oracle_problem
    from mma_gcmma_helpers import gcmma_iteration

    mma = mo.MMA(oracle_problem(case), mopts)
    mma.initialize_subproblem(None)
    raised = 0
    for k in range(max(ITERATIONS) + 1):
        grads = [mma.g.copy()] + [a.copy() for a in mma.A]
        it = gcmma_iteration(mma, {}, DUAL_TOL, MAX_EVALS)
        if k in ITERATIONS:
            assert it["margin"] >= 1e-6, "a decision of the restatement sits on its threshold"

            def evaluate(x):
                _, f, c = mma.prob.eval_obj_con(x)
                return f, c

            got = run_program(program, str(tmp_path / ("sub%d.bin" % k)), it, grads, evaluate, GCMMA_DEFAULTS,
                              mma.prob.nlocal)
            print("%s @%d: %d raises (numpy %d), %d trials, rho0 %s -> rho %s" % (
                name, k, got["raises"], it["raises"], got["trials"], got["rho0"], got["rho"]))
            assert np.all(np.abs(got["rho0"] - it["rho0"]) <= 1e-12 * it["rho0"])
            assert got["raises"] == it["raises"] and got["capped"] == int(it["capped"])
            assert got["trials"] == it["trials"]
            assert np.all(np.abs(got["rho"] - it["rho"]) <= 1e-6 * it["rho"]), (got["rho"], it["rho"])
            assert np.all(np.abs(got["lam"] - it["lam"]) <= 1e-8 * np.maximum(1.0, np.abs(it["lam"])))
            assert np.abs(got["x"] - it["x"]).max() <= 1e-9
            raised += got["raises"]
        mma.zl, mma.zu, mma.z = it["zl"], it["zu"], it["lam"].copy()
        mma.initialize_subproblem(it["x"])
    if name == "mma_rosenbrock_n60":
        assert raised > 0  # (iteration 8 raises: the loop is exercised, not only its first trial)


def test_cap_takes_the_point_and_reports_it(program, tmp_path):
    """With mma_gcmma_max_inner = 1 an iteration that needs two raises ends after one, capped."""
    name = "mma_rosenbrock_n60"
    _, case = load_golden(name)
    _, mopts = mma_options_from_case(case)
    mopts.pop("mma_max_iterations", None)
    from oracle import mma_oracle as mo
    from mma_dual_helpers import oracle_problem
    from mma_gcmma_helpers import gcmma_iteration

    mma = mo.MMA(oracle_problem(case), mopts)
    mma.initialize_subproblem(None)
    for k in range(7):
        it = gcmma_iteration(mma, {}, DUAL_TOL, MAX_EVALS)
        if k < 6:
            mma.zl, mma.zu, mma.z = it["zl"], it["zu"], it["lam"].copy()
            mma.initialize_subproblem(it["x"])
    assert it["raises"] == 2
    grads = [mma.g.copy()] + [a.copy() for a in mma.A]

    def evaluate(x):
        _, f, c = mma.prob.eval_obj_con(x)
        return f, c

    got = run_program(program, str(tmp_path / "cap.bin"), it, grads, evaluate, dict(GCMMA_DEFAULTS, mma_gcmma_max_inner=1),
                      mma.prob.nlocal)
    assert got["raises"] == 1 and got["capped"] == 1 and got["trials"] == 2
