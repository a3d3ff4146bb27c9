"""CPU: the dual of the MMA subproblem with the grouped sparse constraints kept in it (mma_dual_sparse_constraints =
"groups"), as the numpy restatement of tests/mma_dual_group_helpers.py, driving oracle/mma_oracle.MMA on the weighting
golden: every solve converges and every table row stays within the reference's own interior-point tolerance of the
golden table (measured 2.3e-5 relative in fobj, row 6; a factor of 4 is allowed: 1e-4)."""
import json
import os

import numpy as np

from conftest import load_golden
from mma_dual_group_helpers import WEIGHTING_GOLDEN, Groups, dual_eval_groups, group_solve, oracle_group_mma
from mma_dual_helpers import Subproblem, dual_eval
from mma_helpers import mma_options_from_case, parse_mma_table


def test_restatement_follows_the_golden_table():
    g, case = load_golden(WEIGHTING_GOLDEN)
    _, mopts = mma_options_from_case(case)
    niter = mopts["mma_max_iterations"]
    trace, solves = oracle_group_mma(case, mopts, 1e-8, 200, niter)
    ref = parse_mma_table(g["paropt_mma"])
    assert len(trace) == niter + 1 and len(ref) >= niter + 1
    for k, (status, evals, most, cap) in enumerate(solves):
        assert status == 0 and cap == 0, (k, status, evals, most, cap)
    rel = [abs(t["fobj"] - ref[k][1][0]) / max(1.0, abs(ref[k][1][0])) for k, t in enumerate(trace)]
    worst = int(np.argmax(rel))
    record = dict(golden=WEIGHTING_GOLDEN, rows=len(trace), worst_row=worst, worst_relative_fobj=rel[worst],
                  last_l1=trace[-1]["l1"], golden_last_l1=ref[niter][1][1],
                  most_evaluations_in_one_solve=max(s[1] for s in solves),
                  most_group_steps=max(s[2] for s in solves))
    print(json.dumps(record))
    out = os.environ.get("PAROPT_AMD_PROFILE_DIR")
    if out:  # the measurement of profiles/r12_mma_dual_groups_parity.json
        path = os.path.join(out, "r12_mma_dual_groups_parity.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old["host_restatement"] = record
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    for k, r in enumerate(rel):
        assert r <= 1e-4, (k, r, trace[k]["fobj"], ref[k][1][0])


def test_without_groups_the_restatement_is_the_plain_dual():
    rng = np.random.default_rng(3)
    n, m = 50, 3
    x0 = 5.0 + rng.random(n)
    L, U = x0 - 3.0, x0 + 3.0
    sp = Subproblem(L, U, x0 - 0.8, x0 + 0.9, 0.2 * rng.random(n) + 0.01, 0.2 * rng.random(n) + 0.01,
                    0.01 * rng.random((m, n)), 0.01 * rng.random((m, n)), rng.standard_normal(m))
    lam = np.array([0.0, 0.7, 2.0])
    W0, g0, H0 = dual_eval(sp, lam)
    for gr in (Groups(0, 1, 0, 0, -1.0, [], 0), Groups(5, 4, 3, 2, -1.0, np.full(5, 1e3), 5)):  # none / all inactive
        W, g, H, pt = dual_eval_groups(sp, lam, gr)
        assert np.all(pt["zw"] == 0.0)
        assert abs(W - W0) <= 1e-13 * abs(W0) and np.allclose(g, g0, rtol=1e-13, atol=0) and np.allclose(H, H0, rtol=1e-12)


def test_a_strict_group_meets_its_constraint():
    rng = np.random.default_rng(4)
    n = 12
    x0 = 5.0 + rng.random(n)
    sp = Subproblem(x0 - 3.0, x0 + 3.0, x0 - 0.8, x0 + 0.9, 0.2 * rng.random(n) + 0.01, 0.2 * rng.random(n) + 0.01,
                    np.zeros((1, n)), np.zeros((1, n)), [0.0])
    free = group_solve(sp, np.zeros(1), Groups(0, 1, 0, 0, -1.0, [], 0))["x"]
    # psi = -(sum x) + c: c a little under the unconstrained sums makes the constraints active
    gr = Groups(3, 4, 0, 0, -1.0, free.reshape(3, 4).sum(axis=1) - 0.3, 2)
    pt = group_solve(sp, np.zeros(1), gr)
    assert np.all(pt["zw"] > 0.0) and np.all(pt["zw"] < gr.gamma) and pt["cap"] == 0
    assert np.all(np.abs(pt["psi"]) <= 1e-13 * np.abs(gr.c))
    assert np.all(pt["x"] <= free) and np.all(pt["x"] >= sp.alpha)
