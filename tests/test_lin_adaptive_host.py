"""The restatement of the per-problem adaptive penalty of the solve with linear inequality constraints
(lin_adaptive_support.admm_adaptive) on the 48 cases of lin_support.case: batch 3, shapes (6,3),
(12,4), (7,9), (20,5), horizons 2, 5, 8, 16; rho = 1, alpha = 1.6, eps 1e-8, period 25, max_iter 2000. No GPU."""
import numpy as np
import pytest

import cost_support as cs
import lin_adaptive_support as las
import lin_support as ls

CASES = [(n, m, N) for (n, m) in las.SHAPES for N in las.HORIZONS]


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 2), (7, 9, 8)])
def test_period_zero_is_the_fixed_penalty_iteration(n, m, N):
    for c in ls.case(n, m, N):
        got = las.admm_adaptive(c["p"], c["C"], c["D"], c["lo"], c["hi"], every=0)
        ref = c["ref"]
        assert got["iters"] == ref["iters"] and got["status"] == ref["status"] and got["rho"] == ls.RHO and not got["moves"]
        for k in ("z", "v", "y", "mu"):
            assert np.array_equal(got[k], ref[k]), k
        assert tuple(got["resid"]) == tuple(ref["resid"])


@pytest.mark.parametrize("n,m,N", CASES)
def test_moves_keep_the_multipliers(n, m, N):
    """mu = rho y is the same before and after every move the clamp did not cut: the step is a power of two"""
    for i, a in enumerate(las.case(n, m, N)):
        for mv in a["run"]["moves"]:
            if mv["clamped"]:
                continue
            assert np.array_equal(mv["mu_before"], mv["mu_after"]), (i, mv["it"], mv["rho"], mv["rho_new"])


@pytest.mark.parametrize("n,m,N", CASES)
def test_converged_cases_satisfy_the_kkt_conditions(n, m, N):
    for i, (c, a) in enumerate(zip(ls.case(n, m, N), las.case(n, m, N))):
        run = a["run"]
        if run["status"] != 1:
            continue
        bar = ls.kkt_bar(c["p"], c["C"], c["D"], run["z"], run["resid"], rho=run["rho"])
        got = ls.kkt_violation(c["p"], c["C"], c["D"], c["lo"], c["hi"], run["z"], run["mu"], bar["tol"])
        assert got["stationarity"] <= bar["stationarity"], (i, got, bar)
        assert got["feasibility"] <= bar["feasibility"], (i, got, bar)
        assert got["complementarity"] == 0.0, (i, got)


def test_table_undecided_cases_and_the_clamp():
    """The table of DESIGN.md section 3.19 (printed), the cap on undecided cases, and the seeds that do not converge at
    rho = 1: they do not converge adaptively either and end at the clamp rho_max with status 2."""
    undecided, stuck, stuck_fixed = [], [], []
    for n, m, N in CASES:
        for i, (c, a) in enumerate(zip(ls.case(n, m, N), las.case(n, m, N))):
            run, ref = a["run"], c["ref"]
            print("(%d,%d,%d) seed %d | fixed %4d status %d | adaptive %4d status %d | rho %-9g moves %d | margin %.2e%s"
                  % (n, m, N, i, ref["iters"], ref["status"], run["iters"], run["status"], run["rho"], len(run["moves"]),
                     a["margin"], "" if a["decided"] else "  UNDECIDED"))
            if not a["decided"]:
                undecided.append((n, m, N, i, a["margin"]))
            if ref["status"] == 2:
                stuck_fixed.append((n, m, N, i))
            if run["status"] == 2:
                stuck.append((n, m, N, i))
                assert run["rho"] == las.RHO_MAX and run["iters"] == 2000, (n, m, N, i, run["rho"])
    print("undecided:", undecided)
    assert len(undecided) <= las.UNDECIDED_CAP, undecided
    assert stuck == stuck_fixed and len(stuck) == 4, (stuck, stuck_fixed)
