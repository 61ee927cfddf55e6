"""The active-set polish on the host: the numpy restatement of polish_support.py, driving the CPU
oracle, against the direct solution of the active-set system (box_grad_support.active_forward); the seeds of the rounds
case and of the infeasible-guess case that the device tests reuse; and the sweep that fixes the default sigma. No GPU."""
import numpy as np
import pytest

import polish_support as ps
from box_grad_support import active_forward


@pytest.fixture(scope="module")
def solve(oracle):
    return ps.oracle_solve(oracle)


def start(ndlqr, oracle, solve, n, m, N, seed, eps, max_iter):
    prob = ps.synth(ndlqr, n, m, N, seed)
    b = ps.boxes(oracle, prob)
    rho = float(prob.Q.mean())
    return (prob, b, rho) + ps.admm_state(prob, solve, b, rho, 1.6, eps, max_iter)


# (7, 9, 16) runs zero-padded into a larger instance on the device: the padded-shape case
@pytest.mark.parametrize("n,m,N", ps.SWEEP_FAMILIES)
def test_polish_from_loose_admm_reaches_the_active_set_solution(ndlqr, oracle, solve, n, m, N):
    for seed in ps.SWEEP_SEEDS:
        prob, b, rho, z, v, y, it, st = start(ndlqr, oracle, solve, n, m, N, seed, 1e-3, 4000)
        assert st == 1
        o = ps.polish_reference(prob, solve, b, z, v, y, rho)
        assert o["status"] == 1 and o["steps"] >= 1, o
        zt, mt = active_forward(prob, o["codes"], *b)
        got, ref, was = (ps.stationarity(prob, *a, b) for a in ((o["z"], o["mu"]), (zt, mt), (z, rho * y)))
        print((n, m, N, seed), "ADMM iterations", it, "steps", o["steps"], "rounds", o["rounds"], got, ref["stationarity"])
        # exact feasibility and complementarity with a stationarity at the level of the direct solve: the KKT point of a
        # convex problem, so the set is the true one
        assert got["bounds"] == 0 and got["complementarity"] == 0
        assert got["stationarity"] <= 4 * ref["stationarity"]
        assert got["stationarity"] <= 1e-3 * was["stationarity"]
        # both are fp64 solutions of one system of condition well below 1e6
        assert np.abs(o["z"] - zt).max() <= 1e-10 * np.abs(zt).max()
        assert np.abs(o["mu"] - mt).max() <= 1e-10 * max(np.abs(mt).max(), 1.0)
        # what a warm start finds is the polished point
        assert np.array_equal(o["v"], ps.entries_of(prob, o["z"]))


def test_rounds_correct_a_wrong_active_set(ndlqr, oracle, solve):
    case = ps.ROUNDS_CASE
    rounds = []
    for seed in case["seeds"]:
        prob, b, rho, z, v, y, it, st = start(ndlqr, oracle, solve, *case["shape"], seed, 1e-300, case["admm_iters"])
        assert st == 2 and it == case["admm_iters"]
        o = ps.polish_reference(prob, solve, b, z, v, y, rho, max_rounds=case["max_rounds"])
        assert o["status"] == 1, (seed, o["status"], o["rounds"])
        rounds.append(o["rounds"])
        zt, mt = active_forward(prob, o["codes"], *b)
        got, ref = ps.stationarity(prob, o["z"], o["mu"], b), ps.stationarity(prob, zt, mt, b)
        assert got["bounds"] == 0 and got["complementarity"] == 0 and got["stationarity"] <= 4 * ref["stationarity"], got
    print("factorisations per problem", rounds)
    assert max(rounds) >= 3  # (the first factorisation plus at least two correction rounds)


def test_an_infeasible_guess_that_exhausts_the_rounds_keeps_the_admm_solution(ndlqr, oracle, solve):
    case = ps.INFEASIBLE_CASE
    for seed in case["seeds"]:
        prob, b, rho, z, v, y, it, st = start(ndlqr, oracle, solve, *case["shape"], seed, 1e-300, case["admm_iters"])
        for max_steps in (0, 1):
            o = ps.polish_reference(prob, solve, b, z, v, y, rho, max_steps=max_steps, max_rounds=case["max_rounds"])
            assert o["status"] == 2 and o["rounds"] == case["max_rounds"] + 1, (seed, o["status"], o["rounds"])
            assert np.array_equal(o["z"], z) and np.array_equal(o["v"], v) and np.array_equal(o["y"], y)
            assert np.array_equal(o["mu"], rho * y)


def test_a_non_finite_forward_is_left_alone(ndlqr, oracle, solve):
    prob, b, rho, z, v, y, it, st = start(ndlqr, oracle, solve, 3, 2, 8, 1, 1e-3, 4000)
    o = ps.polish_reference(prob, solve, b, z, v, y, rho, forward_status=3)
    assert o["status"] == 3 and o["steps"] == 0 and np.array_equal(o["z"], z)


def test_the_default_sigma_is_the_winner_of_the_sweep(ndlqr, oracle):
    rows = ps.sigma_sweep(ndlqr, oracle)
    for r in rows:
        print("sigma %.0e  total steps %3d  worst stationarity ratio %8.3f  all polished %s" % r)
    assert ps.sweep_winner(rows) == ps.DEFAULT_SIGMA
    import re, os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ndlqr.h")).read()
    assert float(re.search(r"#define NDLQR_POLISH_DEFAULT_SIGMA (\S+)", header).group(1)) == ps.DEFAULT_SIGMA


def test_the_adjoint_restatement_solves_the_active_set_adjoint(ndlqr, oracle, solve):
    from box_grad_support import active_adjoint
    for n, m, N in ps.SWEEP_FAMILIES:
        prob, b, rho, z, v, y, it, st = start(ndlqr, oracle, solve, n, m, N, 1, 1e-3, 4000)
        o = ps.polish_reference(prob, solve, b, z, v, y, rho)
        g = np.random.default_rng(N).standard_normal(prob.nvars)
        w, nu, steps, status = ps.polished_adjoint_reference(prob, solve, o["codes"], o["sig"], g)
        wr, nur = active_adjoint(prob, o["codes"], g)
        print((n, m, N), "adjoint steps", steps)
        assert status == 1 and steps >= 1
        assert (ps.entries_of(prob, w)[o["codes"] >= 2] == 0).all() and (nu[o["codes"] < 2] == 0).all()
        # both are fp64 solutions of one system of condition well below 1e6
        assert np.abs(w - wr).max() <= 1e-10 * np.abs(wr).max()
        assert np.abs(nu - nur).max() <= 1e-10 * max(np.abs(nur).max(), 1.0)
    w, nu, steps, status = ps.polished_adjoint_reference(prob, solve, o["codes"], o["sig"], g, polish_status=2)
    assert status == 2 and steps == 0 and not w.any() and not nu.any()
