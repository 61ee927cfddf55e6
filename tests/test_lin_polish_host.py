"""The active-set polish of the solve with linear inequality rows on the host: the numpy
restatement of lin_polish_support.py against lin_support.kkt_violation and the direct solution of the bordered active-set
system (lin_polish_support.active_direct), on lin_support.case for the shapes (6,3), (12,4), (7,9), (20,5) x horizons 2, 5,
8, 16, each problem from the restatement's ADMM at eps = 1e-3; selector rows on a diagonal cost against the box polish of
polish_support.py; the sweep behind the default sigma; the cap on the problems that may stay unpolished. No GPU.

Bars. The restatement's norms are float64 evaluations of rows that are chains of at most k = 2n + m + p + 2 products: each
is within k eps of the sum of its absolute terms, at most k^2 eps max|K, G| max|z, mu| (`rounding`). The KKT conditions
evaluated in longdouble therefore hold to the final norm (feasibility and the complementarity distance: the final |r_c|)
plus that. Against active_direct: both (z, mu) solve one bordered system, so their difference is at most the norm of its
inverse times the sum of their residuals, both evaluated in longdouble.

Measured, sigma sweep from ADMM at 1e-3 over the 48 problems (total accepted steps, worst final stationarity over that of
active_direct on the same set, both in longdouble; problems ending as status 1):
    sigma 1e2: 322 steps, 1.32, 46     1e3: 249, 1.32, 45     1e4: 198, 1.00, 45     1e5: 161, 1.02, 45
    sigma 1e6: 138 steps, 1.23, 45     1e7: 123, 1.23, 45     1e8: 112, 1.00, 45
Every sigma is within section 3.13's 4 x; the fewest steps are 1e8's: the default. (With rows accumulated in plain float64
the worst ratios were 4.8 - 7.6 and none was: the residual rows are accumulated in double-double on the device, in
longdouble rounded once here.)"""
import os
import re
import warnings

import numpy as np
import pytest

import cost_support as cs
import lin_polish_support as lp
import lin_support as ls
import polish_support as ps

EPS = np.finfo(float).eps


def rounding(c, z, mu):
    """k^2 eps max|K, G| max|z, mu|: what a float64 evaluation of a residual row may be off by (module docstring)"""
    p = c["p"]
    n, m, N = cs.dims(p)
    k = 2 * n + m + c["C"].shape[1] + 2
    big = max(1.0, max(float(np.abs(p[a]).max()) for a in ("A", "B", "Q", "H", "R")), float(np.abs(c["C"]).max()),
              float(np.abs(c["D"]).max()))
    return k * k * EPS * big * max(float(np.abs(z).max()), float(np.abs(mu).max()), 1.0)


def bordered_inverse_norm(c, codes):
    """the infinity norm of the inverse of [[K, G_A'], [G_A, 0]] (None: singular, as active_direct)"""
    p = c["p"]
    n, m, N = cs.dims(p)
    K, _ = cs.dense_kkt(p)
    rows = []
    zb = 2 * n + m
    for k in range(N):
        for r in range(c["C"].shape[1]):
            if codes[k, r] >= 2:
                g = np.zeros(K.shape[0])
                g[k * zb + n:k * zb + 2 * n] = c["C"][k, r]
                if k < N - 1:
                    g[k * zb + 2 * n:k * zb + 2 * n + m] = c["D"][k, r]
                rows.append(g)
    G = np.array(rows).reshape(len(rows), K.shape[0])
    big = np.block([[K, G.T], [G, np.zeros((len(rows), len(rows)))]])
    return float(np.abs(np.linalg.inv(big)).sum(axis=1).max())


def active_residual_ld(c, codes, z, mu):
    """max(|K z - b + G_A' mu|, |G_A z - c_A|) in longdouble"""
    p = c["p"]
    w = ls.rows_of(p, c["C"], c["D"], np.asarray(z, dtype=np.longdouble))
    bound = np.where(codes == 3, c["hi"], np.where(codes == 2, c["lo"], 0.0))
    rc = float(np.abs(np.where(codes >= 2, w - bound, 0)).max())
    return max(lp.stationarity_ld(p, c["C"], c["D"], z, mu), rc)


@pytest.mark.parametrize("n,m,N", lp.CASES)
def test_polished_problems_satisfy_the_kkt_conditions_and_agree_with_the_direct_solve(n, m, N):
    for i, c in enumerate(ls.case(n, m, N)):
        a = lp.admm_start(n, m, N)[i]
        o = lp.polish_case(n, m, N, i)
        print((n, m, N), i, "ADMM", a["iters"], a["status"], "polish status", o["status"], "steps", o["steps"], "rounds", o["rounds"],
              "norms", [["%.1e" % float(x) for x in r] for r in o["norms"]])
        if o["status"] != 1:
            # left alone: what the constrained solve delivered
            assert np.array_equal(o["z"], a["z"]) and np.array_equal(o["v"], a["v"]) and np.array_equal(o["y"], a["y"])
            continue
        p, C, D, lo, hi = c["p"], c["C"], c["D"], c["lo"], c["hi"]
        assert o["steps"] >= 1
        norm = float(o["norm"])
        round_ = rounding(c, o["z"], o["mu"])
        tol = float(o["rc"]) + round_
        got = ls.kkt_violation(p, C, D, lo, hi, o["z"], o["mu"], tol)
        assert got["stationarity"] <= norm + round_, (got, norm, round_)
        assert got["feasibility"] <= tol, (got, tol)
        assert got["complementarity"] == 0.0, got
        # multiplier signs, exact
        assert (o["mu"][o["codes"] == 3] >= 0).all() and (o["mu"][o["codes"] == 2] <= 0).all() and not o["mu"][o["codes"] < 2].any()
        # what a warm start finds is the polished point
        w = ls.rows_of(p, C, D, o["z"])
        M = lp.bounded(lo, hi)
        assert np.array_equal(o["v"][M], np.clip(w, lo, hi)[M]) and np.array_equal(o["y"][M], (o["mu"] / ls.RHO)[M])
        direct = lp.active_direct(p, C, D, lo, hi, o["codes"])
        if direct is None:
            print("   dependent active rows: no direct solve to compare with")
            continue
        zt, mt = direct
        bar = bordered_inverse_norm(c, o["codes"]) * (active_residual_ld(c, o["codes"], o["z"], o["mu"]) +
                                                      active_residual_ld(c, o["codes"], zt, mt))
        bar = 1.01 * bar + 4 * EPS * max(float(np.abs(zt).max()), float(np.abs(mt).max()))
        err = max(float(np.abs(o["z"] - zt).max()), float(np.abs(o["mu"] - mt).max()))
        print("   against the direct solve %.2e (bar %.2e)" % (err, bar))
        assert err <= bar, (err, bar)


def test_the_cap_on_unpolished_problems_holds_at_the_default():
    status = [lp.polish_case(n, m, N, i)["status"] for (n, m, N) in lp.CASES for i in range(cs.BATCH)]
    print("status 1:", status.count(1), "of", len(status), "| 2:", status.count(2), "| 3:", status.count(3))
    assert len(status) == 48 and status.count(1) >= lp.STATUS1_CAP


def test_some_first_sets_are_wrong_and_the_rounds_correct_them():
    rounds = [lp.polish_case(n, m, N, i) for (n, m, N) in lp.CASES for i in range(cs.BATCH)]
    assert any(o["rounds"] >= 2 and o["status"] == 1 for o in rounds)


def test_a_non_finite_and_an_infeasible_forward_are_left_alone():
    c, a = ls.case(6, 3, 5)[0], lp.admm_start(6, 3, 5)[0]
    for fst, want in ((3, 3), (4, 2)):
        o = lp.polish_reference(c["p"], c["C"], c["D"], c["lo"], c["hi"], a["z"], a["v"], a["y"], ls.RHO, forward_status=fst)
        assert o["status"] == want and o["steps"] == 0 and o["rounds"] == 0
        assert np.array_equal(o["z"], a["z"]) and np.array_equal(o["v"], a["v"]) and np.array_equal(o["y"], a["y"])


@pytest.mark.parametrize("n,m,N", ps.SWEEP_FAMILIES)
def test_selector_rows_on_a_diagonal_cost_reproduce_the_box_polish(ndlqr, oracle, n, m, N):
    """Codes, statuses and steps of polish_support.polish_reference, z and mu to the residual floor (measured: steps 2 | 2
    on five of the six problems, 4 | 4 over two rounds on (7,9,16) seed 2; the norms agree from the second slot on)."""
    solve = ps.oracle_solve(oracle)
    steps = []
    for seed in ps.SWEEP_SEEDS:
        prob = ps.synth(ndlqr, n, m, N, seed)
        pd, _, _ = cs.diagonal_problem(n, m, N, seed)
        b = ps.boxes(oracle, prob)
        rho = float(prob.Q.mean())
        z, v, y, it, st = ps.admm_state(prob, solve, b, rho, 1.6, 1e-3, 4000)
        box = ps.polish_reference(prob, solve, b, z, v, y, rho)
        C, D, lo, hi = ls.selector_rows(n, m, N, *b)
        row = lp.polish_reference(pd, C, D, lo, hi, z, v, y, rho, sigma=ps.DEFAULT_SIGMA)
        print((n, m, N, seed), "box: status", box["status"], "steps", box["steps"], "rounds", box["rounds"], "| rows: status",
              row["status"], "steps", row["steps"], "rounds", row["rounds"], "norms",
              [["%.1e" % float(x) for x in r] for r in row["norms"]])
        assert row["sig"] == box["sig"]  # (g = 1 for selector rows)
        assert np.array_equal(row["codes"], box["codes"])
        assert row["status"] == box["status"] == 1
        steps.append((seed, box["steps"], row["steps"]))
        # both are fp64 solutions of one system of condition well below 1e6 (test_polish_host.py)
        assert np.abs(row["z"] - box["z"]).max() <= 1e-10 * np.abs(box["z"]).max()
        assert np.abs(row["mu"] - box["mu"]).max() <= 1e-10 * max(np.abs(box["mu"]).max(), 1.0)
    assert all(b == r for _, b, r in steps), steps


def test_the_default_sigma_is_the_winner_of_the_sweep():
    """Section 3.13's rule: the fewest total steps among the values whose worst stationarity is within 4 x that of
    active_direct (the table is in the module docstring)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows = lp.sigma_sweep()
    for r in rows:
        print("sigma %.0e  total steps %3d  worst stationarity ratio %8.3f  at least %d polished %s (%d)"
              % (r[0], r[1], r[2], lp.STATUS1_CAP, r[3], r[4]))
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ndlqr.h")).read()
    assert float(re.search(r"#define NDLQR_LIN_POLISH_DEFAULT_SIGMA (\S+)", header).group(1)) == lp.DEFAULT_SIGMA
    assert lp.sweep_winner(rows) == lp.DEFAULT_SIGMA
