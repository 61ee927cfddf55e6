"""Compact level-1 records (NDLQR_COMPACT1, DESIGN.md sections 2 and 3.4): the bottom launch keeps the packed Cholesky
factor of a level-1 separator alone, and rb_backsub_cols substitutes with it in three rounds. Each shape runs once per
value of the switch in a child process (tests/compact1_support.py; the switches are read when a context is created), at
the smallest horizons with a level-3 separator: N = 16 and 32 hold the first group (no left neighbour, knot 0 fixed), the
last group (no right neighbour) and interior groups. (12,4) and the padded (11,3) run the fused bottom launch
(bottom8_reduced_mc), (10,4) and (9,3) the four-knot one."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compact1_support as cs
from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9      # the bar of test_batch_fast_within_tolerance
AGREE_TOL = 1e-10   # knob on against knob off: one algorithm up to rounding
SHAPES = [(12, 4, 16), (12, 4, 32), (10, 4, 16), (10, 4, 32), (9, 3, 16), (9, 3, 32), (11, 3, 16), (11, 3, 32)]


@functools.lru_cache(maxsize=None)
def child(knob, *args):
    env = dict(os.environ, NDLQR_COMPACT1=knob, NDLQR_TREE="0")
    r = subprocess.run([sys.executable, os.path.abspath(cs.__file__)] + [str(a) for a in args], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (knob, args, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def oracle_solutions(oracle, n, m, N, r_scale=1.0):
    out = []
    for g in cs.problems(n, m, N, r_scale):
        prob = Problem(n, m, N, *[g[k] for k in cs.KEYS])
        out.append(oracle.solve(prob, 1)[0][: prob.nvars])
    return np.stack(out)


def rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_solution_and_residual(oracle, n, m, N):
    """Knob on: the solve reports compact level-1 records under the schedule name it had, every member is within 1e-9 of
    the oracle, the device KKT residual of every member is below 1e-9 max(1, |b|), and a second solve on the resident
    inputs gives the same answer."""
    full = child("1", n, m, N)["full"]
    assert full["rc"] == [0, 0] and full["second_solve_equal"] is True
    assert full["compact1"] is True
    assert full["schedule"] == ("reduced-fused2" if n >= 11 else "reduced"), full["schedule"]
    sol = np.array(full["sol"])
    err = rel(sol, oracle_solutions(oracle, n, m, N))
    print("error against the oracle", err)
    assert (err <= REL_TOL).all(), err
    res, bn = np.array(full["res"]), np.array(full["bn"])
    print("device KKT residual", res / np.maximum(1.0, bn))
    assert (res <= 1e-9 * np.maximum(1.0, bn)).all(), (res, bn)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_agrees_with_full_level1_records(n, m, N):
    """The same solve with NDLQR_COMPACT1=0 (full level-1 records, one substitution round) agrees to 1e-10 relative."""
    on, off = child("1", n, m, N)["full"], child("0", n, m, N, "basic")["full"]
    assert off["rc"] == [0, 0] and off["compact1"] is False and off["schedule"] == on["schedule"]
    diff = rel(np.array(on["sol"]), np.array(off["sol"]))
    print("knob on against knob off", diff)
    assert (diff <= AGREE_TOL).all(), diff


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_step_that_computes_a_knot_range_alone(n, m, N):
    """SOLN_ONLY steps -- knot 0, an interior tile, the last tile -- equal the same knots of the full solve bit for bit."""
    out = child("1", n, m, N)
    zb = 2 * n + m
    sol = np.array(out["full"]["sol"])
    Z = np.zeros((cs.BATCH, N * zb))
    Z[:, : sol.shape[1]] = sol
    Z = Z.reshape(cs.BATCH, N, zb)
    assert [(r["k0"], r["nk"]) for r in out["ranges"]] == cs.step_ranges(N)
    for r in out["ranges"]:
        assert r["rc"] == [0, 0]
        got = np.array(r["got"])
        want = Z[:, r["k0"]:r["k0"] + r["nk"], :]
        if r["k0"] + r["nk"] == N:  # (the last knot has no input: the slice carries padding there)
            got, want = got.copy(), want.copy()
            got[:, -1, 2 * n:] = 0.0
            want[:, -1, 2 * n:] = 0.0
        assert np.array_equal(got, want), (r["k0"], r["nk"])


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_kept_records_keep_their_format(oracle, n, m, N):
    """A solver created with KEEP_RECORDS in the same environment reports reduced-compact-records with full level-1
    records; its rhs-only re-solve and a multi-rhs call reproduce the full solve (1e-12, equal to rounding, like
    test_step_on_device_pointers) and the oracle."""
    kept = child("1", n, m, N)["kept"]
    assert kept["rc"] == [0, 0]
    assert kept["schedule"] == "reduced-compact-records" and kept["compact1"] is False
    ref = oracle_solutions(oracle, n, m, N)
    sol, resolve, multi = np.array(kept["sol"]), np.array(kept["resolve"]), np.array(kept["multi"])
    assert (rel(sol, ref) <= REL_TOL).all()
    assert (rel(resolve, sol) <= 1e-12).all(), rel(resolve, sol)
    assert (rel(multi[0], sol) <= 1e-12).all(), rel(multi[0], sol)
    rhs = {k: np.array(v) for k, v in kept["multi_rhs1"].items()}
    for p, g in enumerate(cs.problems(n, m, N)):
        prob = Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], rhs["q"][p], rhs["r"][p], rhs["d"][p], rhs["x0"][p])
        want = oracle.solve(prob, 1)[0][: prob.nvars]
        assert np.linalg.norm(multi[1, p] - want) / np.linalg.norm(want) <= REL_TOL


# Observed on MI355X at (12,4,32), R x 1e-4, batch 3, relative l2 error against refine(2) of a KEEP_RECORDS solve of the
# same run (eta 7.4e-12 -> 4.2e-17): knob on 6.6e-12 / 7.9e-12 / 8.8e-12, knob off 7.6e-12 / 7.4e-12 / 9.9e-12 -- a ratio of
# 0.9 to the largest knob-off error (profiles/compact1_ab.txt). The margin is not taken from that: it is the factor of 2
# that round 4's X-free change was held to (two substitutions with L_t in place of X = W'Y change which roundings occur,
# not their number).
WEAK_MARGIN = 2.0


def test_weak_input_costs():
    """The weak-input-cost family (R x 1e-4) at (12,4,32): the error of the knob-on solve against the refined solution is
    at most WEAK_MARGIN times the error of the knob-off solve of the same run."""
    on, off = child("1", 12, 4, 32)["weak"], child("0", 12, 4, 32, "basic")["weak"]
    assert on["rc"] == 0 and off["rc"] == 0 and on["truth_rc"] == 0
    assert on["compact1"] is True and off["compact1"] is False
    truth = np.array(on["truth"])
    assert on["eta"][1] <= on["eta"][0]
    e_on, e_off = rel(np.array(on["sol"]), truth), rel(np.array(off["sol"]), truth)
    print("weak R: error knob on", e_on, "knob off", e_off, "eta before / after refinement", on["eta"])
    assert (e_on <= WEAK_MARGIN * e_off.max()).all(), (e_on, e_off)


# (n, m, N, batch, flags, schedule, whether the switch decides about compact level-1 records)
FAILURE_CASES = [(12, 4, 16, 5, "none", "reduced-fused2", True),
                 (10, 4, 16, 5, "none", "reduced", True),
                 (9, 3, 16, 5, "none", "reduced", True),
                 (12, 4, 16, 5, "records", "reduced-compact-records", False)]


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("n,m,N,batch,flags,want,switched", FAILURE_CASES)
def test_failures_are_reported_per_problem(knob, n, m, N, batch, flags, want, switched):
    """tests/failure_support.py (run_case) with the knob on and off: a NaN or +Inf in A_k or B_k reaches no check of the
    weights, so what reports it is the flag of a Cholesky pass -- for odd k = 1 (mod 4) that of the level-1 pass, on compact
    records (knob on) or with the full record (knob off) -- and the per-problem words name the member: every separator,
    both bad members of a batch of 5, at least one flag per contaminated separator, the healthy members bit-equal to a
    healthy solve. A solver with KEEP_RECORDS keeps full level-1 records whatever the knob says and reports the same."""
    out = child(knob, "nonspd", n, m, N, batch, flags)
    print(knob, n, m, N, flags, out["schedule"], "solves", out["solves"], "isolated infinity", out.get("isolated"))
    assert out["schedule"] == want and out["compact1"] is (switched and knob == "1"), out
    assert not out["violations"], "%d violations, the first: %s" % (len(out["violations"]), out["violations"][:6])


def test_non_spd_block_is_reported():
    """A non-positive R entry -- at knot 3 as in test_gpu_parity.test_non_spd_block_is_reported, and at knot 1 -- makes the
    knob-on solve return NDLQR_ERR_NOT_SPD and count the failure. (What counts it is the check of the weights where the
    bottom launch stages them, not a Cholesky pass: test_failures_are_reported_per_problem holds those.)"""
    for case in child("1", "nonspd"):
        assert case["compact1"] is True
        assert case["rc"] == -3 and case["failures"] >= 1, case
