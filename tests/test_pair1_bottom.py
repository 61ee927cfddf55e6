"""Paired level-1 pass of the fused bottom launch (NDLQR_PAIR1, DESIGN.md sections 3.3 and 3.4): with compact level-1
records the first wavefront of a workgroup of bottom8_reduced_mc takes the level-1 separators of both four-knot groups
through one Cholesky pass (t0 in lanes 0-31, t1 in lanes 32-63). Each shape runs once per value of the switch in a child
process (tests/pair1_support.py; the switches are read when a context is created). N = 16 has two workgroups per problem
-- the first without a left neighbour and with knot 0 fixed, the last without a right neighbour --, N = 32 adds
interior ones. (12,4) and the padded (11,3) run the fused launch by default; (10,4) and (9,3) -- two rows of S-bar to
zero in the Y tiles; odd n, the row loads that are not 16-byte ones, 25 - 6 idle panel lanes -- get it with
NDLQR_FUSE2=1 NDLQR_COMPACT1=1."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compact1_support as cs
import pair1_support as ps
from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9      # the bar of test_batch_fast_within_tolerance
AGREE_TOL = 1e-12   # knob on against knob off: equal to rounding (test_step_on_device_pointers)
SHAPES = [(12, 4, 16), (12, 4, 32), (11, 3, 16), (11, 3, 32), (10, 4, 16), (10, 4, 32), (9, 3, 16), (9, 3, 32)]


def forced(n):
    """(12,4) and what is padded into it run the fused launch with compact level-1 records by default."""
    return {} if n >= 11 else dict(NDLQR_FUSE2="1", NDLQR_COMPACT1="1")


@functools.lru_cache(maxsize=None)
def child(knob, *args):
    n = next((a for a in args if isinstance(a, int)), 12)  # (the block size: the first number)
    env = dict(os.environ, NDLQR_PAIR1=knob, NDLQR_TREE="0", **forced(n))
    r = subprocess.run([sys.executable, os.path.abspath(ps.__file__)] + [str(a) for a in args], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (knob, args, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def oracle_solutions(oracle, n, m, N):
    out = []
    for g in cs.problems(n, m, N):
        prob = Problem(n, m, N, *[g[k] for k in cs.KEYS])
        out.append(oracle.solve(prob, 1)[0][: prob.nvars])
    return np.stack(out)


def rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_solution_and_residual(oracle, n, m, N):
    """Knob on: the solve reports the paired pass, compact level-1 records and the schedule name reduced-fused2, every
    member is within 1e-9 of the oracle, the device KKT residual of every member is at most 1e-9 max(1, |b|), and a second
    solve on the resident inputs is bit-equal to the first."""
    full = child("1", n, m, N)["full"]
    assert full["rc"] == [0, 0]
    assert full["paired"] is True and full["compact1"] is True and full["schedule"] == "reduced-fused2", full["schedule"]
    assert full["second_solve_equal"] is True
    err = rel(np.array(full["sol"]), oracle_solutions(oracle, n, m, N))
    print("error against the oracle", err)
    assert (err <= REL_TOL).all(), err
    res, bn = np.array(full["res"]), np.array(full["bn"])
    print("device KKT residual", res / np.maximum(1.0, bn))
    assert (res <= 1e-9 * np.maximum(1.0, bn)).all(), (res, bn)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_agrees_with_one_pass_per_group(n, m, N):
    """The same solve with NDLQR_PAIR1=0 in the same build (one level-1 pass per wavefront) agrees to 1e-12 relative; by
    construction -- lane for lane the same arithmetic -- the two are bit-equal, which is printed."""
    on, off = child("1", n, m, N)["full"], child("0", n, m, N, "basic")["full"]
    assert off["rc"] == [0, 0] and off["paired"] is False
    assert off["compact1"] is True and off["schedule"] == on["schedule"]
    a, b = np.array(on["sol"]), np.array(off["sol"])
    diff = rel(a, b)
    print("(%d,%d,%d) knob on against knob off: relative difference %s, bit-equal %s" % (n, m, N, diff, np.array_equal(a, b)))
    assert (diff <= AGREE_TOL).all(), diff


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_step_that_computes_a_knot_range_alone(n, m, N):
    """SOLN_ONLY steps -- knot 0, an interior tile, the last tile -- equal the same knots of the full solve bit for bit:
    the records rb_backsub reads are the paired pass's."""
    out = child("1", n, m, N)
    zb = 2 * n + m
    sol = np.array(out["full"]["sol"])
    Z = np.zeros((cs.BATCH, N * zb))
    Z[:, : sol.shape[1]] = sol
    Z = Z.reshape(cs.BATCH, N, zb)
    assert [(r["k0"], r["nk"]) for r in out["ranges"]] == cs.step_ranges(N)
    for r in out["ranges"]:
        assert r["rc"] == [0, 0] and r["paired"] is True
        got = np.array(r["got"])
        want = Z[:, r["k0"]:r["k0"] + r["nk"], :]
        if r["k0"] + r["nk"] == N:  # (the last knot has no input: the slice carries padding there)
            got, want = got.copy(), want.copy()
            got[:, -1, 2 * n:] = 0.0
            want[:, -1, 2 * n:] = 0.0
        assert np.array_equal(got, want), (r["k0"], r["nk"])


@pytest.mark.parametrize("case", [0, 1])
def test_non_spd_block_is_reported(case):
    """A non-positive R entry at knot 1 (it enters t0: lanes 0-31 of the paired pass of the first workgroup) and at knot
    5 (t1: lanes 32-63): each returns NDLQR_ERR_NOT_SPD and counts at least one failure. (The staging of the weights
    flags a non-positive entry as well, so this holds the path as a whole, not the pass's own flag alone.)"""
    got = child("1", "nonspd")[case]
    assert got["knot"] == (1, 5)[case] and got["paired"] is True
    assert got["rc"] == -3 and got["failures"] >= 1, got


# (n, m, N, batch, flags, schedule, compact level-1 records and -- with the knob on -- the paired pass)
FAILURE_CASES = [(12, 4, 16, 5, "none", "reduced-fused2", True),
                 (10, 4, 16, 5, "none", "reduced-fused2", True),
                 (12, 4, 16, 5, "records", "reduced-compact-records", False)]


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("n,m,N,batch,flags,want,compact1", FAILURE_CASES)
def test_failures_are_reported_per_problem(knob, n, m, N, batch, flags, want, compact1):
    """tests/failure_support.py (run_case) with the knob on and off: a NaN or +Inf in A_k or B_k reaches no check of the
    weights, so what reports it is the flag of a Cholesky pass -- for k = 1, 0, 2 (mod 8) that of t0, lane 0 of the paired
    pass, for k = 5, 4, 6 that of t1, lane 32 -- and the per-problem words name the member: every separator, both bad
    members of a batch of 5, the count of flags at least one per contaminated separator, the healthy members bit-equal to
    a healthy solve. A solver with KEEP_RECORDS in the same environment does not pair and reports the same."""
    out = child(knob, "nonspd", n, m, N, batch, flags)
    print(knob, n, m, N, flags, out["schedule"], "solves", out["solves"], "isolated infinity", out.get("isolated"))
    assert out["schedule"] == want and out["compact1"] is compact1 and out["paired"] is (compact1 and knob == "1"), out
    assert not out["violations"], "%d violations, the first: %s" % (len(out["violations"]), out["violations"][:6])


# The paired pass is, lane for lane, the arithmetic of the pass it replaces, so the two errors are expected to be equal.
# The margin is that of test_compact1_records.test_weak_input_costs, for the same reason: a factor of 2 allows for which
# roundings occur, not for more of them.
WEAK_MARGIN = 2.0


def test_weak_input_costs():
    """The weak-input-cost family (R x 1e-4) at (12,4,32): the error of the knob-on solve against the refined solution is
    at most WEAK_MARGIN times the largest error of the knob-off solve of the same run."""
    on, off = child("1", 12, 4, 32)["weak"], child("0", 12, 4, 32, "basic")["weak"]
    assert on["rc"] == 0 and off["rc"] == 0 and on["truth_rc"] == 0
    assert on["paired"] is True and off["paired"] is False and on["compact1"] is True and off["compact1"] is True
    truth = np.array(on["truth"])
    assert on["eta"][1] <= on["eta"][0]
    e_on, e_off = rel(np.array(on["sol"]), truth), rel(np.array(off["sol"]), truth)
    print("weak R: error knob on", e_on, "knob off", e_off, "eta before / after refinement", on["eta"])
    assert (e_on <= WEAK_MARGIN * e_off.max()).all(), (e_on, e_off)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_kept_records_solver_is_not_paired(oracle, n, m, N):
    """A solver created with KEEP_RECORDS in the same environment keeps its schedule (full level-1 records, no paired
    pass) and solves as before: within 1e-9 of the oracle, its rhs-only re-solve equal to rounding (1e-12)."""
    kept = child("1", n, m, N)["kept"]
    assert kept["rc"] == [0, 0]
    assert kept["paired"] is False and kept["compact1"] is False and kept["schedule"] == "reduced-compact-records"
    sol, resolve = np.array(kept["sol"]), np.array(kept["resolve"])
    assert (rel(sol, oracle_solutions(oracle, n, m, N)) <= REL_TOL).all()
    assert (rel(resolve, sol) <= 1e-12).all(), rel(resolve, sol)
