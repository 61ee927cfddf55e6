"""The paired fused bottom launch in 16 KB of LDS (NDLQR_BOTTOM_LDS16, DESIGN.md sections 3.3 and 7): the staged [A | B] at
pitch 17, the level-2 slot laid over the first wavefront's dead LDS, and the level >= 3 slots next to a workgroup stored
once -- the groups' contributions parked in LDS and added to m's Gram tiles -- instead of stored and then added to
atomically. Every delivering lane runs the arithmetic of the launch it replaces, so the solutions are expected BIT-EQUAL to
the knob off, which is what these tests hold it to. Each case runs once per value of the switch in a child process
(tests/lds16_support.py; the switches are read when a context is created). N = 16 has a first and a last workgroup per
problem and one level-3 slot; N = 32 adds interior workgroups. (12,4) and the padded (11,3) pair by default; (10,4) and
(9,3) get the paired launch with NDLQR_FUSE2=1 NDLQR_COMPACT1=1 NDLQR_PAIR1=1."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compact1_support as cs
import lds16_support as ls
from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9  # the bar of test_batch_fast_within_tolerance
SHAPES = [(12, 4, 16), (12, 4, 32), (11, 3, 16), (11, 3, 32)]
OTHER = [(10, 4, 16), (9, 3, 16)]


def forced(n):
    """(12,4) and what is padded into it run the paired fused launch by default."""
    return {} if n >= 11 else dict(NDLQR_FUSE2="1", NDLQR_COMPACT1="1", NDLQR_PAIR1="1")


@functools.lru_cache(maxsize=None)
def child(knob, *args):
    n = next((a for a in args if isinstance(a, int)), 12)  # (the block size: the first number)
    env = dict(os.environ, NDLQR_BOTTOM_LDS16=knob, NDLQR_TREE="0", **forced(n))
    r = subprocess.run([sys.executable, os.path.abspath(ls.__file__)] + [str(a) for a in args], env=env, capture_output=True,
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


def check_against_oracle_and_knob_off(oracle, n, m, N, applied):
    on, off = child("1", n, m, N)["full"], child("0", n, m, N, "basic")["full"]
    for full in (on, off):
        assert full["rc"] == [0, 0]
        assert full["paired"] is True and full["compact1"] is True and full["schedule"] == "reduced-fused2", full["schedule"]
        assert full["second_solve_equal"] is True  # (a stale overlaid slot would show here)
    assert off["lds16"] is False
    if applied is not None:
        assert on["lds16"] is applied
    a, b = np.array(on["sol"]), np.array(off["sol"])
    print("(%d,%d,%d) applied %s, knob on against knob off: bit-equal %s, relative difference %s"
          % (n, m, N, on["lds16"], np.array_equal(a, b), rel(a, b)))
    assert np.array_equal(a, b)
    err = rel(a, oracle_solutions(oracle, n, m, N))
    print("error against the oracle", err)
    assert (err <= REL_TOL).all(), err
    res, bn = np.array(on["res"]), np.array(on["bn"])
    print("device KKT residual", res / np.maximum(1.0, bn))
    assert (res <= 1e-9 * np.maximum(1.0, bn)).all(), (res, bn)
    assert np.array_equal(res, np.array(off["res"]))


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_bit_equal_to_knob_off_and_within_the_bars(oracle, n, m, N):
    """Knob on: the solve reports the 16 KB layout, the paired pass, compact level-1 records and the schedule name
    reduced-fused2; the solutions and device KKT residuals equal those of the knob off bit for bit; every member is within
    1e-9 of the oracle with a device KKT residual of at most 1e-9 max(1, |b|); a second solve on the resident inputs is
    bit-equal to the first."""
    check_against_oracle_and_knob_off(oracle, n, m, N, True)


@pytest.mark.parametrize("n,m,N", OTHER)
def test_other_instances(oracle, n, m, N):
    """(10,4) and (9,3) with the paired launch requested: the new layout with the same checks, or the read-out says "not
    applied" -- either way the results equal the knob off bit for bit."""
    check_against_oracle_and_knob_off(oracle, n, m, N, None)


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
        assert r["rc"] == [0, 0] and r["lds16"] is True
        got = np.array(r["got"])
        want = Z[:, r["k0"]:r["k0"] + r["nk"], :]
        if r["k0"] + r["nk"] == N:  # (the last knot has no input: the slice carries padding there)
            got, want = got.copy(), want.copy()
            got[:, -1, 2 * n:] = 0.0
            want[:, -1, 2 * n:] = 0.0
        assert np.array_equal(got, want), (r["k0"], r["nk"])


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_kept_records_solver_keeps_its_schedule(oracle, n, m, N):
    """A solver created with KEEP_RECORDS in the same environment keeps reduced-compact-records and reports the knob as
    not applied."""
    kept = child("1", n, m, N)["kept"]
    assert kept["rc"] == 0 and kept["schedule"] == "reduced-compact-records"
    assert kept["lds16"] is False and kept["paired"] is False
    assert (rel(np.array(kept["sol"]), oracle_solutions(oracle, n, m, N)) <= REL_TOL).all()


def test_resident_set(oracle, tmp_path):
    """(12,4,32) x 1024: 4096 workgroups, more than ten per CU -- every member bit-equal to the knob off, eight of them
    held to the oracle."""
    n, m, N, batch = 12, 4, 32, 1024
    sols = {}
    for knob in ("1", "0"):
        path = str(tmp_path / ("sol%s.npy" % knob))
        out = child(knob, "resident", n, m, N, batch, path)
        assert out["rc"] == 0 and out["failures"] == 0 and out["lds16"] is (knob == "1") and out["paired"] is True, out
        sols[knob] = np.load(path)
    assert sols["1"].shape == (batch, sols["0"].shape[1])
    differ = np.flatnonzero((sols["1"] != sols["0"]).any(axis=1))
    assert differ.size == 0, differ[:16]
    import rslqr_amd as R
    for p in range(0, batch, batch // 8):
        g = R.generate_synthetic(n, m, N, 1 + p)
        prob = Problem(n, m, N, *[g[k] for k in cs.KEYS])
        ref = oracle.solve(prob, 1)[0][: prob.nvars]
        err = np.linalg.norm(sols["1"][p] - ref) / np.linalg.norm(ref)
        assert err <= REL_TOL, (p, err)


def test_non_positive_weight_is_reported_as_with_the_knob_off():
    """A non-positive R entry at knot 1, 5 and 3 of member 1 of (12,4,16) x 3 -- they enter t0, t1 and m of the first
    workgroup: NDLQR_ERR_NOT_SPD, the word of member 1 alone grows, the healthy members equal a healthy solve -- and return
    code, failure count and per-problem words equal those of the knob off."""
    on, off = child("1", "nonspd"), child("0", "nonspd")
    assert [c["knot"] for c in on] == [1, 5, 3]
    for a, b in zip(on, off):
        assert a["lds16"] is True and b["lds16"] is False
        assert a["rc"] == -3 and a["failures"] >= 1 and a["grow"][0] == 0 and a["grow"][2] == 0 and a["grow"][1] >= 1, a
        assert a["healthy_equal"] is True
        assert {k: a[k] for k in ("rc", "failures", "grow", "healthy_equal")} == {k: b[k] for k in ("rc", "failures", "grow", "healthy_equal")}


@pytest.mark.parametrize("flags,want,applies", [("none", "reduced-fused2", True), ("records", "reduced-compact-records", False)])
def test_failures_are_reported_per_problem(flags, want, applies):
    """tests/failure_support.py (run_case) at (12,4,16) x 5 with the knob on and off: NaN / +Inf in A_k and B_k of every
    separator, the weights, the unused data of the last knot, the isolated infinite pivot -- no violation either way, the
    same number of solves and the same outcome of the isolated pivot. A solver with KEEP_RECORDS keeps its schedule."""
    on, off = child("1", "nonspd", 12, 4, 16, 5, flags), child("0", "nonspd", 12, 4, 16, 5, flags)
    for knob, out in (("1", on), ("0", off)):
        print(knob, flags, out["schedule"], "solves", out["solves"], "isolated infinity", out.get("isolated"))
        assert out["schedule"] == want and out["lds16"] is (applies and knob == "1"), out
        assert not out["violations"], "%d violations, the first: %s" % (len(out["violations"]), out["violations"][:6])
    assert on["solves"] == off["solves"]
    assert json.dumps(on.get("isolated"), sort_keys=True) == json.dumps(off.get("isolated"), sort_keys=True)
