"""Child process of tests/test_compact1_records.py: the developer switches are read once per context, so every value of
NDLQR_COMPACT1 gets a fresh process.     python tests/compact1_support.py n m N [basic]      (prints one JSON line)

In the environment it is given (NDLQR_COMPACT1, NDLQR_TREE=0) it runs, at batch 3:
  full     two solves of the synthetic problems 7, 8, 9: return codes, schedule name, whether the level-1 records were
           compact, solutions, device KKT residual of every member
  (basic: `full` and `weak` alone)
  ranges   MPC steps that compute a knot range alone (SOLN_ONLY): knot 0, an interior tile of eight knots (N >= 32), the
           last tile -- every block of the slice
  kept     a solver with KEEP_RECORDS in the same environment: schedule name, full solve, rhs-only re-solve, and one
           multi-rhs call whose first right-hand side is the problems' own
  (python tests/compact1_support.py nonspd: a non-positive R entry at knot 3 -- the construction of
   test_non_spd_block_is_reported, N = 16 -- and at knot 1: return code and failure count of each. Both are flagged by the
   check of the weights where the bottom launch stages them (kernels_bottom_reduced.hpp:1065), not by a Cholesky pass: with
   every other weight positive the separator blocks stay positive definite.
   python tests/compact1_support.py nonspd n m N batch flags: failure_support.run_case in this environment -- NaN / Inf in
   A_k and B_k of every separator, which only the Cholesky passes can flag, the level-1 pass on compact records
   included -- as JSON: schedule name, compact, paired, the violations found)
  weak     (12,4,32) only: the weak-input-cost family (R x 1e-4), its solution, and the refined solution (refine(2) on a
           KEEP_RECORDS solve of the same problems) in the same process
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import rslqr_amd as R  # noqa: E402

BATCH = 3
SEED = 7
KEYS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def problems(n, m, N, r_scale=1.0):
    gs = [R.generate_synthetic(n, m, N, SEED + p) for p in range(BATCH)]
    for g in gs:
        g["R"] = g["R"] * r_scale
    return gs


def flat(gs):
    return [np.stack([g[k] for g in gs]) for k in KEYS]


def step_ranges(N):
    return [(0, 1)] + ([(8, 8)] if N >= 32 else []) + [(N - 8, 8)]


def non_spd():
    n, m, N = 12, 4, 16
    out = []
    for knot in (3, 1):
        g = R.generate_synthetic(n, m, N, 5)
        g["R"][knot, 1] = -1.0
        bs = R.BatchSolver(n, m, N, 1)
        bs.initialize_flat(*[g[k][None] for k in KEYS])
        rc = bs.solve()
        out.append(dict(knot=knot, rc=rc, failures=bs.cholesky_failures(), compact1=bs.compact_level1()))
        bs.close()
    print(json.dumps(out))


def main():
    if sys.argv[1] == "nonspd" and len(sys.argv) > 2:
        import failure_support as fs
        n, m, N, batch = (int(a) for a in sys.argv[2:6])
        print(json.dumps(fs.run_case(R, n, m, N, batch, sys.argv[6])))
        return None
    if sys.argv[1] == "nonspd":
        return non_spd()
    n, m, N = (int(a) for a in sys.argv[1:4])
    out = {}
    gs = problems(n, m, N)
    bs = R.BatchSolver(n, m, N, BATCH)
    bs.initialize_flat(*flat(gs))
    rc = [bs.solve()]
    first = bs.solutions().copy()
    rc.append(bs.solve())
    sol = bs.solutions()
    res, bn = bs.kkt_residuals()
    out["full"] = dict(rc=rc, schedule=bs.schedule(), compact1=bs.compact_level1(), sol=sol.tolist(), res=res.tolist(),
                       bn=bn.tolist(), second_solve_equal=bool(np.array_equal(first, sol)))
    basic = sys.argv[4:5] == ["basic"]
    x0 = R.pinned_empty((BATCH, n))
    x0[...] = np.stack([g["x0"] for g in gs])
    out["ranges"] = []
    for k0, nk in ([] if basic else step_ranges(N)):
        bs.set_step_selection(k0, nk, 7 | R.SOLN_ONLY)
        got = R.pinned_empty((BATCH, nk, bs.slice_width(7)))
        rc = [bs.step_async(None, None, None, x0, got), bs.synchronize()]
        out["ranges"].append(dict(k0=k0, nk=nk, rc=rc, got=np.array(got).tolist()))
    bs.close()

    if not basic:
        out["kept"] = kept_records(n, m, N, gs)
    if (n, m, N) == (12, 4, 32):
        out["weak"] = weak_family(n, m, N)
    print(json.dumps(out))


def kept_records(n, m, N, gs):
    kb = R.BatchSolver(n, m, N, BATCH, flags=R.FLAG_KEEP_RECORDS)
    kb.initialize_flat(*flat(gs))
    rc = [kb.solve()]
    kept = dict(schedule=kb.schedule(), compact1=kb.compact_level1(), sol=kb.solutions().tolist())
    rc.append(kb.solve_rhs_only())
    kept["resolve"] = kb.solutions().tolist()
    rng = np.random.default_rng(5)
    q = np.stack([np.stack([g["q"] for g in gs]), rng.standard_normal((BATCH, N, n))])
    r = np.stack([np.stack([g["r"] for g in gs]), rng.standard_normal((BATCH, N, m))])
    d = np.stack([np.stack([g["d"] for g in gs]), 0.1 * rng.standard_normal((BATCH, N, n))])
    x = np.stack([np.stack([g["x0"] for g in gs]), rng.standard_normal((BATCH, n))])
    kept["multi"] = kb.solve_multi_rhs(q, r, d, x).tolist()
    kept["multi_rhs1"] = dict(q=q[1].tolist(), r=r[1].tolist(), d=d[1].tolist(), x0=x[1].tolist())
    kept["rc"] = rc
    kb.close()
    return kept


def weak_family(n, m, N):
    ws = problems(n, m, N, 1e-4)
    wb = R.BatchSolver(n, m, N, BATCH)
    wb.initialize_flat(*flat(ws))
    rc = wb.solve()
    weak = dict(rc=rc, compact1=wb.compact_level1(), sol=wb.solutions().tolist())
    wb.close()
    tb = R.BatchSolver(n, m, N, BATCH, flags=R.FLAG_KEEP_RECORDS)
    tb.initialize_flat(*flat(ws))
    weak["truth_rc"] = tb.solve()
    steps, eta0, eta1 = tb.refine(2)
    weak["truth"] = tb.solutions().tolist()
    weak["eta"] = [float(eta0.max()), float(eta1.max())]
    tb.close()
    return weak


if __name__ == "__main__":
    main()
