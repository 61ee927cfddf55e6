"""Child process of tests/test_pair1_bottom.py: the developer switches are read once per context, so every value of
NDLQR_PAIR1 gets a fresh process.     python tests/pair1_support.py n m N [basic]      (prints one JSON line)

In the environment it is given (NDLQR_PAIR1, NDLQR_TREE=0, for the instances whose default is another schedule also
NDLQR_FUSE2=1 NDLQR_COMPACT1=1) it runs, at batch 3, the problems of tests/compact1_support.py:
  full     two solves: return codes, schedule name, whether the level-1 records were compact and the level-1 pass paired,
           solutions, device KKT residual of every member
  (basic: `full` and `weak` alone)
  ranges   MPC steps that compute a knot range alone (SOLN_ONLY): knot 0, an interior tile of eight knots (N >= 32), the
           last tile
  kept     a solver with KEEP_RECORDS in the same environment: schedule name, paired or not, full solve, rhs-only re-solve
  weak     (12,4,32) only: the weak-input-cost family (R x 1e-4), its solution, and the refined solution
  (python tests/pair1_support.py nonspd: (12,4,16), a non-positive R entry at knot 1 -- a weight of the knots of t0 of
   the first workgroup -- and at knot 5 -- of t1: return code and failure count of each. What flags them is the check of
   the weights where the bottom launch stages them (kernels_bottom_reduced.hpp:1065): with every other weight positive
   S-bar of t0 / t1 stays positive definite and the flag of the paired pass (lanes 0 and 32, :916-918) does not fire.
   python tests/pair1_support.py nonspd n m N batch flags: failure_support.run_case in this environment -- NaN / Inf in
   A_k and B_k of every separator, which only the Cholesky passes can flag, t0 and t1 of the paired pass included, the
   weights, the unused data of the last knot and the isolated infinite pivot -- as JSON: schedule name, compact, paired,
   the violations found)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import rslqr_amd as R  # noqa: E402

import compact1_support as cs  # noqa: E402
import failure_support as fs  # noqa: E402


def state(bs):
    return dict(schedule=bs.schedule(), compact1=bs.compact_level1(), paired=bs.level1_paired())


def non_spd():
    n, m, N = 12, 4, 16
    out = []
    for knot in (1, 5):
        g = R.generate_synthetic(n, m, N, 5)
        g["R"][knot, 1] = -1.0
        bs = R.BatchSolver(n, m, N, 1)
        bs.initialize_flat(*[g[k][None] for k in cs.KEYS])
        rc = bs.solve()
        out.append(dict(knot=knot, rc=rc, failures=bs.cholesky_failures(), **state(bs)))
        bs.close()
    print(json.dumps(out))


def kept_records(n, m, N, gs):
    kb = R.BatchSolver(n, m, N, cs.BATCH, flags=R.FLAG_KEEP_RECORDS)
    kb.initialize_flat(*cs.flat(gs))
    rc = [kb.solve()]
    kept = dict(sol=kb.solutions().tolist(), **state(kb))
    rc.append(kb.solve_rhs_only())
    kept["resolve"] = kb.solutions().tolist()
    kept["rc"] = rc
    kb.close()
    return kept


def weak_family(n, m, N):
    ws = cs.problems(n, m, N, 1e-4)
    wb = R.BatchSolver(n, m, N, cs.BATCH)
    wb.initialize_flat(*cs.flat(ws))
    rc = wb.solve()
    weak = dict(rc=rc, sol=wb.solutions().tolist(), **state(wb))
    wb.close()
    tb = R.BatchSolver(n, m, N, cs.BATCH, flags=R.FLAG_KEEP_RECORDS)
    tb.initialize_flat(*cs.flat(ws))
    weak["truth_rc"] = tb.solve()
    steps, eta0, eta1 = tb.refine(2)
    weak["truth"] = tb.solutions().tolist()
    weak["eta"] = [float(eta0.max()), float(eta1.max())]
    tb.close()
    return weak


def main():
    if sys.argv[1] == "nonspd" and len(sys.argv) > 2:
        n, m, N, batch = (int(a) for a in sys.argv[2:6])
        print(json.dumps(fs.run_case(R, n, m, N, batch, sys.argv[6])))
        return None
    if sys.argv[1] == "nonspd":
        return non_spd()
    n, m, N = (int(a) for a in sys.argv[1:4])
    basic = sys.argv[4:5] == ["basic"]
    out = {}
    gs = cs.problems(n, m, N)
    bs = R.BatchSolver(n, m, N, cs.BATCH)
    bs.initialize_flat(*cs.flat(gs))
    rc = [bs.solve()]
    first = bs.solutions().copy()
    rc.append(bs.solve())
    sol = bs.solutions()
    res, bn = bs.kkt_residuals()
    out["full"] = dict(rc=rc, sol=sol.tolist(), res=res.tolist(), bn=bn.tolist(),
                       second_solve_equal=bool(np.array_equal(first, sol)), **state(bs))
    x0 = R.pinned_empty((cs.BATCH, n))
    x0[...] = np.stack([g["x0"] for g in gs])
    out["ranges"] = []
    for k0, nk in ([] if basic else cs.step_ranges(N)):
        bs.set_step_selection(k0, nk, 7 | R.SOLN_ONLY)
        got = R.pinned_empty((cs.BATCH, nk, bs.slice_width(7)))
        rc = [bs.step_async(None, None, None, x0, got), bs.synchronize()]
        out["ranges"].append(dict(k0=k0, nk=nk, rc=rc, got=np.array(got).tolist(), paired=bs.level1_paired()))
    bs.close()
    if not basic:
        out["kept"] = kept_records(n, m, N, gs)
    if (n, m, N) == (12, 4, 32):
        out["weak"] = weak_family(n, m, N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
