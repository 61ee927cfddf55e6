"""Child process of tests/test_bottom_lds16.py: the developer switches are read once per context, so every value of
NDLQR_BOTTOM_LDS16 gets a fresh process. Prints one JSON line.

In the environment it is given (NDLQR_BOTTOM_LDS16, NDLQR_TREE=0, for the instances whose default is another schedule also
NDLQR_FUSE2=1 NDLQR_COMPACT1=1 NDLQR_PAIR1=1):
  python tests/lds16_support.py n m N [basic]
      the problems of tests/compact1_support.py at batch 3 -- `full`: two solves, return codes, schedule name, the
      read-outs (compact level-1 records, paired pass, 16 KB layout), solutions, device KKT residual of every member;
      `ranges`: MPC steps that compute a knot range alone (SOLN_ONLY); `kept`: a solver with KEEP_RECORDS in the same
      environment (basic: `full` alone)
  python tests/lds16_support.py resident n m N batch out.npy
      `batch` synthetic problems (seeds 1 .. batch), one solve, the solutions into out.npy
  python tests/lds16_support.py nonspd
      (12,4,16) x 3 with a non-positive R entry at knot 1, 5 or 3 of member 1 -- the knots of t0, of t1 and of the level-2
      separator m of the first workgroup: return code, failure count and per-problem words of each, and whether the
      healthy members equal a healthy solve bit for bit
  python tests/lds16_support.py nonspd n m N batch flags
      failure_support.run_case in this environment (NaN / +Inf in A_k and B_k of every separator, the weights, the
      unused data of the last knot, the isolated infinite pivot)
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
    return dict(schedule=bs.schedule(), compact1=bs.compact_level1(), paired=bs.level1_paired(), lds16=bs.bottom_lds16())


def shape(n, m, N, basic):
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
        out["ranges"].append(dict(k0=k0, nk=nk, rc=rc, got=np.array(got).tolist(), lds16=bs.bottom_lds16()))
    bs.close()
    if not basic:
        kb = R.BatchSolver(n, m, N, cs.BATCH, flags=R.FLAG_KEEP_RECORDS)
        kb.initialize_flat(*cs.flat(gs))
        out["kept"] = dict(rc=kb.solve(), sol=kb.solutions().tolist(), **state(kb))
        kb.close()
    return out


def resident(n, m, N, batch, path):
    gs = [R.generate_synthetic(n, m, N, 1 + p) for p in range(batch)]
    bs = R.BatchSolver(n, m, N, batch)
    bs.initialize_flat(*cs.flat(gs))
    out = dict(rc=bs.solve(), failures=bs.cholesky_failures(), **state(bs))
    np.save(path, bs.solutions())
    bs.close()
    return out


def non_spd():
    n, m, N, batch = 12, 4, 16, 3
    healthy = [R.generate_synthetic(n, m, N, 5 + p) for p in range(batch)]
    bs = R.BatchSolver(n, m, N, batch)
    bs.initialize_flat(*cs.flat(healthy))
    assert bs.solve() == 0
    base = bs.solutions().copy()
    out = []
    for knot in (1, 5, 3):
        gs = [{k: v.copy() for k, v in g.items()} for g in healthy]
        gs[1]["R"][knot, 1] = -1.0
        before = bs.cholesky_failure_counts().astype(np.int64)
        bs.initialize_flat(*cs.flat(gs))
        rc = bs.solve()
        sol = bs.solutions()
        grow = bs.cholesky_failure_counts().astype(np.int64) - before
        out.append(dict(knot=knot, rc=rc, failures=bs.cholesky_failures(), grow=grow.tolist(),
                        healthy_equal=bool(np.array_equal(sol[[0, 2]], base[[0, 2]])), **state(bs)))
    bs.close()
    return out


def main():
    a = sys.argv[1:]
    if a[0] == "nonspd" and len(a) > 1:
        n, m, N, batch = (int(v) for v in a[1:5])
        out = fs.run_case(R, n, m, N, batch, a[5])
        probe = R.BatchSolver(n, m, N, batch, flags=fs.flag_value(R, a[5]))  # (run_case does not report the new read-out)
        g = [R.generate_synthetic(n, m, N, 1 + p) for p in range(batch)]
        probe.initialize_flat(*cs.flat(g))
        probe.solve()
        out["lds16"] = probe.bottom_lds16()
        probe.close()
    elif a[0] == "nonspd":
        out = non_spd()
    elif a[0] == "resident":
        out = resident(*(int(v) for v in a[1:5]), a[5])
    else:
        out = shape(*(int(v) for v in a[:3]), a[3:4] == ["basic"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
