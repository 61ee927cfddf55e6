"""Cost and benefit of the infeasibility detection of the solve with linear inequality constraints
(ndlqr_BatchSetConstraintInfeasibilityDetection) at (12,4,256) x 1024: HIP-event times
(solve_ms()) of

  * one iteration with detection off and with a check every --every iterations, in the same process, for p = 4 and p = 8
    rows (the problems and rows of tools/lin_bench.py): constrained solves of 1 and of 41 iterations that converge nowhere
    (eps = 1e-300; every problem is feasible, so none is certified) on the remembered factorisation, the host reading
    nothing inside a run; iter_ms = (t41 - t1) / 40 as tools/lin_bench.py forms it -- 41 iterations hold the checks of
    iterations 10, 20, 30 and 40. Medians over --reps repetitions after --warmup, the spread (max - min) / median next to
    each; the off leg is taken again behind the on leg (the drift of the box within the run);
  * the headline case: the batch of p = 5 rows -- the input box |u| <= 0.5 and one dense row that is unbounded -- with
    --infeasible of its members made infeasible by family A of tests/lin_infeas_support.py on knot --knot (the dense row
    c'x_knot <= level, level a fifth of the reachable half-width below the smallest value c'x_knot takes inside the input
    box), a cold solve with the default settings, detection off and on: wall time, HIP-event time, iterations, statuses
    and the iteration at which each infeasible member ends; and the same two legs with the adaptive penalty of section
    3.19 considered every --adapt-every iterations (0: these two legs are left out).

JSON lines written to --out (profiles/lin_infeas_bench.jsonl), which every run replaces. --parent-lines FILE: the JSON
lines tools/lin_bench.py of the parent revision wrote on the same box in the same session; their iter_ms and its spread
are recorded next to this build's.
The algorithmic traffic of detection per check, per knot in doubles: lin_lambda_out twice (the iteration before and the
check: L^ n^2, lambda~ n in, lambda n out), lin_multipliers once (y in, mu out: 2 p) and lin_certify (A n^2, B n m, C p n,
D p m once; lambda, its copy and d: 3 n; y, mu_prev, lo, hi: 4 p).

    python tools/lin_infeas_bench.py [--every 10] [--infeasible 8] [--knot 8] [--adapt-every 25] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rslqr_amd as R  # noqa: E402
import lin_bench as LB  # noqa: E402

COPY_TBPS = 6.3  # achievable HBM rate of the MI355X (read + write bytes per second)
NAMES = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
n, m, N, BATCH = LB.N_, LB.M_, LB.HOR, LB.BATCH


def per_iteration(dense, p, rng, every, reps, warmup):
    C, D, hi = LB.rows(p, rng)
    bs = R.BatchSolver(n, m, N, BATCH)
    bs.initialize_flat_constrained(*[dense[k] for k in NAMES], C, D, -hi, hi)

    def run(k, ev):
        bs.set_constraint_infeasibility(ev)
        it, st = bs.solve_constrained(rho=1.0, max_iter=k, check_every=k, **LB.SET)
        assert (st == 2).all() and (it == k).all()
        return bs.solve_ms()
    run(1, 0)  # (factors)
    legs = {}
    for name, ev in (("off", 0), ("on", every), ("off_again", 0)):
        t1, _ = LB.median(lambda: run(1, ev), reps, warmup)
        t41, s41 = LB.median(lambda: run(41, ev), reps, warmup)
        legs[name] = dict(iter_ms=(t41 - t1) / 40.0, iter1_ms=t1, iter41_ms=t41, iter41_spread=s41)
    bs.close()
    knots = BATCH * N
    lam = 2 * (n * n + 2 * n)
    certify = n * n + n * m + p * n + p * m + 3 * n + 4 * p
    gb = 8.0 * knots * (lam + 2 * p + certify) / 1e9
    off, on = legs["off"]["iter_ms"], legs["on"]["iter_ms"]
    return dict(shape=[n, m, N], batch=BATCH, p=p, every=every, reps=reps, off=legs["off"], on=legs["on"], off_again=legs["off_again"],
                overhead_percent=100.0 * (on - off) / off, ms_per_check=(on - off) * every, GB_per_check=gb,
                estimate_ms_per_check_at_copy_rate=gb / COPY_TBPS)


def reach(g, c, knot):
    """(c0, G [knot, m]): c'x_knot = c0 + sum_k G_k . u_k over the inputs before `knot` (backward recursion on the row)"""
    A = g["A"].reshape(N, n, n).transpose(0, 2, 1)
    B = g["B"].reshape(N, m, n).transpose(0, 2, 1)
    row = c.copy()
    G = np.zeros((knot, m))
    c0 = 0.0
    for k in range(knot - 1, -1, -1):
        G[k] = row @ B[k]
        c0 += row @ g["d"][k]
        row = row @ A[k]
    return c0 + row @ g["x0"], G


def headline(dense, ninf, knot, every, adapt_every, ubar=0.5):
    p = m + 1
    C = np.zeros((BATCH, N, p, n))
    D = np.zeros((BATCH, N, p, m))
    D[:, :, :m, :] = np.eye(m)
    lo = np.full((BATCH, N, p), -np.inf)
    hi = np.full((BATCH, N, p), np.inf)
    lo[:, : N - 1, :m] = -ubar
    hi[:, : N - 1, :m] = ubar
    members = [int(b) for b in np.linspace(0, BATCH - 1, ninf).round()] if ninf > 0 else []
    rng = np.random.default_rng(41)
    for b in members:
        g = R.generate_synthetic(n, m, N, 1 + b % 8)  # (the problem tools/lin_bench.py puts at b)
        c = rng.standard_normal(n) / np.sqrt(n)
        c0, G = reach(g, c, knot)
        width = float(np.abs(G).sum()) * ubar
        C[b, knot, m] = c
        hi[b, knot, m] = (c0 - width) - 0.2 * width
    flat = lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(BATCH, N, -1)
    Cf, Df = flat(C), flat(D)
    out = dict(shape=[n, m, N], batch=BATCH, p=p, case="cold solve with the default settings", infeasible_members=len(members),
               bounded_knot=knot, every=every, adapt_every=adapt_every)
    legs = [("off", 0, 0), ("on", every, 0)]
    if adapt_every > 0:
        legs += [("off_adaptive", 0, adapt_every), ("on_adaptive", every, adapt_every)]
    for key, ev, ad in legs:
        bs = R.BatchSolver(n, m, N, BATCH)  # (a fresh solver: every leg pays its reduction and factorisation)
        bs.initialize_flat_constrained(*[dense[k] for k in NAMES], Cf, Df, lo, hi)
        bs.set_constraint_infeasibility(ev)
        bs.set_constraint_adaptation(ad)
        t0 = time.perf_counter()
        it, st = bs.solve_constrained()
        wall = (time.perf_counter() - t0) * 1e3
        out[key] = dict(wall_ms=round(wall, 2), solve_ms=round(bs.solve_ms(), 2), max_iterations=int(it.max()),
                        status_counts={str(s): int((st == s).sum()) for s in sorted(set(st.tolist()))},
                        status_of_the_infeasible_members=st[members].tolist(),
                        iterations_of_the_infeasible_members=it[members].tolist())
        bs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--infeasible", type=int, default=8)
    ap.add_argument("--knot", type=int, default=8, help="knot of the contradicting row of the infeasible members")
    ap.add_argument("--adapt-every", type=int, default=25, help="period of the adaptive penalty in the two extra legs of the headline case")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lin_infeas_bench.jsonl"))
    a = ap.parse_args()
    parent = {}
    if a.parent_lines:
        for line in open(a.parent_lines):
            if line.startswith("{"):
                d = json.loads(line)
                parent[d["p"]] = dict(iter_ms=d["iter_ms"], iter41_spread=d["iter41_spread"])
    _, dense = LB.problems()
    rng = np.random.default_rng(11)
    lines = []
    for p in (4, 8):
        line = per_iteration(dense, p, rng, a.every, a.reps, a.warmup)
        if p in parent:
            line["parent_lin_bench"] = parent[p]
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.infeasible > 0:
        lines.append(headline(dense, a.infeasible, a.knot, a.every, a.adapt_every))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
