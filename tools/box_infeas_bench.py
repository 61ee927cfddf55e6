"""Cost and benefit of the infeasibility detection of the box-constrained solve (ndlqr_BatchSetInfeasibilityDetection;
DESIGN.md section 3.14): HIP-event times (ndlqr_BatchSolveTimeMs) of

  * one ADMM iteration with detection off and with a check every --every iterations, in the same process: a constrained
    solve of --iters iterations that converges nowhere (eps = 1e-300; every problem is feasible, so none is certified) on
    the remembered shifted factorisation, divided by --iters -- with shared input bounds, and with per-problem input and
    state bounds (the bounds of tools/box_bench.py),
  * the headline case: the same batch with --infeasible of its problems made infeasible (|u| <= half the mean |u| of the
    unconstrained solution, and one upper state bound of knot --knot placed a fifth of the reachable half-width below
    the smallest value that state reaches inside the input box: a limit the bounded inputs cannot recover early in the
    horizon), a cold solve at the default max_iter with detection off and on: wall time, HIP-event time, iterations and
    statuses.

Medians over --reps repetitions after --warmup; JSON lines appended to --out (profiles/box_infeas_bench.jsonl).
--parent-lines FILE: the JSON lines tools/box_bench.py of the parent revision printed on the same box in the same
session; their ms_per_iteration is recorded next to this build's.
The algorithmic traffic of detection per check: the three copies read and write z, y and rho once (2 x 8 B per entry), and
box_certify reads [A | B] once plus z, y, their copies and the bounds.

    python tools/box_infeas_bench.py [--shape 12,4,256,1024] [--iters 200] [--every 10] [--infeasible 8] [--knot 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rslqr_amd as R  # noqa: E402

COPY_TBPS = 6.3  # achievable HBM rate of the MI355X (read + write bytes per second)


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


def unconstrained(bs, n, m, N, batch):
    assert bs.solve() == 0
    Z = np.zeros((batch, N * (2 * n + m)))
    Z[:, : bs.nvars] = bs.solutions()
    Z = Z.reshape(batch, N, 2 * n + m)
    return Z[:, :, n:2 * n], Z[:, : N - 1, 2 * n:]


def reach_row(g, n, m, N, knot):
    """(c, G) of state 0 of `knot`: x_knot[0] = c + G . U over the stacked inputs (backward recursion on the row)"""
    A = g["A"].reshape(N, n, n).transpose(0, 2, 1)
    B = g["B"].reshape(N, m, n).transpose(0, 2, 1)
    row = np.zeros(n)
    row[0] = 1.0
    G = np.zeros((N, m))
    c = 0.0
    for k in range(knot - 1, -1, -1):
        G[k] = row @ B[k]
        c += row @ g["d"][k]
        row = row @ A[k]
    return c + row @ g["x0"], G


def per_iteration(bs, name, bounds, rho, iters, every, reps, warmup, n, m, N, batch):
    bs.set_bounds(*bounds)
    bs.set_box_infeasibility(0)
    bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)  # (factors)

    def timed(ev):
        def fn():
            bs.set_box_infeasibility(ev)
            it, st = bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
            assert (st == 2).all() and (it == iters).all()
            return bs.solve_ms()
        return fn

    off = median(timed(0), reps, warmup) / iters
    on = median(timed(every), reps, warmup) / iters
    off2 = median(timed(0), reps, 0) / iters  # (again behind the other leg: the drift of the box within the run)
    ne = batch * N
    copy_gb = 2 * 8 * ne * ((2 * n + m) + (n + m)) / 1e9
    certify_gb = 8 * ne * (n * (n + m) + 2 * n + 4 * (n + m) + n) / 1e9
    return {"shape": [n, m, N, batch], "bounds": name, "schedule": bs.schedule(), "every": every,
            "ms_per_iteration_off": round(off, 4), "ms_per_iteration_on": round(on, 4),
            "ms_per_iteration_off_again": round(off2, 4), "overhead_percent": round(100.0 * (on - off) / off, 2),
            "ms_per_check": round((on - off) * every, 4), "copies_GB_per_check": round(copy_gb, 4),
            "certify_GB_per_check": round(certify_gb, 4),
            "estimate_ms_per_check_at_copy_rate": round((copy_gb + certify_gb) / COPY_TBPS, 4), "iters_timed": iters, "reps": reps}


def headline(bs, n, m, N, batch, u, ninf, every, rho, knot):
    """8 infeasible members in the batch at the default max_iter, detection off | on"""
    ucap = 0.5 * np.abs(u).mean(axis=(0, 1))
    xhi = np.full((batch, N, n), np.inf)
    ulo = np.broadcast_to(-ucap, (batch, N, m)).copy()
    uhi = np.broadcast_to(ucap, (batch, N, m)).copy()
    members = [int(p) for p in np.linspace(0, batch - 1, ninf).round()] if ninf > 0 else []
    for p in members:
        g = R.generate_synthetic(n, m, N, 1 + p)
        ubar = 0.5 * float(np.abs(u[p]).mean())
        c, G = reach_row(g, n, m, N, knot)
        width = float(np.abs(G).sum()) * ubar
        ulo[p], uhi[p] = -ubar, ubar
        xhi[p, knot, 0] = (c - width) - 0.2 * width
    bs.set_bounds(None, xhi, ulo, uhi)
    out = {"shape": [n, m, N, batch], "case": "cold solve at the default max_iter", "infeasible_members": len(members),
           "bounded_knot": knot, "every": every, "rho": rho}
    for key, ev in (("off", 0), ("on", every)):
        bs.initialize_synthetic(1)  # (fresh inputs: both legs pay their factorisation)
        bs.set_bounds(None, xhi, ulo, uhi)
        bs.set_box_infeasibility(ev)
        t0 = time.perf_counter()
        it, st = bs.solve_box(rho=rho)
        wall = (time.perf_counter() - t0) * 1e3
        out[key] = {"wall_ms": round(wall, 2), "solve_ms": round(bs.solve_ms(), 2), "max_iterations": int(it.max()),
                    "status_counts": {str(s): int((st == s).sum()) for s in sorted(set(st.tolist()))},
                    "status_of_the_infeasible_members": st[members].tolist(),
                    "iterations_of_the_infeasible_members": it[members].tolist()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--infeasible", type=int, default=8)
    ap.add_argument("--knot", type=int, default=8, help="knot of the contradicting state bound of the infeasible members")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_infeas_bench.jsonl"))
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    parent = {}
    if a.parent_lines:
        for line in open(a.parent_lines):
            if line.startswith("{"):
                d = json.loads(line)
                parent[d["bounds"]] = d["ms_per_iteration"]
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_synthetic(1)
    x, u = unconstrained(bs, n, m, N, batch)
    ucap = 0.5 * np.abs(u).mean(axis=(0, 1))
    xcap = np.empty((batch, N, n))
    for p in range(batch):
        g = R.generate_synthetic(n, m, N, 1 + p)
        roll = np.zeros((N, n))
        roll[0] = g["x0"]
        for k in range(N - 1):
            roll[k + 1] = g["A"][k].reshape(n, n).T @ roll[k] + g["d"][k]
        xcap[p] = np.maximum(0.7 * np.abs(x[p, 1:]).max(axis=0), np.abs(roll))
    g0 = R.generate_synthetic(n, m, N, 1)
    configs = {"shared_input_bounds": (None, None, -ucap, ucap),
               "per_problem_input_and_state_bounds": (-xcap, xcap, np.broadcast_to(-ucap, (batch, N, m)),
                                                      np.broadcast_to(ucap, (batch, N, m)))}
    lines = []
    for name, b in configs.items():
        line = per_iteration(bs, name, b, float(g0["R"].mean()), a.iters, a.every, a.reps, a.warmup, n, m, N, batch)
        if name in parent:
            line["parent_ms_per_iteration"] = parent[name]
        lines.append(line)
    if a.infeasible > 0:
        lines.append(headline(bs, n, m, N, batch, u, a.infeasible, a.every, float(g0["Q"].mean()), a.knot))
    bs.close()
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
