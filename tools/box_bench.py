"""Box-constrained solve timings (ndlqr_SolveBatchBoxConstrained): HIP-event times (ndlqr_BatchSolveTimeMs) of

  * the rhs-only re-solve on the kept records (the floor of one ADMM iteration),
  * one ADMM iteration: a constrained solve of --iters iterations that converges nowhere (eps = 1e-300) on the remembered
    shifted factorisation, divided by --iters -- with shared input bounds, and with per-problem input and state bounds,
  * the iterations a cold constrained solve takes to eps = 1e-6 (the default) on the synthetic family,

medians over --reps repetitions after --warmup, one JSON line per bounds configuration. The bounds come from the
unconstrained solution: inputs clipped at half their mean magnitude per channel, states at 70 % of their largest
(widened where the trajectory of u = 0 needs more, so that every problem is feasible).
The update kernel's algorithmic traffic per iteration: per bounded entry z, v, y, the resident -q and lo, hi read and
v, y, the next right-hand side written (72 B; shared bounds are read from L2: 56 B of HBM traffic), per unbounded entry
lo and hi read. Its own time comes from a rocprofv3 --kernel-trace --stats run of this script (box_update).

--adapt-every K adds the per-problem adaptive penalty: for both bounds configurations a cold
fixed-penalty solve and a cold adaptive one (period K) of the same problems and bounds in this process, each after
fresh inputs so that both pay their first factorisation -- iterations, problems not converged, factorisations and
HIP-event time per constrained solve -- next to the time per iteration of adapt_every = 0, appended as JSON lines to
--out (profiles/box_adaptive_bench.jsonl).

    python tools/box_bench.py [--shape 12,4,256,1024] [--iters 200] [--reps 5] [--warmup 1] [--adapt-every 25]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rslqr_amd as R  # noqa: E402

COPY_TBPS = 6.3  # achievable HBM rate of the MI355X (read + write bytes per second)


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


def cold_solve(bs, bounds, **kw):
    """one cold constrained solve after fresh inputs (nothing remembered): its figures for the adaptive comparison"""
    bs.initialize_synthetic(1)
    bs.set_bounds(*bounds)
    f0 = bs.factor_count()
    it, st = bs.solve_box(max_iter=20000, **kw)
    ms = bs.solve_ms()
    pen = bs.box_penalties()
    return {"iterations": {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())},
            "not_converged": int((st != 1).sum()), "factorisations": int(bs.factor_count() - f0),
            "solve_ms": round(ms, 3), "ms_per_iteration_of_the_solve": round(ms / int(it.max()), 4),
            "rho_min_max": [float(pen.min()), float(pen.max())]}


def run(n, m, N, batch, iters, reps, warmup, adapt_every=0):
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_synthetic(1)
    assert bs.solve() == 0
    sol = bs.solutions()
    Z = np.zeros((batch, N * (2 * n + m)))
    Z[:, : bs.nvars] = sol
    Z = Z.reshape(batch, N, 2 * n + m)
    x, u = Z[:, :, n:2 * n], Z[:, : N - 1, 2 * n:]
    ucap = 0.5 * np.abs(u).mean(axis=(0, 1))
    # states: 70 % of their largest unconstrained magnitude, widened where the trajectory of u = 0 needs more (feasible)
    xcap = np.empty((batch, N, n))
    for p in range(batch):
        g = R.generate_synthetic(n, m, N, 1 + p)
        roll = np.zeros((N, n))
        roll[0] = g["x0"]
        for k in range(N - 1):
            roll[k + 1] = g["A"][k].reshape(n, n).T @ roll[k] + g["d"][k]
        xcap[p] = np.maximum(0.7 * np.abs(x[p, 1:]).max(axis=0), np.abs(roll))
    rho = float(R.generate_synthetic(n, m, N, 1)["R"].mean())  # (the penalty near the scale of diag R)

    def resolve():
        assert bs.solve_rhs_only() == 0
        return bs.solve_ms()

    resolve_ms = median(resolve, reps, warmup)
    schedule = bs.schedule()
    configs = {
        "shared_input_bounds": (None, None, -ucap, ucap),
        "per_problem_input_and_state_bounds": (-xcap, xcap,
                                               np.broadcast_to(-ucap, (batch, N, m)), np.broadcast_to(ucap, (batch, N, m)))}
    out = []
    for name, b in configs.items():
        bs.set_bounds(*b)
        # iterations to the default tolerance, cold
        it, st = bs.solve_box(rho=rho, max_iter=20000)
        cold_ms = bs.solve_ms()
        bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)  # (factored already)

        def fixed():
            bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
            return bs.solve_ms()

        per_iter = median(fixed, reps, warmup) / iters
        nb = batch * ((N - 1) * m + ((N - 1) * n if b[0] is not None else 0))
        ne = batch * N * (n + m)
        shared = b[0] is None
        gbytes = (nb * (72 - (16 if shared else 0)) + (0 if shared else (ne - nb) * 16)) / 1e9
        out.append({"shape": [n, m, N, batch], "bounds": name, "schedule": schedule, "rho": rho,
                    "rhs_only_resolve_ms": round(resolve_ms, 4), "ms_per_iteration": round(per_iter, 4),
                    "iteration_minus_resolve_ms": round(per_iter - resolve_ms, 4),
                    "update_algorithmic_GB": round(gbytes, 4),
                    "update_estimate_ms_at_copy_rate": round(gbytes / COPY_TBPS, 4),
                    "iterations_to_1e-6": {"max": int(it.max()), "median": float(np.median(it)), "min": int(it.min())},
                    "converged": int((st == 1).sum()), "cold_solve_ms": round(cold_ms, 3), "iters_timed": iters,
                    "reps": reps})
        if adapt_every > 0:
            out[-1]["adaptive"] = {"adapt_every": adapt_every, "fixed": cold_solve(bs, b, rho=rho),
                                   "adaptive": cold_solve(bs, b, rho=rho, adapt_every=adapt_every)}
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--adapt-every", type=int, default=0, help="also compare a cold fixed-penalty solve with a cold "
                    "adaptive one of this period and append the figures to --out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "box_adaptive_bench.jsonl"))
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    for line in run(n, m, N, batch, a.iters, a.reps, a.warmup, a.adapt_every):
        print(json.dumps(line), flush=True)
        if a.adapt_every > 0:
            keep = ("shape", "bounds", "schedule", "rho", "ms_per_iteration", "iters_timed", "reps", "adaptive")
            with open(a.out, "a") as f:
                f.write(json.dumps({k: line[k] for k in keep}) + "\n")


if __name__ == "__main__":
    main()
