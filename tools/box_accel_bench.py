"""Anderson acceleration of the box-constrained solve (ndlqr_BatchSetBoxAcceleration): what an
iteration costs and how many a solve takes, with memory 0 (box_update, the plain algorithm), 5 and 10 in one process.

For shared input bounds and for per-problem input and state bounds (the bounds and the penalty, mean diag R, of
tools/box_bench.py), with a fixed penalty and with adapt_every = 25, per memory:

  * ms per iteration: a constrained solve of --iters iterations that converges nowhere (eps = 1e-300) on the remembered
    shifted factorisation, divided by --iters; the median of --reps repetitions after --warmup (fixed penalty only: an
    adapting solve factors in between);
  * a cold solve to eps = 1e-6 after fresh inputs: iterations as min / median / max, problems not converged, the
    HIP-event time of the solve, accepted and rejected steps summed over the batch.

HIP-event times (ndlqr_BatchSolveTimeMs). The ring traffic the new kernel adds per bounded entry and iteration: the
g entries kept and the t entries of the step read, t and g written, the plain v+, y+ saved and read back -- about
2 (mem + 1) + 2 doubles. One JSON line per bounds configuration, printed and appended to --out.

    python tools/box_accel_bench.py [--shape 12,4,256,1024] [--iters 200] [--reps 5] [--warmup 1] [--mems 0,5,10]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rslqr_amd as R  # noqa: E402

COPY_TBPS = 6.3  # achievable HBM rate of the MI355X (read + write bytes per second)
ADAPT = 25


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


def cold_solve(bs, bounds, mem, **kw):
    bs.initialize_synthetic(1)
    bs.set_bounds(*bounds)
    bs.set_box_acceleration(mem)
    it, st = bs.solve_box(max_iter=20000, **kw)
    ms = bs.solve_ms()
    out = {"iterations": {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())},
           "not_converged": int((st != 1).sum()), "solve_ms": round(ms, 3),
           "ms_per_iteration_of_the_solve": round(ms / int(it.max()), 4)}
    if mem > 0:
        accepted, rejected, _, _ = bs.box_acceleration()
        out["accepted"], out["rejected"] = int(accepted.sum()), int(rejected.sum())
    return out


def run(n, m, N, batch, iters, reps, warmup, mems):
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_synthetic(1)
    assert bs.solve() == 0
    sol = bs.solutions()
    Z = np.zeros((batch, N * (2 * n + m)))
    Z[:, : bs.nvars] = sol
    Z = Z.reshape(batch, N, 2 * n + m)
    x, u = Z[:, :, n:2 * n], Z[:, : N - 1, 2 * n:]
    ucap = 0.5 * np.abs(u).mean(axis=(0, 1))
    xcap = np.empty((batch, N, n))
    for p in range(batch):
        g = R.generate_synthetic(n, m, N, 1 + p)
        roll = np.zeros((N, n))
        roll[0] = g["x0"]
        for k in range(N - 1):
            roll[k + 1] = g["A"][k].reshape(n, n).T @ roll[k] + g["d"][k]
        xcap[p] = np.maximum(0.7 * np.abs(x[p, 1:]).max(axis=0), np.abs(roll))
    rho = float(R.generate_synthetic(n, m, N, 1)["R"].mean())

    def resolve():
        assert bs.solve_rhs_only() == 0
        return bs.solve_ms()

    resolve_ms = median(resolve, reps, warmup)
    configs = {
        "shared_input_bounds": (None, None, -ucap, ucap),
        "per_problem_input_and_state_bounds": (-xcap, xcap,
                                               np.broadcast_to(-ucap, (batch, N, m)), np.broadcast_to(ucap, (batch, N, m)))}
    out = []
    for name, b in configs.items():
        nb = batch * ((N - 1) * m + ((N - 1) * n if b[0] is not None else 0))  # bounded entries
        line = {"shape": [n, m, N, batch], "bounds": name, "schedule": bs.schedule(), "rho": rho,
                "rhs_only_resolve_ms": round(resolve_ms, 4), "iters_timed": iters, "reps": reps, "memory": {}}
        for mem in mems:
            bs.initialize_synthetic(1)
            bs.set_bounds(*b)
            bs.set_box_acceleration(mem)
            kw = dict(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
            bs.solve_box(**kw)  # (factors)

            def fixed():
                bs.solve_box(**kw)
                return bs.solve_ms()

            per_iter = median(fixed, reps, warmup) / iters
            ring_gb = nb * 8 * (2 * (mem + 1) + 2) / 1e9 if mem > 0 else 0.0
            line["memory"][str(mem)] = {
                "ms_per_iteration": round(per_iter, 4), "iteration_minus_resolve_ms": round(per_iter - resolve_ms, 4),
                "ring_GB_per_iteration": round(ring_gb, 4), "ring_estimate_ms_at_copy_rate": round(ring_gb / COPY_TBPS, 4),
                "fixed_rho": cold_solve(bs, b, mem, rho=rho),
                "adapt_every_%d" % ADAPT: cold_solve(bs, b, mem, rho=rho, adapt_every=ADAPT)}
        base = line["memory"].get("0")
        if base:
            for mem, r in line["memory"].items():
                r["update_ms_over_box_update"] = round(r["ms_per_iteration"] - base["ms_per_iteration"], 4)
        out.append(line)
    bs.set_box_acceleration(0)
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mems", default="0,5,10")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "box_accel_bench.jsonl"))
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    for line in run(n, m, N, batch, a.iters, a.reps, a.warmup, [int(x) for x in a.mems.split(",")]):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
