"""Cost of a horizon that is no power of two ("Padded horizon"): the device runs the next power of
two, so by construction a solve at N costs what that costs. HIP-event times (ndlqr_BatchSolveTimeMs) at
(--shape n,m) x --batch for every horizon of --horizons:

  * solve: factor + solve in the default mode,
  * rhs_only: the re-solve on the records kept by a solve with FLAG_KEEP_RECORDS,
  * box_iteration: one ADMM iteration -- a constrained solve of --iters iterations that converges nowhere (eps = 1e-300)
    on the remembered shifted factorisation, shared input bounds at half the mean |u|, divided by --iters.

Medians over --reps repetitions after --warmup, and the spread of the repetitions, (max - min) / median, next to each; one
JSON line per horizon written to --out (profiles/horizon_bench.jsonl), which every run replaces.

    python tools/horizon_bench.py [--shape 12,4] [--batch 1024] [--horizons 100,128,129,192,255,256] [--iters 100]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rslqr_amd as R  # noqa: E402


def median(fn, reps, warmup):
    """(median, (max - min) / median) of `reps` calls after `warmup`"""
    for _ in range(warmup):
        fn()
    t = np.array([fn() for _ in range(reps)])
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def timed(bs, call):
    def run():
        assert call() == 0
        return bs.solve_ms()
    return run


def one_horizon(n, m, N, batch, iters, reps, warmup):
    P = 1
    while P < N:
        P *= 2
    out = dict(shape=[n, m, N, batch], device_horizon=P)
    bs = R.BatchSolver(n, m, N, batch)
    bs.initialize_synthetic(1)
    out["solve_ms"], out["solve_spread"] = median(timed(bs, bs.solve), reps, warmup)
    out["schedule"] = bs.schedule()
    bs.set_flags(R.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    out["rhs_only_ms"], out["rhs_only_spread"] = median(timed(bs, bs.solve_rhs_only), reps, warmup)
    # shared input bounds at half the mean |u| of the unconstrained solution of problem 0
    z = np.zeros(N * (2 * n + m))
    z[: bs.nvars] = bs.solution(0)
    u = z.reshape(N, 2 * n + m)[: N - 1, 2 * n:]
    hi = np.tile(0.5 * np.abs(u).mean(axis=0), (N, 1))
    bs.set_flags(0)
    bs.set_bounds(None, None, -hi, hi)
    kw = dict(rho=1.0, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
    bs.solve_box(**kw)  # (factors)

    def box():
        bs.solve_box(warm_start=True, **kw)
        return bs.solve_ms() / iters
    out["box_iteration_ms"], out["box_iteration_spread"] = median(box, max(3, reps // 4), 1)
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="12,4")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizons", default="100,128,129,192,255,256")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horizon_bench.jsonl"))
    a = ap.parse_args()
    n, m = (int(v) for v in a.shape.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()  # (a run replaces the file: no lines of an earlier run stay)
    for N in (int(v) for v in a.horizons.split(",")):
        line = json.dumps(one_horizon(n, m, N, a.batch, a.iters, a.reps, a.warmup))
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
