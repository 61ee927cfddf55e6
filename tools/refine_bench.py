"""Cost and effect of the iterative refinement (ndlqr_RefineBatch) at 1024 x (12,4,256), on the benign synthetic family and
on a weak-input-cost one (R x 1e-4), one JSON line per family appended to profiles/refine_bench.jsonl:

  * HIP-event times, medians over --reps calls: the whole refine(max_steps) call; under NDLQR_FLAG_PROFILE the residual
    kernels (max_steps + 1 launches of kkt_residual_dd), the re-solves and the commits of one call; the rhs-only re-solve
    (ndlqr_SolveBatchRhsOnly) and ndlqr_BatchKktResiduals (kkt_residual_generic) in the same process, on the same batch;
    ndlqr_BatchKktResidualVector (one kkt_residual_dd launch plus the pack);
  * kkt_residual_dd against its byte estimate: it reads [A | B], QR, rhs, z and delta and writes r;
  * eta before and after, the steps taken, and the normwise error per field of --check problems against
    refined_solution(iters=5) (CPU oracle) before and after.

    python tools/refine_bench.py [--shape 12,4,256,1024] [--max-steps 2] [--reps 10] [--check 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rslqr_amd as R  # noqa: E402
from refine_support import EPS, field_errors  # noqa: E402
from support import Oracle, Problem, refined_solution  # noqa: E402

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
COPY_TBPS = 6.0  # measured HBM copy rate of the MI355X (read + write bytes per second)


def family(n, m, N, batch, r_scale):
    probs = []
    for p in range(batch):
        g = R.generate_synthetic(n, m, N, 1 + p)
        g["R"] = g["R"] * r_scale
        probs.append(g)
    return [np.stack([g[k] for g in probs]) for k in ARGS]


def median_event_ms(fn, bs, reps):
    ts = []
    for _ in range(reps):
        fn()
        ts.append(bs.solve_ms())
    return float(np.median(ts))


def run(name, n, m, N, batch, r_scale, max_steps, reps, ncheck):
    arrs = family(n, m, N, batch, r_scale)
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*arrs)

    def solve():
        assert bs.solve() == 0

    solve()
    z0 = bs.solutions().copy()
    steps, before, after = bs.refine(max_steps)
    z1 = bs.solutions().copy()
    orc = Oracle()
    errs = []
    for p in range(ncheck):
        prob = Problem(n, m, N, *[a[p] for a in arrs])
        truth = refined_solution(orc, prob, iters=5)
        e0, size = field_errors(prob, z0[p], truth)
        e1, _ = field_errors(prob, z1[p], truth)
        errs.append({"problem": p, "before_eps": (e0 / (EPS * size)).round(2).tolist(),
                     "after_eps": (e1 / (EPS * size)).round(2).tolist()})
    # timings: every refinement starts from a fresh solve (a refined solution would reject its first step)
    whole = []
    for _ in range(reps):
        solve()
        bs.refine(max_steps)
        whole.append(bs.solve_ms())
    resolve = median_event_ms(lambda: bs.solve_rhs_only(), bs, reps)
    solve()
    bs.kkt_residuals()  # (warm-up: its scratch is allocated on first use)
    vec = R.DeviceArray((batch, bs.nvars))
    t_vector = median_event_ms(lambda: bs.kkt_residual_vector(vec), bs, reps)
    bs.set_flags(R.FLAG_KEEP_RECORDS | R.FLAG_PROFILE)
    phases = []
    for _ in range(reps):
        solve()
        bs.refine(max_steps)
        phases.append(bs.refine_phase_ms())
    bs.set_flags(R.FLAG_KEEP_RECORDS)
    solve()
    residual_ms, resolve_in_ms, commit_ms = (float(x) for x in np.median(np.array(phases), axis=0))
    one_residual = residual_ms / (max_steps + 1)
    w, rows = n + m, 2 * n + m
    gbytes = 8.0 * batch * N * (n * w + w + 4 * rows) / 1e9  # [A | B], QR; rhs, z, delta read; r written
    # ndlqr_BatchKktResiduals has no event of its own: host wall time around the blocking call, the batch being resident
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        bs.kkt_residuals()
        ts.append((time.perf_counter() - t) * 1e3)
    t_generic = float(np.median(ts))
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        bs.kkt_residual_vector(vec)
        ts.append((time.perf_counter() - t) * 1e3)
    t_vector_wall = float(np.median(ts))
    out = {"family": name, "shape": [n, m, N, batch], "schedule": bs.schedule(), "max_steps": max_steps, "reps": reps,
           "refine_call_ms": round(float(np.median(whole)), 4), "rhs_only_resolve_ms": round(resolve, 4),
           "residual_dd_kernels_ms": round(residual_ms, 4), "residual_dd_one_launch_ms": round(one_residual, 4),
           "resolves_in_refine_ms": round(resolve_in_ms, 4), "commits_ms": round(commit_ms, 4),
           "step_over_resolve": round((float(np.median(whole)) - one_residual) / max_steps / resolve, 3),
           "residual_dd_algorithmic_GB": round(gbytes, 4), "residual_dd_TBps": round(gbytes / one_residual, 3),
           "residual_dd_fraction_of_copy_rate": round(gbytes / one_residual / COPY_TBPS, 3),
           "kkt_residual_vector_event_ms": round(t_vector, 4), "kkt_residual_vector_wall_ms": round(t_vector_wall, 4),
           "kkt_residuals_generic_wall_ms": round(t_generic, 4),
           "steps_histogram": np.bincount(steps, minlength=max_steps + 1).tolist(),
           "eta_before_median": float(np.median(before)), "eta_before_max": float(np.max(before)),
           "eta_after_median": float(np.median(after)), "eta_after_max": float(np.max(after)),
           "field_errors_lambda_x_u": errs}
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--max-steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.jsonl"))
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    with open(a.out, "a") as fh:
        for name, r_scale in (("benign", 1.0), ("weak-R", 1e-4)):
            line = json.dumps(run(name, n, m, N, batch, r_scale, a.max_steps, a.reps, a.check))
            print(line, flush=True)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
