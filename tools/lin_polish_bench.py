"""Cost of the active-set polish of the solve with linear inequality constraints at (12,4,256) x
1024 with p = 4 (the input box as rows: C = 0, D = I) and p = 8 (four dense rows added) -- the problems and rows of
tools/lin_bench.py: medians over --reps repetitions after --warmup, the spread (max - min) / median next to each; one
JSON line per p written to --out (profiles/lin_polish_bench.jsonl), which every run replaces. Device times between the HIP
events of a blocking call (solve_ms()).

  * admm6: cold constrained solves to eps 1e-6 (a penalty 1 + k 2^-30 in repetition k, so that none reuses a
    factorisation): ms, iterations over the batch (min / median / max), statuses;
  * admm3_polish: the same to eps 1e-3, then polish_constrained() with the default settings: ms of each and their sum,
    iterations, accepted steps (min / median / max), factorisations of the polish (its rounds), statuses of the polish;
  * step: under FLAG_PROFILE on a second context, the device time of one polish split by launch kind -- residual_ms
    (lin_polish_residual), resolve_ms (lin_polish_apply_t + the re-solve), update_ms (lin_polish_update), each per launch;
  * residual_hbm_ms: the time lin_polish_residual's compulsory bytes take at the HBM peak of rslqr_amd/roofline.py: per
    knot Q, H, R, A, B, C, D, q, r, d, the knot's z and lambda, x of the next, mu, the codes (bytes) and both bounds in, the
    right-hand side and r_c out.

    python tools/lin_polish_bench.py [--reps 20] [--warmup 3] [--out profiles/lin_polish_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rslqr_amd as R  # noqa: E402
from lin_bench import BATCH, HOR, M_, N_, problems, rows  # noqa: E402
from rslqr_amd.roofline import HBM_PEAK_GBS  # noqa: E402

NAMES = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")


def spread(t):
    t = np.asarray(t, dtype=float)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def three(a):
    return [int(a.min()), int(np.median(a)), int(a.max())]


def counts(status):
    return {str(k): int((status == k).sum()) for k in sorted(set(status.tolist()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lin_polish_bench.jsonl"))
    a = ap.parse_args()
    _, dense = problems()
    rng = np.random.default_rng(11)
    lines = []
    for p in (4, 8):
        C, D, hi = rows(p, rng)
        line = dict(shape=[N_, M_, HOR], batch=BATCH, p=p, reps=a.reps, rho=1.0, alpha=1.6, max_iter=a.max_iter)
        bs = R.BatchSolver(N_, M_, HOR, BATCH)
        bs.initialize_flat_constrained(*[dense[k] for k in NAMES], C, D, -hi, hi)
        k = 0

        def admm(eps):
            nonlocal k
            k += 1
            iters, status = bs.solve_constrained(rho=1.0 + k * 2.0 ** -30, alpha=1.6, eps_abs=eps, eps_rel=eps, max_iter=a.max_iter)
            return bs.solve_ms(), iters, status
        ms = []
        for rep in range(a.warmup + a.reps):
            t, iters, status = admm(1e-6)
            ms.append(t)
        med, sp = spread(ms[a.warmup:])
        line["admm6"] = dict(ms=med, spread=sp, iters=three(iters), status=counts(status))
        ms3, msp = [], []
        for rep in range(a.warmup + a.reps):
            t, iters, status = admm(1e-3)
            fc = bs.factor_count()
            steps, pstatus = bs.polish_constrained()
            ms3.append(t)
            msp.append(bs.solve_ms())
            rounds = int(bs.factor_count() - fc)
        m3, s3 = spread(ms3[a.warmup:])
        mp, spp = spread(msp[a.warmup:])
        tot, stot = spread(np.array(ms3[a.warmup:]) + np.array(msp[a.warmup:]))
        line["admm3_polish"] = dict(admm_ms=m3, admm_spread=s3, polish_ms=mp, polish_spread=spp, total_ms=tot, total_spread=stot,
                                    iters=three(iters), admm_status=counts(status), steps=three(steps), rounds=rounds,
                                    polish_status=counts(pstatus))
        bs.close()
        # the split of a step, on a profiled context
        bs = R.BatchSolver(N_, M_, HOR, BATCH, flags=R.FLAG_PROFILE)
        bs.initialize_flat_constrained(*[dense[k] for k in NAMES], C, D, -hi, hi)
        per = []
        for rep in range(a.warmup + a.reps):
            admm(1e-3)
            bs.polish_constrained()
            phase, launches = bs.constraint_polish_phase_ms()
            per.append(phase / np.maximum(launches, 1))
        bs.close()
        per = np.array(per[a.warmup:])
        names = ("residual_ms", "resolve_ms", "update_ms")
        line["step"] = {nm: spread(per[:, i])[0] for i, nm in enumerate(names)}
        line["step"].update({nm.replace("_ms", "_spread"): spread(per[:, i])[1] for i, nm in enumerate(names)})
        line["step"]["launches"] = [int(x) for x in launches]
        n, m = N_, M_
        per_knot = 8 * (2 * n * n + 2 * n * m + m * m + p * (n + m) + (2 * n + m) + (2 * n + m) + 2 * n + p + 2 * p + (2 * n + m) + p) + p
        nbytes = per_knot * BATCH * HOR
        line["residual_bytes"] = nbytes
        line["residual_hbm_ms"] = nbytes / (HBM_PEAK_GBS * 1e9) * 1e3
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
