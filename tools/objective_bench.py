"""Cost of the objective read-out (ndlqr_BatchObjective), every array in device memory: the
HIP-event median (ndlqr_BatchSolveTimeMs: objective_diag or objective_dense, then objective_finish) over --reps calls after
--warmup, the spread (max - min) / median next to it, with the stage costs (`*_ms`) and without them (`*_J_ms`), beside

  * `*_hbm_ms`: the time of the call's bytes at the HBM peak of rslqr_amd/roofline.py -- z, QR and the right-hand side read
    once (diagonal costs and dense-cost mode, which runs the same kernel on the reduced problem), or z and the retained Q,
    H, R, q, r read once (after a constrained solve); the partials written and read once, J and the stage costs written;
  * `*_solve_ms`: solve() of the same solver, timed the same way in the same run.

Legs: (12,4,256) x 1024 with diagonal costs, dense costs, and after a constrained solve with p = 4 rows (five iterations:
the read-out does not care whether they converged); (12,4,8192) x 1 with diagonal costs. One JSON line per leg written to
--out, which every run replaces.

    python tools/objective_bench.py [--reps 20] [--warmup 3] [--out profiles/objective_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rslqr_amd as R  # noqa: E402
from rslqr_amd.roofline import HBM_PEAK_GBS  # noqa: E402
from cost_bench import median, on_device  # noqa: E402
from gain_bench import tiled_problems  # noqa: E402

DIAG = ("A", "B", "Q", "R", "q", "r", "d", "x0")
DENSE = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
LEGS = [("diagonal", 12, 4, 256, 1024), ("dense", 12, 4, 256, 1024), ("constrained", 12, 4, 256, 1024), ("diagonal", 12, 4, 8192, 1)]
ROWS = 4


def one_leg(kind, n, m, N, batch, reps, warmup):
    out = dict(leg=kind, shape=[n, m, N, batch], reps=reps)
    diag, dense = tiled_problems(n, m, N, batch)
    bs = R.BatchSolver(n, m, N, batch)
    kn = batch * N
    dev_in = None
    if kind == "diagonal":
        # (held until the first solve has waited for the pack kernel, which runs asynchronously: a DeviceArray frees its
        #  memory when it dies)
        dev_in = on_device(diag, DIAG)
        bs.initialize_flat_device(*[a.ptr for a in dev_in])
    elif kind == "dense":
        bs.initialize_flat_dense(*on_device(dense, DENSE))
    else:
        rng = np.random.default_rng(11)
        Cr = rng.standard_normal((batch, N, ROWS * n)) / np.sqrt(n)
        Dr = rng.standard_normal((batch, N, ROWS * m)) / np.sqrt(m)
        hi = np.full((N, ROWS), 0.5)
        bs.initialize_flat_constrained(*on_device(dense, DENSE), *on_device(dict(C=Cr, D=Dr), ("C", "D")), -hi, hi)
    assert bs.solve() == 0
    del dev_in
    print("%s %s: initialised and solved" % (kind, out["shape"]), file=sys.stderr, flush=True)

    def solve():
        assert bs.solve() == 0
        return bs.solve_ms()

    out["solve_ms"], out["solve_spread"] = median(solve, reps, warmup)
    out["solve_schedule"] = bs.schedule()
    if kind == "constrained":
        iters, status = bs.solve_constrained(rho=1.0, alpha=1.6, max_iter=5)
        out["constrained_status"] = sorted(set(status.tolist()))
        read = 8 * kn * ((2 * n + m) + n * n + n * m + m * m + n + m)
    else:
        read = 8 * kn * (2 * (2 * n + m) + (n + m))
    J, stage = R.DeviceArray((batch,)), R.DeviceArray((batch, N))
    for key, dst in (("objective", dict(J=J, stage=stage)), ("objective_J", dict(J=J))):
        def call():
            bs.objective(out=dst)
            return bs.solve_ms()
        out[key + "_ms"], out[key + "_spread"] = median(call, reps, warmup)
        moved = read + 8 * (4 * kn + batch + (kn if "stage" in dst else 0))
        out[key + "_bytes"] = moved
        out[key + "_hbm_ms"] = moved / (HBM_PEAK_GBS * 1e9) * 1e3
        out[key + "_over_hbm"] = out[key + "_ms"] / out[key + "_hbm_ms"]
        out[key + "_over_solve"] = out[key + "_ms"] / out["solve_ms"]
    assert np.isfinite(J.get()).all()
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for leg in LEGS:
        res = one_leg(*leg, args.reps, args.warmup)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
