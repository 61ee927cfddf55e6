"""Backward-pass timings of the batch solver: HIP-event times (ndlqr_BatchSolveTimeMs) of

  * the forward solve with NDLQR_FLAG_KEEP_RECORDS,
  * ndlqr_SolveBatchAdjoint (adjoint right-hand side packed, re-solve on the kept records),
  * ndlqr_BatchGradients, per problem, all eight outputs into device memory,
  * ndlqr_BatchGradients, every output summed over the batch,

medians over --reps repetitions after --warmup, one JSON line per shape. The per-problem gradient kernel is store-bound:
its algorithmic traffic is (n^2 + n m + 3 n + 2 m) doubles written per knot (+ n for x0 per problem) and z, w read
(2 (2n+m) doubles per knot), set against the ~6 TB/s copy rate of the MI355X.

    python tools/grad_bench.py [--shapes 12,4,256,1024 64,16,512,256] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rslqr_amd as R  # noqa: E402

COPY_TBPS = 6.0  # measured HBM copy rate of the MI355X (read + write bytes per second)


def median_ms(fn, bs, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        fn()
        ts.append(bs.solve_ms())
    return float(np.median(ts))


def run(n, m, N, batch, reps, warmup):
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_synthetic(1)

    def solve():
        assert bs.solve() == 0

    fwd = median_ms(solve, bs, reps, warmup)
    schedule = bs.schedule()
    g = R.DeviceArray((batch, bs.nvars)).set(np.random.default_rng(0).standard_normal((batch, bs.nvars)))

    def adjoint():
        assert bs.solve_adjoint(g) == 0

    adj = median_ms(adjoint, bs, reps, warmup)
    per_out = {k: R.DeviceArray(bs.gradient_shape(k)) for k in R.GRAD_NAMES}
    sum_out = {k: R.DeviceArray(bs.gradient_shape(k, True)) for k in R.GRAD_NAMES}
    per = median_ms(lambda: bs.gradients(0, per_out), bs, reps, warmup)
    summed = median_ms(lambda: bs.gradients(0xFF, sum_out), bs, reps, warmup)
    wsum = n * n + n * m + 3 * n + 2 * m
    written = 8.0 * batch * (N * wsum + n)
    read = 8.0 * batch * N * 2 * (2 * n + m)
    gbytes = (written + read) / 1e9
    bs.close()
    return {"shape": [n, m, N, batch], "schedule": schedule, "forward_keep_records_ms": round(fwd, 4),
            "adjoint_ms": round(adj, 4), "gradients_per_problem_ms": round(per, 4),
            "gradients_batch_sum_ms": round(summed, 4), "per_problem_algorithmic_GB": round(gbytes, 4),
            "per_problem_TBps": round(gbytes / per, 3) if per > 0 else None,
            "fraction_of_copy_rate": round(gbytes / per / COPY_TBPS, 3) if per > 0 else None,
            "reps": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="*", default=["12,4,256,1024", "64,16,512,256"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for s in a.shapes:
        n, m, N, batch = (int(x) for x in s.split(","))
        print(json.dumps(run(n, m, N, batch, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
