"""Cost of the gradients through the solve with linear inequality constraints at (12,4,256) x
1024 with p = 4 and p = 8, the rows of tools/lin_bench.py: medians over --reps repetitions after --warmup, the spread
(max - min) / median next to each; one JSON line per p written to --out (profiles/lin_grad_bench.jsonl), which every run
replaces. Device times between the HIP events of a blocking call (solve_ms()); no host read inside a timed run
(check_every = max_iter; the adjoint's one read of its running count behind lin_adjoint_start cancels in the difference).

  * fwd_iter_ms, adj_iter_ms: one iteration of the forward and of the adjoint in the same process, each from runs of 1 and
    of 41 iterations on the remembered factorisation with tolerances that never converge; adj_over_fwd their ratio;
  * fwd_iters, adj_iters: the iteration counts to eps_abs = eps_rel = 1e-6 at rho = 1 (median and largest over the batch,
    and how many problems report status 1), g seeded standard normal;
  * adj_overhead_ms = adj1_ms - adj_iter_ms: what an adjoint costs beyond its iterations -- the two packs of the scope,
    lin_adjoint_start, lin_adjoint_finish, the saved and restored record columns;
  * grads_ms, grads_sum_ms: ndlqr_BatchConstraintGradients per problem and summed over the batch, all four outputs in
    device memory.

    python tools/lin_grad_bench.py [--reps 20] [--warmup 3] [--out profiles/lin_grad_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rslqr_amd as R  # noqa: E402
from lin_bench import BATCH, HOR, M_, N_, SET, median, problems, rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lin_grad_bench.jsonl"))
    a = ap.parse_args()
    _, dense = problems()
    rng = np.random.default_rng(11)
    names = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
    lines = []
    for p in (4, 8):
        C, D, hi = rows(p, rng)
        bs = R.BatchSolver(N_, M_, HOR, BATCH)
        bs.initialize_flat_constrained(*[dense[k] for k in names], C, D, -hi, hi)
        g = R.DeviceArray((BATCH, bs.nvars)).set(np.random.default_rng([p, 23]).standard_normal((BATCH, bs.nvars)))

        def fwd(k):
            bs.solve_constrained(rho=1.0, max_iter=k, check_every=k, **SET)
            return bs.solve_ms()
        f1, _ = median(lambda: fwd(1), a.reps, a.warmup)
        f41, sf41 = median(lambda: fwd(41), a.reps, a.warmup)
        # the forward the adjoint belongs to
        fit, fst = bs.solve_constrained(rho=1.0, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000)

        def adj(k):
            bs.solve_constrained_adjoint(g, max_iter=k, check_every=k, **SET)
            return bs.solve_ms()
        a1, sa1 = median(lambda: adj(1), a.reps, a.warmup)
        a41, sa41 = median(lambda: adj(41), a.reps, a.warmup)
        ait, ast = bs.solve_constrained_adjoint(g, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000)
        codes = bs.constraint_codes()
        outs = {s: {k: R.DeviceArray(((HOR, w) if s else (BATCH, HOR, w))) for k, w in
                    (("C", p * N_), ("D", p * M_), ("lo", p), ("hi", p))} for s in (False, True)}

        def grads(summed):
            bs.constraint_gradients(summed, outs[summed])
            return bs.solve_ms()
        gp, sgp = median(lambda: grads(False), a.reps, a.warmup)
        gs, sgs = median(lambda: grads(True), a.reps, a.warmup)
        bs.close()
        fi, ai = (f41 - f1) / 40.0, (a41 - a1) / 40.0
        lines.append(dict(shape=[N_, M_, HOR], batch=BATCH, p=p, reps=a.reps, fwd_iter_ms=fi, fwd41_spread=sf41, adj_iter_ms=ai,
                          adj41_spread=sa41, adj_over_fwd=ai / fi, adj1_ms=a1, adj1_spread=sa1, adj_overhead_ms=a1 - ai,
                          fwd_iters=[int(np.median(fit)), int(fit.max())], fwd_converged=int((fst == 1).sum()),
                          adj_iters=[int(np.median(ait)), int(ait.max())], adj_converged=int((ast == 1).sum()),
                          active_rows=float((codes >= 2).mean()), grads_ms=gp, grads_spread=sgp, grads_sum_ms=gs,
                          grads_sum_spread=sgs))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
