"""Box adjoint timings (ndlqr_SolveBatchBoxAdjoint, ndlqr_BatchBoundGradients): HIP-event times (ndlqr_BatchSolveTimeMs) of

  * one forward ADMM iteration and one backward (box adjoint) iteration: --iters iterations that converge nowhere
    (eps = 1e-300) on the remembered shifted factorisation, divided by --iters, against the rhs-only re-solve,
  * the iterations a cold forward and then its backward take to eps = 1e-6 (the default; at most --max-iter each),
  * the bound-gradient kernels, per problem and summed over the batch,

medians over --reps repetitions after --warmup, one JSON line per bounds configuration: shared input bounds, and
per-problem input + state bounds (those of tools/box_bench.py). The backward update kernel's algorithmic traffic per
iteration: per bounded entry z, the code, the adjoint's resident right-hand side and one of v / y read, that one and the
next right-hand side written (41 B); unbounded entries read the code alone. Its own time comes from a rocprofv3
--kernel-trace --stats run of this script (box_adjoint_update).

    python tools/box_grad_bench.py [--shape 12,4,256,1024] [--iters 200] [--reps 5] [--warmup 1] [--max-iter 3000]
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


def stats(a):
    return {"max": int(a.max()), "median": float(np.median(a)), "min": int(a.min())}


def run(n, m, N, batch, iters, reps, warmup, max_iter):
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
    gz = np.random.default_rng(0).standard_normal((batch, bs.nvars))

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
        it, st = bs.solve_box(rho=rho, max_iter=max_iter)
        fwd_ms = bs.solve_ms()
        ait, ast = bs.solve_box_adjoint(gz, max_iter=max_iter)
        bwd_ms = bs.solve_ms()
        bsum = bs.bound_gradients(summed=True)
        nactive = sum(int((bsum[k] != 0).sum()) for k in bsum)

        def bound_grads(summed):
            def f():
                bs.bound_gradients(summed=summed, out=out_dev[summed])
                return bs.solve_ms()
            return f

        out_dev = {False: {k: R.DeviceArray((batch, N, n if k[0] == "x" else m)) for k in ("xlo", "xhi", "ulo", "uhi")},
                   True: {k: R.DeviceArray((N, n if k[0] == "x" else m)) for k in ("xlo", "xhi", "ulo", "uhi")}}
        bg_ms = median(bound_grads(False), reps, warmup)
        bgs_ms = median(bound_grads(True), reps, warmup)

        def fixed_fwd():
            bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
            return bs.solve_ms()

        def fixed_bwd():
            bs.solve_box_adjoint(gz, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, check_every=iters)
            return bs.solve_ms()

        fwd_iter = median(fixed_fwd, reps, warmup) / iters
        bwd_iter = median(fixed_bwd, reps, warmup) / iters
        nb = batch * ((N - 1) * m + ((N - 1) * n if b[0] is not None else 0))
        ne = batch * N * (n + m)
        gbytes = (nb * 41 + (ne - nb) * 1) / 1e9
        out.append({"shape": [n, m, N, batch], "bounds": name, "schedule": schedule, "rho": rho,
                    "rhs_only_resolve_ms": round(resolve_ms, 4),
                    "forward_ms_per_iteration": round(fwd_iter, 4), "backward_ms_per_iteration": round(bwd_iter, 4),
                    "backward_minus_resolve_ms": round(bwd_iter - resolve_ms, 4),
                    "backward_update_algorithmic_GB": round(gbytes, 4),
                    "backward_update_estimate_ms_at_copy_rate": round(gbytes / COPY_TBPS, 4),
                    "forward_iterations_to_1e-6": stats(it), "forward_converged": int((st == 1).sum()),
                    "backward_iterations_to_1e-6": stats(ait), "backward_converged": int((ast == 1).sum()),
                    "forward_cold_ms": round(fwd_ms, 3), "backward_cold_ms": round(bwd_ms, 3),
                    "bound_gradients_ms": round(bg_ms, 4), "bound_gradients_summed_ms": round(bgs_ms, 4),
                    "active_bound_entries_of_the_sum": nactive, "max_iter": max_iter, "iters_timed": iters,
                    "reps": reps})
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=3000)
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    for line in run(n, m, N, batch, a.iters, a.reps, a.warmup, a.max_iter):
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
