"""Cost of the solve with linear inequality constraints at (12,4,256) x 1024 with p = 4 (the
input box as rows: C = 0, D = I) and p = 8 (four dense rows added): medians over --reps repetitions after --warmup, the
spread (max - min) / median next to each; one JSON line per p written to --out (profiles/lin_bench.jsonl), which every
run replaces. Device times between the HIP events of a blocking call (solve_ms()); the host reads nothing inside a run
(check_every = max_iter).

  * setup_ms: lin_shift_cost + the reduction of the shifted problem (cost_factor, cost_transform, S^' of the right-hand
    side) + the pack + the factorisation: a constrained solve of one iteration with a penalty it has not seen, minus one
    iteration;
  * iter_ms: one iteration, from constrained solves of 1 and of 41 iterations on the remembered factorisation; split
    into resolve_ms -- the rhs-only re-solve of the same context on kept records -- and update_ms = iter_ms - resolve_ms,
    the share of lin_update; beside update_hbm_ms, the time lin_update's compulsory bytes take at the HBM peak of
    rslqr_amd/roofline.py: per knot the shifted record, C, D, the x and u rows of z~, of the resident and of the next
    right-hand side, and lo, hi, v, y in and v, y out;
  * reuse_overhead_ms = iter1_ms - iter_ms: what a constrained solve on the remembered factorisation costs beyond its
    iterations -- the pack of the shifted reduced problem on the way in and of the plain one on the way out (each an
    initialiser's pack launch behind a wait for both streams), lin_start and lin_finish -- beside pack_wall_ms, the host
    wall-clock of one such pack alone (initialize_flat_device + synchronize on a diagonal context, inputs in device
    memory), and call1_wall_ms, the host wall-clock of the whole one-iteration call;
  * for comparison from the same run: box_iter_ms, one iteration of the diagonal box solve (the same input box through
    ndlqr_BatchSetBounds on a diagonal context), and unfused_ms, S' + re-solve + S of section 3.16 (a new right-hand side
    through ndlqr_BatchSetRhsFlat + the rhs-only re-solve + the delivery's S, HIP events of FLAG_PROFILE).

    python tools/lin_bench.py [--reps 20] [--warmup 3] [--out profiles/lin_bench.jsonl]

With --adapt-every K it measures the per-problem adaptive penalty instead and writes
profiles/lin_adaptive_bench.jsonl: at the same shape and rows, cold solves from rho = 1 (+ k 2^-30 in repetition k, so that none reuses a factorisation) to eps 1e-6 within --max-iter
iterations, with the fixed penalty and with the penalty considered every K iterations, in one process on one context; per
variant the iterations over the batch (min / median / max), the statuses, the factorisations of one solve, ms per solve
(median device time over --reps) and ms per iteration (ms per solve / the largest iteration count, which is what the batch
runs), and for the adaptive variant the smallest and largest final penalty.

    python tools/lin_bench.py --adapt-every 25 [--reps 3] [--max-iter 1000] [--out profiles/lin_adaptive_bench.jsonl]
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
from rslqr_amd.roofline import HBM_PEAK_GBS  # noqa: E402

N_, M_, HOR, BATCH = 12, 4, 256, 1024
SET = dict(alpha=1.6, eps_abs=1e-300, eps_rel=1e-300)  # (never converged: every iteration runs; 0 would mean the default)


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = np.array([fn() for _ in range(reps)])
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def problems():
    eight = [R.generate_synthetic(N_, M_, HOR, 1 + p) for p in range(8)]
    g = [eight[p % 8] for p in range(BATCH)]
    diag = {k: np.stack([x[k] for x in g]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")}
    col = lambda v: np.ascontiguousarray(np.einsum("bkj,ij->bkij", v, np.eye(v.shape[-1]))).reshape(BATCH, HOR, -1)
    dense = dict(diag, Q=col(diag["Q"]), R=col(diag["R"]), H=np.zeros((BATCH, HOR, N_ * M_)))
    return diag, dense


def rows(p, rng):
    """C [batch, N, p*n], D [batch, N, p*m] column-major per knot and the shared bounds [p]: the input box, then dense rows"""
    C = np.zeros((BATCH, HOR, p, N_))
    D = np.zeros((BATCH, HOR, p, M_))
    D[:, :, :M_, :] = np.eye(M_)
    if p > M_:
        C[:, :, M_:, :] = rng.standard_normal((p - M_, N_)) / np.sqrt(N_)
        D[:, :, M_:, :] = rng.standard_normal((p - M_, M_)) / np.sqrt(M_)
    flat = lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(BATCH, HOR, -1)
    return flat(C), flat(D), np.full(p, 0.5)


def adaptive_main(a):
    _, dense = problems()
    rng = np.random.default_rng(11)
    names = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
    lines = []
    for p in (4, 8):
        C, D, hi = rows(p, rng)
        bs = R.BatchSolver(N_, M_, HOR, BATCH)
        bs.initialize_flat_constrained(*[dense[k] for k in names], C, D, -hi, hi)
        line = dict(shape=[N_, M_, HOR], batch=BATCH, p=p, reps=a.reps, rho=1.0, alpha=1.6, eps=1e-6, max_iter=a.max_iter,
                    adapt_every=a.adapt_every)
        for name, every in (("fixed", 0), ("adaptive", a.adapt_every)):
            bs.set_constraint_adaptation(every)
            ms, out = [], None
            for k in range(a.warmup + a.reps):
                fc = bs.factor_count()
                # (a penalty the remembered factorisation does not have: every solve shifts, reduces and factors)
                iters, status = bs.solve_constrained(rho=1.0 + (k + 1) * 2.0 ** -30, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_iter=a.max_iter)
                ms.append(bs.solve_ms())
                rho = bs.constraint_penalties()
                out = dict(iters=[int(iters.min()), int(np.median(iters)), int(iters.max())],
                           status={str(k): int((status == k).sum()) for k in sorted(set(status.tolist()))},
                           factorisations=int(bs.factor_count() - fc), rho=[float(rho.min()), float(rho.max())])
            t = np.array(ms[a.warmup:])
            out.update(solve_ms=float(np.median(t)), solve_spread=float((t.max() - t.min()) / np.median(t)),
                       ms_per_iteration=float(np.median(t)) / out["iters"][2])
            line[name] = out
        bs.close()
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--adapt-every", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    adaptive = a.adapt_every > 0
    a.reps = a.reps if a.reps is not None else (3 if adaptive else 20)
    a.warmup = a.warmup if a.warmup is not None else (1 if adaptive else 3)
    a.out = a.out or os.path.join(ROOT, "profiles", "lin_adaptive_bench.jsonl" if adaptive else "lin_bench.jsonl")
    if adaptive:
        return adaptive_main(a)
    diag, dense = problems()
    rng = np.random.default_rng(11)
    names = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
    lines = []
    # the diagonal box iteration, once
    box = R.BatchSolver(N_, M_, HOR, BATCH)
    box.initialize_flat(*[diag[k] for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")])
    box.set_bounds(ulo=-0.5 * np.ones(M_), uhi=0.5 * np.ones(M_))

    def box_run(k):
        box.solve_box(rho=1.0, max_iter=k, check_every=k, **SET)
        return box.solve_ms()
    b1, _ = median(lambda: box_run(1), a.reps, a.warmup)
    b41, bs41 = median(lambda: box_run(41), a.reps, a.warmup)
    devs = [R.DeviceArray(diag[k].shape).set(diag[k]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")]

    def pack_wall():
        t0 = time.perf_counter()
        box.initialize_flat_device(*[d.ptr for d in devs])
        box.synchronize()
        return (time.perf_counter() - t0) * 1e3
    pk, spk = median(pack_wall, a.reps, a.warmup)
    box.close()
    for p in (4, 8):
        C, D, hi = rows(p, rng)
        bs = R.BatchSolver(N_, M_, HOR, BATCH)
        bs.initialize_flat_constrained(*[dense[k] for k in names], C, D, -hi, hi)
        state = {"rho": 1.0}

        def run(k, fresh=False):
            if fresh:
                state["rho"] *= 1.0 + 2.0 ** -20  # (a penalty the remembered factorisation does not have)
            bs.solve_constrained(rho=state["rho"], max_iter=k, check_every=k, **SET)
            return bs.solve_ms()
        t1, s1 = median(lambda: run(1), a.reps, a.warmup)

        def call_wall():
            t0 = time.perf_counter()
            run(1)
            return (time.perf_counter() - t0) * 1e3
        cw, scw = median(call_wall, a.reps, a.warmup)
        t41, s41 = median(lambda: run(41), a.reps, a.warmup)
        f1, sf = median(lambda: run(1, True), a.reps, a.warmup)
        iter_ms = (t41 - t1) / 40.0
        # the re-solve alone, and the unfused S' + re-solve + S, on the same context
        bs.set_flags(R.FLAG_KEEP_RECORDS | R.FLAG_PROFILE)
        assert bs.solve() == 0

        def resolve():
            assert bs.solve_rhs_only() == 0
            return bs.solve_ms()
        rs, srs = median(resolve, a.reps, a.warmup)

        def unfused():
            bs.set_rhs_flat(dense["q"], dense["r"], dense["d"], dense["x0"])
            assert bs.solve_rhs_only() == 0
            t = bs.solve_ms()
            bs.solutions()
            ph = bs.cost_phase_ms()
            return ph[1] + t + ph[2]
        uf, suf = median(unfused, a.reps, a.warmup)
        bs.close()
        knots = BATCH * HOR
        per_knot = (N_ * N_ + M_ * M_ + M_ * N_) + p * (N_ + M_) + 3 * (N_ + M_) + 6 * p
        hbm_ms = 8.0 * per_knot * knots / (HBM_PEAK_GBS * 1e9) * 1e3
        lines.append(dict(shape=[N_, M_, HOR], batch=BATCH, p=p, reps=a.reps, setup_ms=f1 - iter_ms, setup_spread=sf,
                          iter_ms=iter_ms, iter1_ms=t1, reuse_overhead_ms=t1 - iter_ms, pack_wall_ms=pk, pack_wall_spread=spk,
                          call1_wall_ms=cw, call1_wall_spread=scw, iter41_ms=t41, iter41_spread=s41, resolve_ms=rs, resolve_spread=srs,
                          update_ms=iter_ms - rs, update_hbm_ms=hbm_ms, update_bytes=8 * per_knot * knots,
                          box_iter_ms=(b41 - b1) / 40.0, box41_spread=bs41, unfused_ms=uf, unfused_spread=suf))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
