"""Cost of the dense-cost reduction at (12,4,256) x 1024 and (32,8,128) x 256: medians over
--reps repetitions after --warmup, the spread (max - min) / median next to each; one JSON line per shape written to
--out (profiles/cost_bench.jsonl), which every run replaces. All inputs live in device memory.

  * reduce_ms: cost_factor + cost_transform (HIP events, FLAG_PROFILE), beside reduce_hbm_ms, the time their compulsory
    bytes take at the HBM peak of rslqr_amd/roofline.py -- read Q, H, R, A, B once, write the records and A~, B~ once, read
    the records of knots k and k + 1 again in cost_transform;
  * rhs_dense_ms = apply_t_ms + resolve_ms + apply_ms: S' of a new right-hand side, the re-solve on the kept records, S of
    the packed solution (HIP events each), beside rhs_plain_ms, the plain rhs-only re-solve of a diagonal-cost solver of the
    same shape;
  * init_solve_dense_ms: initialize_flat_dense + solve, beside init_solve_plain_ms: initialize_flat_device + solve of a
    diagonal-cost problem -- host wall-clock around the blocking calls (the sequences synchronise in between, so no pair of
    events brackets them).

    python tools/cost_bench.py [--reps 20] [--warmup 3] [--out profiles/cost_bench.jsonl]
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

SHAPES = [(12, 4, 256, 1024), (32, 8, 128, 256)]


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = np.array([fn() for _ in range(reps)])
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def problems(n, m, N, batch):
    """a diagonal synthetic problem per batch entry, and the dense one it becomes with H = 0.3 randn and R, Q' rotated"""
    rng = np.random.default_rng(7)
    eight = [R.generate_synthetic(n, m, N, 1 + p) for p in range(8)]
    g = [eight[p % 8] for p in range(batch)]
    diag = {k: np.stack([x[k] for x in g]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")}
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((m, m)))
    Rm = np.einsum("ij,bkj,lj->bkil", V, diag["R"], V)
    H = 0.3 * rng.standard_normal((batch, N, n, m))
    Q = np.einsum("ij,bkj,lj->bkil", U, diag["Q"], U) + H @ np.linalg.solve(Rm, H.transpose(0, 1, 3, 2))
    Q = 0.5 * (Q + Q.transpose(0, 1, 3, 2))
    col = lambda M: np.ascontiguousarray(M.transpose(0, 1, 3, 2)).reshape(batch, N, -1)
    dense = dict(diag, Q=col(Q), H=col(H), R=col(Rm))
    return diag, dense


def on_device(arrs, names):
    return [R.DeviceArray(arrs[k].shape).set(arrs[k]) for k in names]


def wall(fn):
    def run():
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    return run


def one_shape(n, m, N, batch, reps, warmup):
    out = dict(shape=[n, m, N, batch])
    diag, dense = problems(n, m, N, batch)
    d_diag = on_device(diag, ("A", "B", "Q", "R", "q", "r", "d", "x0"))
    d_dense = on_device(dense, ("A", "B", "Q", "H", "R", "q", "r", "d", "x0"))
    kn = batch * N
    rec = n * n + m * m + m * n
    bytes_reduce = 8 * kn * ((n * n + n * m + m * m) + rec + (n * n + n * m) + (rec + n * n) + (n * n + n * m))
    out["reduce_bytes"] = bytes_reduce
    out["reduce_hbm_ms"] = bytes_reduce / (HBM_PEAK_GBS * 1e9) * 1e3

    plain = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    dns = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)

    def init_solve_plain():
        plain.initialize_flat_device(*[a.ptr for a in d_diag])
        assert plain.solve() == 0

    def init_solve_dense():
        dns.initialize_flat_dense(*d_dense)
        assert dns.solve() == 0

    out["init_solve_plain_ms"], out["init_solve_plain_spread"] = median(wall(init_solve_plain), reps, warmup)
    out["init_solve_dense_ms"], out["init_solve_dense_spread"] = median(wall(init_solve_dense), reps, warmup)
    out["schedule"] = dns.schedule()

    def rhs_plain():
        assert plain.solve_rhs_only() == 0
        return plain.solve_ms()

    out["rhs_plain_ms"], out["rhs_plain_spread"] = median(rhs_plain, reps, warmup)

    def resolve():
        assert dns.solve_rhs_only() == 0
        return dns.solve_ms()

    out["resolve_ms"], out["resolve_spread"] = median(resolve, reps, warmup)
    # the reduction's own kernels, by HIP events (a profiled call waits for its kernels: these runs are not the wall-clock ones)
    dns.set_flags(R.FLAG_KEEP_RECORDS | R.FLAG_PROFILE)
    sol = R.DeviceArray((batch, dns.nvars))

    def phase(i, call):
        def run():
            call()
            return dns.cost_phase_ms()[i]
        return run

    out["reduce_ms"], out["reduce_spread"] = median(phase(0, lambda: dns.initialize_flat_dense(*d_dense)), reps, warmup)
    assert dns.solve() == 0
    out["apply_t_ms"], out["apply_t_spread"] = median(phase(1, lambda: dns.set_rhs_flat(dense["q"], dense["r"], dense["d"], dense["x0"])), reps, warmup)
    assert dns.solve_rhs_only() == 0

    def deliver():
        dns.solutions_to_device(sol.ptr)
        dns.synchronize()

    out["apply_ms"], out["apply_spread"] = median(phase(2, deliver), reps, warmup)
    out["rhs_dense_ms"] = out["apply_t_ms"] + out["resolve_ms"] + out["apply_ms"]
    plain.close()
    dns.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for n, m, N, batch in SHAPES:
        res = one_shape(n, m, N, batch, args.reps, args.warmup)
        print(json.dumps(res))
        lines.append(json.dumps(res))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
