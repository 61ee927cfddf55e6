"""Cost of the asynchronous step in dense-cost mode (ndlqr_BatchStepAsyncDense; DESIGN.md section 3.16, "The asynchronous
step") at (12,4,256) x 1024 and (32,8,128) x 256, every array in device memory. Per leg the HIP-event median
(ndlqr_BatchSolveTimeMs: from the first launch of the step to its last) over --reps steps after --warmup, each step
synchronised before the next, the spread (max - min) / median next to it, and the wall-clock median of step +
synchronize of the same steps; `*_pipelined_wall_ms`: wall clock per step of --reps steps with two in flight
(synchronize_previous). Legs, for the dense step and for the diagonal-cost step of the same shape:

  * a: the full right-hand side up, the whole vectors down;
  * b: the full right-hand side up, u of knot 0 down;
  * c: x0 up, u of knot 0 down with SOLN_ONLY;
  * d: as c under FLAG_KEEP_RECORDS (every timed step is the re-solve on the kept records).

The yardstick is what dense-cost mode offered for the same data before the step: set_rhs_flat (from device memory) +
solve (flags 0; `yard_solve`) or solve_rhs_only (KEEP_RECORDS; `yard_resolve`) + solutions() into pinned host memory,
each call synchronous -- wall-clock medians; `*_dev`: the same with solutions_to_device + synchronize in place of
solutions(), the kindest form of it. One JSON line per shape written to --out, which every run replaces.

    python tools/dense_step_bench.py [--reps 20] [--warmup 3] [--out profiles/dense_step_bench.jsonl] [--shapes 0,1]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rslqr_amd as R  # noqa: E402
from cost_bench import on_device  # noqa: E402
from gain_bench import tiled_problems  # noqa: E402

SHAPES = [(12, 4, 256, 1024), (32, 8, 128, 256)]
DIAG = ("A", "B", "Q", "R", "q", "r", "d", "x0")
DENSE = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
RHS = ("q", "r", "d", "x0")
U0 = R.SOLN_INPUT


def stats(t):
    t = np.asarray(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def time_steps(bs, call, reps, warmup, out, key):
    """call() enqueues one step; event and wall medians of synchronised steps, then the two-deep loop"""
    ev, wall = [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        assert call() == 0 and bs.synchronize() == 0
        if i >= warmup:
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(bs.solve_ms())
    out[key + "_ms"], out[key + "_spread"] = stats(ev)
    out[key + "_wall_ms"], out[key + "_wall_spread"] = stats(wall)
    t0 = time.perf_counter()
    for i in range(reps):
        assert call() == 0
        if i:
            assert bs.synchronize_previous() == 0
    assert bs.synchronize() == 0
    out[key + "_pipelined_wall_ms"] = 1e3 * (time.perf_counter() - t0) / reps
    out[key + "_schedule"] = bs.schedule()


def time_wall(call, reps, warmup):
    t = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            t.append(1e3 * (time.perf_counter() - t0))
    return stats(t)


def one_shape(n, m, N, batch, reps, warmup):
    out = dict(shape=[n, m, N, batch], reps=reps)
    diag, dense = tiled_problems(n, m, N, batch)
    rhs = dict(zip(RHS, on_device(dense, RHS)))  # (the right-hand side of the two problems is the same)
    dp = C.POINTER(C.c_double)
    rhs_ptrs = [C.cast(C.c_void_p(rhs[k].ptr), dp) for k in RHS]
    for tag, arrs, names in (("dense", dense, DENSE), ("diag", diag, DIAG)):
        for flags, legs in ((0, "abc"), (R.FLAG_KEEP_RECORDS, "d")):
            bs = R.BatchSolver(n, m, N, batch, flags=flags)
            dev_in = on_device(arrs, names)
            if tag == "diag":
                bs.initialize_flat_device(*[a.ptr for a in dev_in])
            else:
                bs.initialize_flat_dense(*dev_in)
            del dev_in
            whole, u0 = R.DeviceArray((batch, bs.nvars)), R.DeviceArray((batch, 1, m))
            full = (rhs["q"], rhs["r"], rhs["d"], rhs["x0"])
            x0only = (None, None, None, rhs["x0"])
            for leg in legs:
                args = full if leg in "ab" else x0only
                sel = None if leg == "a" else (0, 1, U0 | (R.SOLN_ONLY if leg in "cd" else 0))
                dst = whole if leg == "a" else u0
                if tag == "dense":
                    call = lambda: bs.step_dense_async(*args, dst, selection=sel)
                else:
                    bs.set_step_selection(*(sel or (0, 0, 7)))
                    call = lambda: bs.step_async(*args, dst)
                time_steps(bs, call, reps, warmup, out, "%s_%s" % (tag, leg))
            if tag == "diag":
                bs.set_step_selection()
                bs.close()
                continue
            # the yardstick: the synchronous sequence for the same data, on the same solver
            host = R.pinned_empty((batch, bs.nvars))
            resolve = flags == R.FLAG_KEEP_RECORDS
            assert bs.solve() == 0

            def yard(to_device):
                assert bs.L.ndlqr_BatchSetRhsFlat(bs.h, *rhs_ptrs) == 0
                assert (bs.solve_rhs_only() if resolve else bs.solve()) == 0
                if to_device:
                    bs.solutions_to_device(whole.ptr)
                    assert bs.synchronize() == 0
                else:
                    bs.solutions(host)

            key = "yard_resolve" if resolve else "yard_solve"
            out[key + "_wall_ms"], out[key + "_wall_spread"] = time_wall(lambda: yard(False), reps, warmup)
            out[key + "_dev_wall_ms"], out[key + "_dev_wall_spread"] = time_wall(lambda: yard(True), reps, warmup)
            out[key + "_schedule"] = bs.schedule()
            bs.close()
    for leg in "abcd":
        yard_key = "yard_resolve" if leg == "d" else "yard_solve"
        out["dense_%s_over_yard" % leg] = out["dense_%s_wall_ms" % leg] / out[yard_key + "_wall_ms"]
        out["dense_%s_over_yard_dev" % leg] = out["dense_%s_wall_ms" % leg] / out[yard_key + "_dev_wall_ms"]
        out["dense_%s_minus_diag_ms" % leg] = out["dense_%s_ms" % leg] - out["diag_%s_ms" % leg]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_step_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for i in [int(s) for s in args.shapes.split(",")]:
        res = one_shape(*SHAPES[i], args.reps, args.warmup)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
