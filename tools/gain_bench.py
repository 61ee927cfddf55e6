"""Cost of the feedback gains (ndlqr_BatchFeedbackGains) at (12,4,256) x 1024, (32,8,128) x 256 and
(64,16,512) x 256, outputs in device memory: HIP-event medians (ndlqr_BatchSolveTimeMs) over --reps calls after --warmup,
the spread (max - min) / median next to each; one JSON line per shape written to --out (profiles/gain_bench.jsonl), which
every run replaces. Legs, in diagonal-cost and in dense-cost mode:

  * all: K, k, P, p of every knot;
  * K0: feedback_gains(0, 1, want=("K",)) -- the sweep runs over the whole horizon and writes one knot.

Beside each: *_bytes / *_hbm_ms, the bytes the call has to move -- [A | B], Q | R and the right-hand side of every knot
read once, the outputs written once; dense-cost mode: the sweep's outputs written and read once more and the records of
the delivered knots read -- and their time at the HBM peak of rslqr_amd/roofline.py; solve_ms: a plain solve() of the same
solver in the same run. `threads`: the diagonal `all` leg again at every workgroup size (NDLQR_GAIN_THREADS), with the
second input buffer and without it (NDLQR_GAIN_PREFETCH=0), where the shape allows them.

    python tools/gain_bench.py [--reps 20] [--warmup 3] [--out profiles/gain_bench.jsonl] [--shapes 0,1,2]
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
from cost_bench import median, on_device, problems  # noqa: E402

SHAPES = [(12, 4, 256, 1024), (32, 8, 128, 256), (64, 16, 512, 256)]
DIAG = ("A", "B", "Q", "R", "q", "r", "d", "x0")
DENSE = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")


def tiled_problems(n, m, N, batch):
    """cost_bench.problems for eight problems, repeated over the batch (the generator's dense algebra is host work)"""
    diag, dense = problems(n, m, N, min(batch, 8))
    rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (batch // a.shape[0]), axis=0)) if batch > a.shape[0] else a
    return {k: rep(v) for k, v in diag.items()}, {k: rep(v) for k, v in dense.items()}


def legs(bs, n, m, N, batch, reps, warmup, dense, out, tag):
    flat = dict(K=m * n, k=m, P=n * n, p=n)
    read = 8 * batch * N * (n * (n + m) + (n + m) + (2 * n + m))
    for leg, k0, nk, names in (("all", 0, N, ("K", "k", "P", "p")), ("K0", 0, 1, ("K",))):
        dev = {k: R.DeviceArray((batch, nk, flat[k])) for k in names}

        def call():
            assert not bs.feedback_gains(k0, nk, out=dev)["failures"].any()
            return bs.solve_ms()

        key = "%s_%s" % (tag, leg)
        out[key + "_ms"], out[key + "_spread"] = median(call, reps, warmup)
        written = 8 * batch * nk * sum(flat[k] for k in names)
        moved = read + written
        if dense:  # the sweep writes all four of the range, the map reads them and the records of those knots
            moved += 8 * batch * nk * (2 * sum(flat.values()) + n * n + m * m + m * n)
        out[key + "_bytes"] = moved
        out[key + "_hbm_ms"] = moved / (HBM_PEAK_GBS * 1e9) * 1e3
        out[key + "_over_hbm"] = out[key + "_ms"] / out[key + "_hbm_ms"]
        del dev


def one_shape(n, m, N, batch, reps, warmup):
    out = dict(shape=[n, m, N, batch], reps=reps, lds_bytes=R.feedback_gains_lds(n, m),
               lds_bytes_second=R.feedback_gains_lds(n, m, second=True))
    diag, dense = tiled_problems(n, m, N, batch)
    for tag, arrs, names in (("diag", diag, DIAG), ("dense", dense, DENSE)):
        bs = R.BatchSolver(n, m, N, batch)
        dev_in = on_device(arrs, names)
        if tag == "diag":
            bs.initialize_flat_device(*[a.ptr for a in dev_in])
        else:
            bs.initialize_flat_dense(*dev_in)
        del dev_in

        def solve():
            assert bs.solve() == 0
            return bs.solve_ms()

        out[tag + "_solve_ms"], out[tag + "_solve_spread"] = median(solve, reps, warmup)
        out[tag + "_schedule"] = bs.schedule()
        legs(bs, n, m, N, batch, reps, warmup, tag == "dense", out, tag)
        for leg in ("all", "K0"):
            out["%s_%s_over_solve" % (tag, leg)] = out["%s_%s_ms" % (tag, leg)] / out[tag + "_solve_ms"]
        if tag == "diag":  # the workgroup size and the second buffer, on the `all` leg
            flat = dict(K=m * n, k=m, P=n * n, p=n)
            dev = {k: R.DeviceArray((batch, N, v)) for k, v in flat.items()}
            sweep = {}
            for threads in (64, 128, 256):
                for pf in (1, 0):
                    if pf and not (n * (n + m) <= 8 * threads and 3 * n + 2 * m <= threads and  # (gain_prefetch_fits)
                                   out["lds_bytes_second"] <= 160 * 1024):
                        continue
                    os.environ["NDLQR_GAIN_THREADS"], os.environ["NDLQR_GAIN_PREFETCH"] = str(threads), str(pf)

                    def call():
                        bs.feedback_gains(out=dev)
                        return bs.solve_ms()

                    ms, spread = median(call, reps, warmup)
                    sweep["%d_%s" % (threads, "second" if pf else "single")] = [ms, spread]
            del os.environ["NDLQR_GAIN_THREADS"], os.environ["NDLQR_GAIN_PREFETCH"]
            out["threads"] = sweep
            del dev
        bs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain_bench.jsonl"))
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
