"""Cost of the dense-cost gradient assembly (ndlqr_BatchGradientsDense) at (12,4,256) x 1024 and
(32,8,128) x 256, all nine outputs in device memory (torch tensors): medians over --reps repetitions after --warmup, the
spread (max - min) / median next to each; one JSON line per shape written to --out (profiles/grad_dense_bench.jsonl), which
every run replaces. Three legs:

  * per_problem: all nine per problem;
  * summed: all nine summed over the batch;
  * ab_summed: A and B summed, the rest per problem (system identification with shared dynamics).

For each, device_ms is the HIP-event time of the library's kernels (ndlqr_BatchSolveTimeMs: the packing of z and w, the map
to the caller's variables, grad_assemble_dense and the split pass) and torch_ms the torch assembly it replaces
(rslqr_amd.autograd._dense_gradients on the same z and w, plus .sum(0) of the summed outputs), timed with torch events in
the same process. *_peak_bytes: the growth of torch.cuda.max_memory_allocated over the leg, outputs included (the library's
outputs are allocated by torch, as the backward pass does). library_scratch_bytes: device-wide free memory before the legs
minus after them -- the library's own staging (the packed z | w and the partial sums) at the granularity of the
allocator, and whatever the runtime retains in between: an indication, not an exact count. written_bytes /
written_hbm_ms: the bytes the per-problem leg writes and their time at the HBM peak of rslqr_amd/roofline.py.
map_back_ms: one of the two launches of cost_apply inside a call (the map of the packed w to the caller's variables; HIP
events of its own under FLAG_PROFILE, in calls that are not the timed ones).

    python tools/grad_dense_bench.py [--reps 20] [--warmup 3] [--out profiles/grad_dense_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.zeros(1, device="cuda")  # (torch's HIP runtime before the library's: rslqr_amd/autograd.py)
import rslqr_amd as R  # noqa: E402
from rslqr_amd.autograd import _View, _dense_gradients  # noqa: E402
from rslqr_amd.roofline import HBM_PEAK_GBS  # noqa: E402
from cost_bench import on_device, problems  # noqa: E402

SHAPES = [(12, 4, 256, 1024), (32, 8, 128, 256)]
NAMES = R.GRAD_DENSE_NAMES
LEGS = (("per_problem", 0), ("summed", (1 << 9) - 1), ("ab_summed", R.GRADD_A | R.GRADD_B))


def median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = np.array([fn() for _ in range(reps)])
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


def peak_growth(fn):
    """growth of torch's peak allocation over one call of fn (whatever fn returns is dropped first)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def one_shape(n, m, N, batch, reps, warmup):
    out = dict(shape=[n, m, N, batch], reps=reps)
    _, dense = problems(n, m, N, batch)
    d_dense = on_device(dense, NAMES)
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_flat_dense(*d_dense)
    assert bs.solve() == 0 and bs.cholesky_failures() == 0
    out["schedule"] = bs.schedule()
    g = torch.randn((batch, bs.nvars), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    torch.cuda.synchronize()
    assert bs.solve_adjoint(_View(g)) == 0
    out["adjoint_ms"] = bs.solve_ms()
    z, w = torch.empty_like(g), torch.empty_like(g)
    bs.solutions_to_device(z.data_ptr())
    bs.synchronize()
    bs.adjoint(_View(w))
    written = 8 * batch * (N * (2 * n * n + 2 * n * m + m * m + 2 * n + m) + n)
    out["written_bytes"] = written
    out["written_hbm_ms"] = written / (HBM_PEAK_GBS * 1e9) * 1e3
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for leg, mask in LEGS:
        summed = [bool(mask & (1 << i)) for i in range(9)]

        def device(keep=None):
            res = {k: torch.empty(bs.dense_gradient_shape(k, s), dtype=torch.float64, device="cuda") for k, s in zip(NAMES, summed)}
            torch.cuda.synchronize()
            bs.gradients_dense(mask, {k: _View(v) for k, v in res.items()})
            if keep is not None:
                keep.update(res)
            return bs.solve_ms()

        def in_torch(keep=None):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = [t.sum(0) if s else t for t, s in zip(_dense_gradients(z, w, n, m, N), summed)]
            b.record()
            torch.cuda.synchronize()
            if keep is not None:
                keep.update(zip(NAMES, res))
            return a.elapsed_time(b)

        out[leg + "_device_ms"], out[leg + "_device_spread"] = median(device, reps, warmup)
        out[leg + "_torch_ms"], out[leg + "_torch_spread"] = median(in_torch, reps, warmup)
        out[leg + "_device_peak_bytes"] = peak_growth(device)
        out[leg + "_torch_peak_bytes"] = peak_growth(in_torch)
        # the two assemblies agree (math convention against flat column-major: compared through the norms of the difference)
        dev, ref = {}, {}
        device(dev)
        in_torch(ref)
        worst = 0.0
        for k in NAMES:
            a, b = dev[k], ref[k]
            if k in ("A", "B", "Q", "H", "R"):
                b = b.transpose(-1, -2).reshape(a.shape)
            worst = max(worst, float((a - b).norm() / b.norm()))
        out[leg + "_max_rel_diff"] = worst
        del dev, ref
    # the share of the map to the caller's variables: the second cost_apply of a per-problem call, by its own events
    bs.set_flags(R.FLAG_KEEP_RECORDS | R.FLAG_PROFILE)
    res = {k: torch.empty(bs.dense_gradient_shape(k), dtype=torch.float64, device="cuda") for k in NAMES}
    views = {k: _View(v) for k, v in res.items()}

    def map_back():
        bs.gradients_dense(0, views)
        return bs.cost_phase_ms()[2]

    out["map_back_ms"], out["map_back_spread"] = median(map_back, reps, warmup)
    bs.set_flags(R.FLAG_KEEP_RECORDS)
    del res, views
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out["library_scratch_bytes"] = int(free0 - torch.cuda.mem_get_info()[0])
    bs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_dense_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for n, m, N, batch in SHAPES:
        res = one_shape(n, m, N, batch, args.reps, args.warmup)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
