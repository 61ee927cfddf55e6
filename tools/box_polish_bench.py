"""Active-set polish timings (ndlqr_PolishBatchBoxConstrained, ndlqr_SolveBatchPolishedAdjoint)
against the ADMM they replace: HIP-event times (ndlqr_BatchSolveTimeMs), one JSON line per bounds configuration and leg,
appended to --out (profiles/box_polish_bench.jsonl). Bounds as tools/box_bench.py: shared input bounds, and per-problem
input and state bounds. Legs, each a cold solve after fresh inputs, fixed rho and adaptive rho (--adapt-every):

  * admm_1e-6: the constrained solve to 1e-6;
  * admm_1e-3_polish: the constrained solve to 1e-3, then the polish (both times, iterations, steps, statuses);
  * box_adjoint_1e-6: the box adjoint to 1e-6 behind the first leg;
  * polished_adjoint: the polished adjoint behind the second.

Every leg records the certificate (tests/box_support.certificate, tol 0) of a sample of problems.

    python tools/box_polish_bench.py [--shape 12,4,256,1024] [--adapt-every 25] [--sample 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rslqr_amd as R  # noqa: E402
from box_support import certificate  # noqa: E402
from support import Problem  # noqa: E402

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def bounds_of(bs, n, m, N, batch):
    """the two bound sets of tools/box_bench.py from the unconstrained solution"""
    assert bs.solve() == 0
    Z = np.zeros((batch, N * (2 * n + m)))
    Z[:, : bs.nvars] = bs.solutions()
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
    ub = np.broadcast_to(ucap, (batch, N, m))
    return {"shared_input_bounds": (None, None, -ucap, ucap),
            "per_problem_input_and_state_bounds": (-xcap, xcap, -ub, ub)}


def certificates(bs, b, n, m, N, sample):
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    full = lambda a, k, p, sign: (np.full((N, k), sign * np.inf) if a is None else (a[p] if a.ndim == 3 else np.broadcast_to(a, (N, k))))
    out = []
    for p in range(sample):
        g = R.generate_synthetic(n, m, N, 1 + p)
        prob = Problem(n, m, N, *[g[k] for k in ARGS])
        out.append(certificate(prob, sol[p], mux[p], muu[p], full(b[0], n, p, -1), full(b[1], n, p, 1),
                               full(b[2], m, p, -1), full(b[3], m, p, 1), 0.0))
    return out


def counts(a):
    return {"min": int(a.min()), "median": float(np.median(a)), "max": int(a.max())}


def statuses(st):
    return {str(k): int((st == k).sum()) for k in sorted(set(st.tolist()))}


def run(n, m, N, batch, adapt_every, sample):
    bs = R.BatchSolver(n, m, N, batch, flags=R.FLAG_KEEP_RECORDS)
    bs.initialize_synthetic(1)
    rho = float(R.generate_synthetic(n, m, N, 1)["R"].mean())
    g = np.random.default_rng(0).standard_normal((batch, bs.nvars))
    for name, b in bounds_of(bs, n, m, N, batch).items():
        for adapt in (0, adapt_every):
            base = {"shape": [n, m, N, batch], "bounds": name, "rho": rho, "adapt_every": adapt}
            for eps, polish in ((1e-6, False), (1e-3, True)):
                bs.initialize_synthetic(1)
                bs.set_bounds(*b)
                f0 = bs.factor_count()
                it, st = bs.solve_box(rho=rho, eps_abs=eps, eps_rel=eps, max_iter=20000, adapt_every=adapt)
                leg = dict(base, leg="admm_1e-3_polish" if polish else "admm_1e-6", admm_ms=round(bs.solve_ms(), 3),
                           iterations=counts(it), admm_status=statuses(st))
                if polish:
                    steps, pst = bs.polish_box()
                    leg.update(polish_ms=round(bs.solve_ms(), 3), steps=counts(steps), polish_status=statuses(pst))
                leg.update(factorisations=int(bs.factor_count() - f0), certificates=certificates(bs, b, n, m, N, sample))
                yield leg
                if polish:
                    asteps, ast = bs.solve_polished_adjoint(g)
                    yield dict(base, leg="polished_adjoint", ms=round(bs.solve_ms(), 3), steps=counts(asteps),
                               status=statuses(ast))
                else:
                    ait, ast = bs.solve_box_adjoint(g, eps_abs=eps, eps_rel=eps, max_iter=20000)
                    yield dict(base, leg="box_adjoint_1e-6", ms=round(bs.solve_ms(), 3), iterations=counts(ait),
                               status=statuses(ast))
    bs.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="12,4,256,1024")
    ap.add_argument("--adapt-every", type=int, default=25)
    ap.add_argument("--sample", type=int, default=4, help="problems whose certificate is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_polish_bench.jsonl"))
    a = ap.parse_args()
    n, m, N, batch = (int(x) for x in a.shape.split(","))
    for line in run(n, m, N, batch, a.adapt_every, a.sample):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
