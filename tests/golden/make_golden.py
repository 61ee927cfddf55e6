#!/usr/bin/env python3
"""Generates tests/golden/synthetic_ref.npz and tests/golden/reference_trace.json from the REAL reference
(oracle/_ref/libref.so, built from the reference's sources by oracle/Makefile). Run where those sources are:

    make -C oracle && python tests/golden/make_golden.py            # both files
    make -C oracle && python tests/golden/make_golden.py trace      # reference_trace.json alone

The fixture holds, for a few seeded synthetic problems (inputs regenerated at test time from the
seed by ndlqr_GenerateSyntheticFlat, inputs are NOT stored): the reference's solution vector, its
KKT residual, and a few factor blocks after the full solve. Data only -- no reference source.
The JSON files next to this script are the reference's own test fixtures (lqr_prob.json,
lqr_prob_256.json, sample_problem.json, lqr_data.json), copied verbatim as data.

reference_trace.json is what tests/test_oracle_vs_reference.py compares the oracle with, phase by phase: for every
case the reference's arrays at each checkpoint as digests (support.digest: bit-exact, -0.0 read as 0.0), the integer
results of its tree-index functions and separator factorisations, and its Riccati solver's solution of the two JSON
fixtures.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from support import (GOLDEN, Oracle, Problem, Reference, digest, have_reference, load_json_problem,  # noqa: E402
                     split_block)

CASES = [  # (n, m, N, seed)
    (12, 4, 16, 1), (12, 4, 64, 2), (12, 4, 256, 3), (6, 3, 32, 4), (6, 3, 256, 5),
    (5, 2, 8, 6), (3, 1, 2, 7), (16, 8, 16, 8), (2, 2, 128, 9),
]


def main():
    assert have_reference(), "build oracle/_ref first (make -C oracle)"
    import rslqr_amd
    ref, orc = Reference(), Oracle()
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for (n, m, N, seed) in CASES:
        g = rslqr_amd.generate_synthetic(n, m, N, seed)
        prob = Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])
        rs = ref.solver(prob)
        rs.solve(1)
        z = rs.soln()[: prob.nvars].copy()
        res, bnorm = orc.kkt_residual(prob, z)
        key = "n%d_m%d_N%d_s%d" % (n, m, N, seed)
        out[key + "_soln"] = z
        out[key + "_kkt"] = np.array([res, bnorm])
        fact = rs.fact()
        K = prob.K
        # a few blocks: top column of first/middle/last knot, column 0 of knot 1
        picks = [(0, K - 1), (N // 2, K - 1), (N - 1, K - 1), (1, 0)]
        for (k, lvl) in picks:
            lam, st, inp = split_block(fact, prob, k, lvl)
            out[key + "_F%d_%d" % (k, lvl)] = np.concatenate([lam.ravel(), st.ravel(), inp.ravel()])
        # checksum of the whole factor array (sum and sum of squares)
        out[key + "_factsum"] = np.array([fact.sum(), (fact * fact).sum()])
        print(key, "kkt", res, "|soln|", np.linalg.norm(z))
    path = os.path.join(HERE, "synthetic_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


# the cases of tests/test_oracle_vs_reference.py
FIXTURES = ["lqr_prob.json", "lqr_prob_256.json"]
PHASE_CASES = [(12, 4, 32), (6, 3, 64), (5, 2, 8), (3, 1, 2), (16, 8, 16), (2, 1, 4)]  # seed 11
FULL_SOLVE_THREADS = [1, 3, 8]  # (12, 4, 64), seed 5


def synth(n, m, N, seed):
    import rslqr_amd
    g = rslqr_amd.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])


def phase_trace(ref, prob):
    """The reference's nested-dissection solve of `prob` taken apart (src/solve.c:68-134): [label, value] after
    every phase, in the order tests/test_oracle_vs_reference.py walks the oracle through the same phases."""
    r, RL = ref.solver(prob), ref.L
    N, K = prob.N, prob.K
    out = [["init data", digest(r.data())], ["init soln", digest(r.soln())]]
    RL.ndlqr_SolveLeaves(r.h)
    out += [["leaves fact", digest(r.fact())], ["leaves soln", digest(r.soln())]]
    tree, rdata, rfact = RL.ref_tree(r.h), RL.ref_data_nd(r.h), RL.ref_fact_nd(r.h)
    for level in range(K):
        nleaf = 1 << (K - level - 1)
        idxs = [RL.ndlqr_GetIndexFromLeaf(tree, leaf, level) for leaf in range(nleaf)]
        out.append(["level %d index from leaf" % level, idxs])
        for idx in idxs:
            for up in range(level, K):
                RL.ndlqr_FactorInnerProduct(rdata, rfact, idx, level, up)
        out.append(["level %d inner products" % level, digest(r.fact())])
        out.append(["level %d separator status" % level, [RL.ref_factor_separator(r.h, leaf, level)
                                                           for leaf in range(nleaf)]])
        out.append(["level %d separators" % level, digest(r.fact())])
        for leaf in range(nleaf):
            for up in range(level + 1, K):
                RL.ref_solve_chol_factor(r.h, leaf, level, up)
        out.append(["level %d cholesky solves" % level, digest(r.fact())])
        at = [RL.ndlqr_GetIndexAtLevel(tree, k, level) for k in range(N)]
        calc = [int(RL.ndlqr_ShouldCalcLambda(tree, idx, k)) for k, idx in enumerate(at)]
        out += [["level %d index at level" % level, at], ["level %d should calc lambda" % level, calc]]
        for k in range(N):
            for up in range(level + 1, K):
                RL.ndlqr_UpdateShurFactor(rfact, rfact, at[k], k, level, up, bool(calc[k]))
        out.append(["level %d schur updates" % level, digest(r.fact())])
    out.append(["index level", [RL.ndlqr_GetIndexLevel(tree, k) for k in range(N - 1)]])
    return out


def trace():
    assert have_reference(), "build oracle/_ref first (make -C oracle)"
    ref = Reference()
    out = {"fixtures": {}, "phases": {}, "full_solve": {}, "riccati": {}}
    for fname in FIXTURES:
        prob, _ = load_json_problem(os.path.join(GOLDEN, fname))
        rs = ref.solver(prob)
        rs.solve(1)
        out["fixtures"][fname] = {"soln": digest(rs.soln()), "fact": digest(rs.fact())}
        x, _ = ref.riccati(prob, reps=1)
        out["riccati"][fname] = x.tolist()  # (repr of a float is exact)
    for (n, m, N) in PHASE_CASES:
        out["phases"]["%d,%d,%d" % (n, m, N)] = phase_trace(ref, synth(n, m, N, 11))
    prob = synth(12, 4, 64, 5)
    for threads in FULL_SOLVE_THREADS:
        rs = ref.solver(prob)
        rs.solve(threads)
        out["full_solve"][str(threads)] = {"soln": digest(rs.soln()), "fact": digest(rs.fact())}
    path = os.path.join(HERE, "reference_trace.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] != ["trace"]:
        main()
    trace()
