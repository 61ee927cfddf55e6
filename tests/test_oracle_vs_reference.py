"""Oracle vs the real reference (oracle/_ref/libref.so, compiled from the reference's sources), replayed from
tests/golden/reference_trace.json: make_golden.py took the reference through the same phases on the same inputs and
stored a digest of every array these tests compare bit for bit (support.digest), the integer results of its
tree-index functions and separator factorisations, and its Riccati solver's solutions. Runs without the reference."""
import json
import os

import numpy as np
import pytest

from support import GOLDEN, Problem, digest, load_json_problem

with open(os.path.join(GOLDEN, "reference_trace.json")) as _fh:
    TRACE = json.load(_fh)


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])


@pytest.mark.parametrize("fname", ["lqr_prob.json", "lqr_prob_256.json"])
def test_fixture_bit_identical(oracle, fname):
    prob, soln = load_json_problem(os.path.join(GOLDEN, fname))
    z, fact, _, _ = oracle.solve(prob, 1, want_fact=True)
    ref = TRACE["fixtures"][fname]
    assert digest(z) == ref["soln"]
    assert digest(fact) == ref["fact"]
    assert np.linalg.norm(z[: prob.nvars] - soln) < 1e-6  # reference (bit-identical to z) vs its own golden


@pytest.mark.parametrize("n,m,N", [(12, 4, 32), (6, 3, 64), (5, 2, 8), (3, 1, 2), (16, 8, 16), (2, 1, 4)])
# nstates = 1 is outside the reference's domain: ndlqr_NewNdData(width=1) forces depth 1 (src/nddata.c:23-29),
# so its matrix factors lose their levels. The oracle and the GPU path handle it; no parity claim there.
def test_synthetic_bit_identical_every_phase(oracle, ndlqr, n, m, N):
    prob = synth(ndlqr, n, m, N, 11)
    ref = iter(TRACE["phases"]["%d,%d,%d" % (n, m, N)])

    def check(label, value):
        rlabel, rvalue = next(ref)
        assert rlabel == label
        assert value == rvalue, label

    o = oracle.solver(prob)
    OL = oracle.L
    check("init data", digest(o.data()))  # KKT assembly
    check("init soln", digest(o.soln()))
    for k in range(N):
        OL.oracle_solve_leaf(o.h, k)
    check("leaves fact", digest(o.fact()))
    check("leaves soln", digest(o.soln()))
    K = prob.K
    for level in range(K):
        nleaf = 1 << (K - level - 1)
        idxs = [(1 << level) * (2 * leaf + 1) - 1 for leaf in range(nleaf)]
        check("level %d index from leaf" % level, idxs)
        for idx in idxs:
            for up in range(level, K):
                OL.oracle_inner_product(o.h, 0, idx, level, up)
        check("level %d inner products" % level, digest(o.fact()))
        check("level %d separator status" % level, [OL.oracle_factor_separator(o.h, leaf, level)
                                                     for leaf in range(nleaf)])
        check("level %d separators" % level, digest(o.fact()))
        for idx in idxs:
            for up in range(level + 1, K):
                OL.oracle_solve_chol_factor(o.h, idx, level, up)
        check("level %d cholesky solves" % level, digest(o.fact()))
        at = [OL.oracle_index_at_level(k, level) for k in range(N)]
        calc = [OL.oracle_should_calc_lambda(idx, level, k) for k, idx in enumerate(at)]
        check("level %d index at level" % level, at)
        check("level %d should calc lambda" % level, [int(bool(c)) for c in calc])
        for k in range(N):
            for up in range(level + 1, K):
                OL.oracle_update_schur(o.h, 0, at[k], k, level, up, calc[k])
        check("level %d schur updates" % level, digest(o.fact()))
    check("index level", [OL.oracle_index_level(k) for k in range(N - 1)])
    assert next(ref, None) is None


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_full_solve_bit_identical(oracle, ndlqr, threads):
    prob = synth(ndlqr, 12, 4, 64, 5)
    z, fact, _, _ = oracle.solve(prob, threads, want_fact=True)
    ref = TRACE["full_solve"][str(threads)]
    assert digest(z) == ref["soln"] and digest(fact) == ref["fact"]
    res, bnorm = oracle.kkt_residual(prob, z[: prob.nvars])
    assert res <= 1e-9 * max(1.0, bnorm)


@pytest.mark.parametrize("fname", ["lqr_prob.json", "lqr_prob_256.json"])
def test_reference_riccati_on_the_fixtures(oracle, fname):
    """the reference's serial Riccati solver (src/riccati_solve.c:26-150), compiled into
    oracle/_ref, is the second CPU column of bench.py. On the two JSON fixtures it reproduces the stored
    solution (the reference's own check: test/riccati_solver_test.c:332-370, test/sample_problem_test.c:150-151)."""
    prob, soln = load_json_problem(os.path.join(GOLDEN, fname))
    x = np.asarray(TRACE["riccati"][fname])
    assert x.shape == (prob.nvars,)
    assert np.linalg.norm(x - soln) < 1e-6
    z, _, _, _ = oracle.solve(prob, 1)  # bit-identical to the reference's rsLQR (test_fixture_bit_identical)
    assert np.linalg.norm(x - z[: prob.nvars]) < 1e-6  # "same answer" as rsLQR (sample_problem_test.c:151)
