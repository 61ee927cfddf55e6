"""Iterative refinement, the CPU side (no GPU): the numpy restatement of the device's double-double residual
(refine_support.residual_dd) against the 80-bit residual, and the refinement loop with its acceptance rule on the oracle
against support.refined_solution."""
import numpy as np
import pytest

from refine_support import EPS, field_errors, hard_problem, refine_loop, residual_dd
from support import kkt_residual_ld, refined_solution

# (n, m, N) x (a_scale, q_scale, r_scale): weak input cost, A scaled to 1.02 .. 1.1, Q by 1e-2 .. 1e-3
SHAPES = [(6, 3, 32), (12, 4, 64), (12, 4, 256), (16, 4, 32)]
SCALES = [(1.02, 1e-2, 1e-4), (1.1, 1e-3, 1e-4)]
# problems whose oracle solution is at rounding already: the first step does not lower the residual (found by a search
# over seeds on the CPU; tests/test_gpu_refine.py puts them beside a weak-R problem)
AT_ROUNDING = [(6, 3, 8, 38), (12, 4, 16, 258)]
AT_ROUNDING_SCALES = (0.125, 16.0, 16.0)


@pytest.fixture(scope="module")
def solved(ndlqr, oracle):
    """(problem, oracle solution, refined truth) of every family, computed once."""
    out = {}
    for i, (n, m, N) in enumerate(SHAPES):
        for j, sc in enumerate(SCALES):
            prob = hard_problem(ndlqr.generate_synthetic, n, m, N, 100 + 10 * i + j, *sc)
            z = oracle.solve(prob, 1)[0][: prob.nvars]
            out[(n, m, N, sc)] = (prob, z, refined_solution(oracle, prob, iters=5))
    return out


@pytest.mark.parametrize("n,m,N", SHAPES)
@pytest.mark.parametrize("sc", SCALES)
def test_restatement_against_the_extended_precision_residual(solved, n, m, N, sc):
    """Both values are roundings of the same exact number; 80-bit accumulation over at most n + m + 2 terms bounds the
    difference: every row within 2^-60 (|b_i| + sum_j |K_ij| |z_j|)."""
    prob, z, _ = solved[(n, m, N, sc)]
    r, rho, scale = residual_dd(prob, z)
    r_ld = np.concatenate(kkt_residual_ld(prob, z), axis=1).reshape(-1)[: prob.nvars]
    size_ld = np.concatenate(kkt_residual_ld_size(prob, z), axis=1).reshape(-1)[: prob.nvars]
    diff = np.abs(r.astype(np.longdouble) - r_ld)
    assert np.all(diff <= 2.0 ** -60 * size_ld), float(np.max(diff / size_ld))
    assert rho == np.max(np.abs(r)) and 0.5 * float(size_ld.max()) <= scale <= 2.0 * float(size_ld.max())


def kkt_residual_ld_size(prob, z):
    """|b_i| + sum_j |K_ij| |z_j| per row in extended precision: the residual of the problem with every datum and every
    entry of z replaced by its absolute value and the signs of K's identity blocks turned, so that all terms add."""
    n, m, N = prob.n, prob.m, prob.N
    ld = np.longdouble
    full = np.zeros(N * (2 * n + m), dtype=ld)
    full[: z.size] = np.abs(z)
    Z = full.reshape(N, 2 * n + m)
    lam, x, u = Z[:, :n], Z[:, n:2 * n], Z[:, 2 * n:]
    A = np.abs(prob.A).astype(ld).reshape(N, n, n).transpose(0, 2, 1)
    B = np.abs(prob.B).astype(ld).reshape(N, m, n).transpose(0, 2, 1)
    s_lam, s_x, s_u = np.zeros((N, n), dtype=ld), np.zeros((N, n), dtype=ld), np.zeros((N, m), dtype=ld)
    s_lam[0] = np.abs(prob.x0) + x[0]
    for k in range(N):
        nxt = A[k].T @ lam[k + 1] if k < N - 1 else 0
        s_x[k] = np.abs(prob.q[k]) + np.abs(prob.Q[k]) * x[k] + lam[k] + nxt
        if k < N - 1:
            s_u[k] = np.abs(prob.r[k]) + np.abs(prob.R[k]) * u[k] + B[k].T @ lam[k + 1]
            s_lam[k + 1] = np.abs(prob.d[k]) + A[k] @ x[k] + B[k] @ u[k] + x[k + 1]
    return s_lam, s_x, s_u


@pytest.mark.parametrize("n,m,N", SHAPES)
@pytest.mark.parametrize("sc", SCALES)
def test_one_step_lands_at_rounding(oracle, solved, n, m, N, sc):
    """One accepted step on the oracle's solution: within 4 ulp, normwise per field, of refined_solution(iters=5)."""
    prob, z, truth = solved[(n, m, N, sc)]
    z1, steps, before, after = refine_loop(oracle, prob, z, 1)
    err, size = field_errors(prob, z1, truth)
    print((n, m, N), sc, "error / (eps |field|):", err / (EPS * size), "eta %.2e -> %.2e" % (before, after))
    assert steps == 1 and after < before
    assert np.all(err <= 4 * EPS * size), err / (EPS * size)


def test_a_second_step_is_rejected_somewhere(oracle, solved):
    taken = [refine_loop(oracle, prob, z, 2)[1] for prob, z, _ in solved.values()]
    print("steps of two:", taken)
    assert all(1 <= t <= 2 for t in taken) and min(taken) == 1


@pytest.mark.parametrize("n,m,N,seed", AT_ROUNDING)
def test_a_problem_at_rounding_keeps_its_solution(ndlqr, oracle, n, m, N, seed):
    """The pairs of tests/test_gpu_refine.py: the problem at rounding is rejected at step 1 and keeps its z bit for bit,
    the weak-R one beside it is accepted."""
    prob = hard_problem(ndlqr.generate_synthetic, n, m, N, seed, *AT_ROUNDING_SCALES)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    z2, steps, before, after = refine_loop(oracle, prob, z, 2)
    assert steps == 0 and before == after and z2.tobytes() == z.tobytes()
    weak = hard_problem(ndlqr.generate_synthetic, n, m, N, seed)
    zw = oracle.solve(weak, 1)[0][: weak.nvars]
    assert refine_loop(oracle, weak, zw, 2)[1] >= 1
