"""Adjoint solve and parameter gradients, host side: the entry points are exported and refuse a NULL solver, and the
gradient formulas of kernels_grad.hpp -- evaluated by numpy on the CPU oracle's z and w -- agree with central differences
of L = g . z through the oracle (no GPU needed)."""
import numpy as np
import pytest

from support import Problem, gradient_direction_bar, gradient_direction_ld
from test_gpu_gradients import ARGS, adjoint_problem, directions, grad_formula


def test_null_solver_is_refused(ndlqr):
    L = ndlqr.lib()
    g = np.zeros(4)
    assert L.ndlqr_SolveBatchAdjoint(None, g.ctypes.data_as(ndlqr.api.dp)) == -1
    assert L.ndlqr_CopyBatchAdjoint(None, g.ctypes.data_as(ndlqr.api.dp)) == -1
    assert L.ndlqr_BatchGradients(None, 0, *([None] * 8)) == -1
    assert ndlqr.GRAD_NAMES == ARGS and [getattr(ndlqr, "GRAD_" + k) for k in ARGS] == [1 << i for i in range(8)]


@pytest.mark.parametrize("n,m,N,seed", [(3, 2, 8, 1), (2, 1, 4, 2)])
def test_gradient_formulas_match_finite_differences(ndlqr, oracle, n, m, N, seed):
    gen = ndlqr.generate_synthetic(n, m, N, seed)
    prob = Problem(n, m, N, *[gen[k] for k in ARGS])
    g = np.random.default_rng(seed).standard_normal(prob.nvars)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    w = oracle.solve(adjoint_problem(prob, g), 1)[0][: prob.nvars]
    grads = grad_formula(prob, z, w)
    for k in ARGS:
        base = getattr(prob, k)
        fd = np.zeros(base.size)
        for e in range(base.size):
            h = 1e-5 * max(1.0, abs(base.flat[e]))
            vals = []
            for sgn in (1.0, -1.0):
                kw = {a: getattr(prob, a) for a in ARGS}
                kw[k] = base.copy()
                kw[k].flat[e] += sgn * h
                pr = Problem(n, m, N, *[kw[a] for a in ARGS])
                vals.append(float(g @ oracle.solve(pr, 1)[0][: pr.nvars]))
            fd[e] = (vals[0] - vals[1]) / (2 * h)
        assert np.linalg.norm(grads[k].ravel() - fd) <= 1e-6 * max(1.0, np.linalg.norm(fd)), (k, grads[k], fd)


@pytest.mark.parametrize("n,m,N,seed", [(3, 2, 8, 3)])
def test_kkt_operator_reference_matches_finite_differences(ndlqr, oracle, n, m, N, seed):
    """support.gradient_direction_ld (w^T times the change of the KKT residual, extended precision) against central
    differences of L = g . z through the oracle, in every direction of test_gpu_gradients.directions."""
    gen = ndlqr.generate_synthetic(n, m, N, seed)
    prob = Problem(n, m, N, *[gen[k] for k in ARGS])
    g = np.random.default_rng(seed).standard_normal(prob.nvars)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    w = oracle.solve(adjoint_problem(prob, g), 1)[0][: prob.nvars]
    h = 1e-5
    for k, label, V in directions(prob, seed):
        vals = []
        for sgn in (1.0, -1.0):
            kw = {a: getattr(prob, a) for a in ARGS}
            kw[k] = kw[k] + sgn * h * V
            pr = Problem(n, m, N, *[kw[a] for a in ARGS])
            vals.append(float(g @ oracle.solve(pr, 1)[0][: pr.nvars]))
        fd = (vals[0] - vals[1]) / (2 * h)
        value, size = gradient_direction_ld(prob, k, V, z, w)
        assert abs(float(value) - fd) <= 1e-6 * max(1.0, float(size)), (k, label, float(value), fd)
        if label == "knot %d" % (N - 1) and k in ("A", "B", "R", "r", "d"):
            assert value == 0 and size == 0, (k, label)


def test_kkt_operator_reference_matches_the_formulas(ndlqr, oracle):
    """... and against the outer-product formulas of kernels_grad.hpp (grad_formula) at (12,4,16): <G, V> within the
    rounding of the products, and gradient_direction_bar with exact z, w is rounding alone."""
    n, m, N = 12, 4, 16
    gen = ndlqr.generate_synthetic(n, m, N, 5)
    prob = Problem(n, m, N, *[gen[k] for k in ARGS])
    g = np.random.default_rng(5).standard_normal(prob.nvars)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    w = oracle.solve(adjoint_problem(prob, g), 1)[0][: prob.nvars]
    G = grad_formula(prob, z, w)
    for k, label, V in directions(prob, 6):
        got = (np.asarray(G[k], dtype=np.longdouble) * V).sum()
        value, size = gradient_direction_ld(prob, k, V, z, w)
        assert abs(got - value) <= 4 * np.finfo(np.float64).eps * size, (k, label, float(got), float(value))
        ref, bar = gradient_direction_bar(prob, k, V, z, w, z, w)
        assert ref == value and bar == 32 * np.finfo(np.float64).eps * size, (k, label)
    # a wrong formula is caught: gA with its two terms' roles swapped in one knot
    bad = G["A"].copy()
    bad[3] = bad[3].reshape(n, n).T.ravel()
    V = np.zeros_like(bad)
    V[3] = np.random.default_rng(7).standard_normal(n * n)
    value, size = gradient_direction_ld(prob, "A", V, z, w)
    assert abs((np.asarray(bad, dtype=np.longdouble) * V).sum() - value) > 1e3 * np.finfo(np.float64).eps * size
