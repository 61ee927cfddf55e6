"""Adjoint solve and parameter gradients, host side: the entry points are exported and refuse a NULL solver, and the
gradient formulas of kernels_grad.hpp -- evaluated by numpy on the CPU oracle's z and w -- agree with central differences
of L = g . z through the oracle (no GPU needed)."""
import numpy as np
import pytest

from support import Problem
from test_gpu_gradients import ARGS, adjoint_problem, grad_formula


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
