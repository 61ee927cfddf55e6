"""Gradients through the box-constrained solve, host side: the entry points are exported and refuse a NULL solver, and the
math of DESIGN.md section 3.10 -- the adjoint of the active-set system, the parameter gradients of kernels_grad.hpp on the
constrained solution, the bound gradients = nu -- agrees with central differences of L = g . z* through an exact
constrained forward (bvls on the condensed problem, input bounds; no GPU needed)."""
import numpy as np
import pytest

from box_grad_support import active_adjoint, active_codes, active_forward, bound_grads
from box_support import bvls_inputs, split
from support import Problem
from test_gpu_gradients import ARGS, grad_formula


def test_entry_points_refuse_without_a_solver(ndlqr):
    L = ndlqr.lib()
    for name in ("ndlqr_SolveBatchBoxAdjoint", "ndlqr_BatchBoundGradients"):
        assert name in ndlqr.exported_symbols()
    g = np.zeros(4)
    assert L.ndlqr_SolveBatchBoxAdjoint(None, g.ctypes.data_as(ndlqr.api.dp), None, None, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_BatchBoundGradients(None, 0, None, None, None, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_BatchBoundGradients(None, ndlqr.BOUNDS_SHARED, None, None, None, None) == ndlqr.api.ERR_INVALID
    from rslqr_amd.autograd import lqr_solve_box  # noqa: F401
    assert hasattr(ndlqr.BatchSolver, "solve_box_adjoint") and hasattr(ndlqr.BatchSolver, "bound_gradients")


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def exact_forward(prob, ulo, uhi):
    """z* [nvars] with input bounds: u, x from bvls, lambda by the backward recursion of the x rows of the KKT system
    (no bounds on x: lam_k = Q_k x_k + q_k + A_k' lam_k+1)"""
    n, m, N = prob.n, prob.m, prob.N
    u, x = bvls_inputs(prob, ulo, uhi)
    A = prob.A.reshape(N, n, n).transpose(0, 2, 1)
    lam = np.zeros((N, n))
    for k in range(N - 1, -1, -1):
        lam[k] = prob.Q[k] * x[k] + prob.q[k] + (A[k].T @ lam[k + 1] if k < N - 1 else 0.0)
    zb = 2 * n + m
    Z = np.zeros((N, zb))
    Z[:, :n], Z[:, n:2 * n], Z[: N - 1, 2 * n:] = lam, x, u
    return Z.reshape(-1)[: prob.nvars]


def snap(prob, z, ulo, uhi, tol):
    """z with the inputs within tol of a bound put on it (bvls' result is clipped, but may sit an ulp away)"""
    n, m, N = prob.n, prob.m, prob.N
    zb = 2 * n + m
    Z = np.zeros(N * zb)
    Z[: z.size] = z
    Z = Z.reshape(N, zb)
    u = Z[: N - 1, 2 * n:]
    u[:] = np.where(np.abs(u - uhi[: N - 1]) <= tol, uhi[: N - 1], np.where(np.abs(u - ulo[: N - 1]) <= tol, ulo[: N - 1], u))
    return Z.reshape(-1)[: z.size]


@pytest.mark.parametrize("n,m,N,seed,frac", [(3, 2, 8, 11, 0.5), (2, 1, 8, 13, 0.6)])
def test_math_matches_central_differences(ndlqr, oracle, n, m, N, seed, frac):
    prob = synth(ndlqr, n, m, N, seed)
    z0 = oracle.solve(prob, 1)[0][: prob.nvars]
    u0 = split(z0, n, m, N)[2]
    cap = frac * np.abs(u0).mean(axis=0)
    uhi = np.tile(cap, (N, 1))
    ulo = -uhi
    z = snap(prob, exact_forward(prob, ulo, uhi), ulo, uhi, 1e-12)
    codes = active_codes(prob, z, None, None, ulo, uhi)
    assert (codes >= 2).any() and (codes == 1).any(), codes
    # the equality-constrained forward on that active set is the bvls solution, with strictly complementary multipliers
    za, mu = active_forward(prob, codes, None, None, ulo, uhi)
    assert np.abs(za - z).max() <= 1e-10 * max(1.0, np.abs(z).max())
    u = split(z, n, m, N)[2]
    margin_mu = np.abs(mu[codes >= 2]).min()
    gap = np.minimum(np.abs(u - uhi[: N - 1]), np.abs(u - ulo[: N - 1]))[codes[: N - 1, n:] == 1]
    assert margin_mu > 1e-4 and gap.min() > 1e-4, (margin_mu, gap.min())
    assert (np.sign(mu[codes == 3]) >= 0).all() and (np.sign(mu[codes == 2]) <= 0).all()
    g = np.random.default_rng(seed).standard_normal(prob.nvars)
    w, nu = active_adjoint(prob, codes, g)
    grads = grad_formula(prob, z, w)
    bgr = bound_grads(codes, nu, n)
    L = lambda pr, lo, hi: float(g @ exact_forward(pr, lo, hi))
    for k in ARGS:
        base = getattr(prob, k)
        fd = np.zeros(base.size)
        for e in range(base.size):
            h = 1e-6 * max(1.0, abs(base.flat[e]))
            vals = []
            for sgn in (1.0, -1.0):
                kw = {a: getattr(prob, a) for a in ARGS}
                kw[k] = base.copy()
                kw[k].flat[e] += sgn * h
                vals.append(L(Problem(n, m, N, *[kw[a] for a in ARGS]), ulo, uhi))
            fd[e] = (vals[0] - vals[1]) / (2 * h)
        assert np.linalg.norm(grads[k].ravel() - fd) <= 1e-5 * max(1.0, np.linalg.norm(fd)), (k, grads[k], fd)
    for name, arr in (("ulo", ulo), ("uhi", uhi)):
        fd = np.zeros(arr.shape)
        for idx in np.ndindex(arr.shape):
            h = 1e-6
            vals = []
            for sgn in (1.0, -1.0):
                lo, hi = ulo.copy(), uhi.copy()
                (lo if name == "ulo" else hi)[idx] += sgn * h
                vals.append(L(prob, lo, hi))
            fd[idx] = (vals[0] - vals[1]) / (2 * h)
        assert np.linalg.norm(bgr[name] - fd) <= 1e-5 * max(1.0, np.linalg.norm(fd)), (name, bgr[name], fd)
        assert np.linalg.norm(fd) > 1e-3  # (a bound that matters)
    assert not bgr["xlo"].any() and not bgr["xhi"].any()
