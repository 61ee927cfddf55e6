"""Host-side checks of the box-constrained solve: the C entry points exist and refuse bad arguments without a device, and
the independent references of box_support.py agree with each other and with the oracle (CPU only)."""
import ctypes as C

import numpy as np
import pytest

from box_support import active_set_qp, admm_reference, bvls_inputs, certificate, condensed, split
from support import Problem

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def test_entry_points_refuse_without_a_solver(ndlqr):
    L = ndlqr.lib()
    for name in ("ndlqr_BatchSetBounds", "ndlqr_SolveBatchBoxConstrained", "ndlqr_CopyBatchBoundMultipliers"):
        assert name in ndlqr.exported_symbols()
    assert L.ndlqr_BatchSetBounds(None, 0, None, None, None, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_SolveBatchBoxConstrained(None, None, None, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_CopyBatchBoundMultipliers(None, None, None) == ndlqr.api.ERR_INVALID
    assert C.sizeof(ndlqr.NdLqrBoxSettings) == 4 * 8 + 3 * 4 + 4  # (padded to 8 bytes)
    assert ndlqr.BOUNDS_SHARED == 1


def test_condensed_problem_matches_the_oracle(ndlqr, oracle):
    prob = synth(ndlqr, 4, 2, 16, 5)
    G, c, H, g = condensed(prob)
    U = np.linalg.solve(H, -g)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    _, x, u = split(z, prob.n, prob.m, prob.N)
    assert np.abs(U.reshape(u.shape) - u).max() <= 1e-9 * max(1.0, np.abs(u).max())
    assert np.abs(c + np.einsum("kij,j->ki", G, U) - x).max() <= 1e-9 * max(1.0, np.abs(x).max())


def _input_box(oracle, prob, frac):
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    u = split(z, prob.n, prob.m, prob.N)[2]
    cap = frac * np.abs(u).max(axis=0)
    uhi = np.tile(cap, (prob.N, 1))
    return -uhi, uhi, u


def test_bvls_reference(ndlqr, oracle):
    prob = synth(ndlqr, 4, 2, 16, 6)
    ulo, uhi, u0 = _input_box(oracle, prob, 10.0)  # loose: the unconstrained solution
    u, _ = bvls_inputs(prob, ulo, uhi)
    assert np.abs(u - u0).max() <= 1e-8 * np.abs(u0).max()
    ulo, uhi, _ = _input_box(oracle, prob, 0.5)
    u, _ = bvls_inputs(prob, ulo, uhi)
    _, _, H, g = condensed(prob)
    grad = (H @ u.reshape(-1) + g).reshape(u.shape)
    hi, lo = uhi[: prob.N - 1], ulo[: prob.N - 1]
    at_hi, at_lo = np.isclose(u, hi, rtol=0, atol=1e-12), np.isclose(u, lo, rtol=0, atol=1e-12)
    assert at_hi.any() or at_lo.any()
    tol = 1e-8 * np.abs(grad).max()
    assert (np.abs(grad[~at_hi & ~at_lo]) <= tol).all()
    assert (grad[at_hi] <= tol).all() and (grad[at_lo] >= -tol).all()


def test_admm_restatement_with_the_oracle_meets_the_references(ndlqr, oracle):
    """The numpy restatement of the iteration, solving with the oracle: input bounds reach the bvls solution, state and
    input bounds pass the certificate and match the active-set QP."""
    n, m, N = 4, 2, 16
    prob = synth(ndlqr, n, m, N, 7)
    solve = lambda p: oracle.solve(p, 1)[0][: p.nvars]
    rho = float(prob.R.mean())
    ulo, uhi, _ = _input_box(oracle, prob, 0.5)
    inf = np.full((N, n), np.inf)
    x, u, mux, muu, lam, it, st = admm_reference(prob, solve, -inf, inf, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000)
    assert st == 1, it
    ub, _ = bvls_inputs(prob, ulo, uhi)
    assert np.linalg.norm(u[: N - 1] - ub) <= 1e-6 * np.linalg.norm(ub), it
    assert (u[: N - 1] <= uhi[: N - 1]).all() and (u[: N - 1] >= ulo[: N - 1]).all()
    # state bounds as well: clip x at 60 % of its unconstrained range
    z0 = solve(prob)
    x0 = split(z0, n, m, N)[1]
    xhi = np.tile(0.6 * np.abs(x0[1:]).max(axis=0), (N, 1))
    xlo = -xhi
    x, u, mux, muu, lam, it, st = admm_reference(prob, solve, xlo, xhi, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000)
    assert st == 1, it
    z = np.concatenate([lam, x, u], axis=1).reshape(-1)[: prob.nvars]
    cert = certificate(prob, z, mux, muu, xlo, xhi, ulo, uhi, 1e-7)
    assert cert["stationarity"] <= 1e-7 and cert["bounds"] <= 0 and cert["complementarity"] <= 1e-7, cert
    ua, xa, na = active_set_qp(prob, xlo, xhi, ulo, uhi, x, u, mux, muu, 1e-7)
    assert na > 0
    assert np.linalg.norm(u[: N - 1] - ua) <= 1e-6 * np.linalg.norm(ua)
