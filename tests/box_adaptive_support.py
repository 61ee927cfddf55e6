"""Reference for the per-problem adaptive penalty of the box-constrained batch solve.

- penalty_step(): the decision of one problem at an adapt iteration -- exact or correctly rounded operations only
  (ilogb through frexp, ldexp, one division), so that it reproduces the device's decision bit for bit.
- admm_adaptive_reference(): box_support.admm_reference with that rule, in the operation order of strict mode: each
  solve by a caller-given solver on the problem shifted by the current rho.
Test infrastructure.
"""
import math

import numpy as np

from box_support import blocks, masks, shifted_problem

RHO_MIN, RHO_MAX = 1e-6, 1e6  # the library's defaults


def ilogb(x):
    """C's ilogb of a finite x > 0"""
    return math.frexp(x)[1] - 1


def penalty_step(rho, r_prim, r_dual, sp, sd, rho_min=RHO_MIN, rho_max=RHO_MAX):
    """rho+ of a running problem from its residuals and their scales (rho itself when nothing moves)"""
    vals = (r_prim, r_dual, sp, sd)
    if not all(math.isfinite(a) and a > 0.0 for a in vals):
        return rho
    e = ilogb(r_prim / sp) - ilogb(r_dual / sd)
    k = int(e / 2)  # (C integer division: toward zero; |e| is far below 2^53)
    k = max(-6, min(6, k))
    if k == 0:
        return rho
    return min(max(math.ldexp(rho, k), rho_min), rho_max)


def admm_adaptive_reference(prob, solve, xlo, xhi, ulo, uhi, rho, alpha, eps_abs, eps_rel, max_iter, adapt_every,
                            rho_min=RHO_MIN, rho_max=RHO_MAX, trace=None):
    """The iteration of DESIGN.md sections 3.9 and 3.11 in the operation order of strict mode; solve(problem) -> z (nvars).
    adapt_every == 0: box_support.admm_reference. Returns (x, u from v as [N, n], [N, m]; mu_x, mu_u; lam of the last
    solve; iters; status; the final rho; the number of times rho changed). trace: a list that gets one dict per iteration
    -- it, resid = (r_prim, r_dual, sp, sd) and rho, the penalty the iteration ran with."""
    n, m, N = prob.n, prob.m, prob.N
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    M = np.concatenate([Mx, Mu], axis=1) > 0
    lo = np.concatenate([np.where(Mx > 0, xlo, -np.inf), np.where(Mu > 0, ulo, -np.inf)], axis=1)
    hi = np.concatenate([np.where(Mx > 0, xhi, np.inf), np.where(Mu > 0, uhi, np.inf)], axis=1)
    q = np.concatenate([prob.q, prob.r], axis=1)
    v = np.zeros((N, n + m))
    y = np.zeros((N, n + m))
    oma = 1.0 - alpha
    qt = q.copy()
    rho = float(rho)
    status, it, changes = 0, 0, 0
    Z = None
    mx = lambda a: float(np.abs(a[M]).max()) if M.any() else 0.0
    for it in range(1, max_iter + 1):
        z = solve(shifted_problem(prob, rho, Mx, Mu, np.ascontiguousarray(qt[:, :n]), np.ascontiguousarray(qt[:, n:])))
        Z = blocks(z, n, m, N)
        zx = Z[:, n:]
        zh = alpha * zx + oma * v
        vn = np.minimum(np.maximum(zh + y, lo), hi)
        yn = (y + zh) - vn
        vn = np.where(M, vn, 0.0)
        yn = np.where(M, yn, 0.0)
        r_prim = mx(zx - vn)
        r_dual = rho * mx(vn - v)
        sp = max(mx(zx), mx(vn))
        sd = rho * mx(yn)
        finite = all(math.isfinite(a) for a in (r_prim, r_dual, mx(zx), mx(vn), mx(yn)))
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        if trace is not None:
            trace.append(dict(it=it, resid=(r_prim, r_dual, sp, sd), rho=rho))
        if conv or not finite:
            status = 1 if conv else 3
            break
        if adapt_every > 0 and it % adapt_every == 0 and it < max_iter:
            new = penalty_step(rho, r_prim, r_dual, sp, sd, rho_min, rho_max)
            if new != rho:
                s = rho / new
                y = np.where(M, y * s, 0.0)
                rho = new
                changes += 1
        t = y - v
        t = rho * t
        qt = np.where(M, q + t, q)
    xu = np.where(M, v, Z[:, n:])
    mu = rho * y
    return xu[:, :n], xu[:, n:], mu[:, :n], mu[:, n:], Z[:, :n], it, status or 2, rho, changes
