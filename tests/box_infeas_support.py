"""Independent references for the infeasibility detection of the box-constrained batch solve
(ndlqr_BatchSetInfeasibilityDetection, ndlqr_CopyBatchInfeasibilityCertificate).

- infeasible_bounds() / barely_feasible_bounds(): input bounds +-ubar on every knot and ONE upper state bound placed
  `gap` below / above the SMALLEST value that state can reach inside the input box (box_support.condensed: x = c + G U,
  so min over the box of (G U)[0] = -||G[0, :]||_1 ubar): the first is provably infeasible, the second feasible with
  that bound active or nearly so. (An upper bound below the largest reachable value would exclude nothing.)
- farkas_check(): the four conditions of the certificate test evaluated in numpy longdouble from the problem data; it
  shares no code with the kernel.
- admm_infeas_reference(): box_support.admm_reference plus the test at the check iterations, each solve by a
  caller-given solver (the oracle on the shifted problem).
Test infrastructure.
"""
import numpy as np

from box_support import blocks, condensed, masks, matrices, shifted_problem


def _reach(prob, ubar, knot):
    """smallest value of state 0 of `knot` over the input box |u| <= ubar; for knot 1: (A_0 x0 + d_0)[0] - ||B_0[0, :]||_1 ubar"""
    G, c, _, _ = condensed(prob)
    return float(c[knot][0] - np.abs(G[knot][0]).sum() * ubar)


def _bounds(prob, ubar, knot, level):
    n, m, N = prob.n, prob.m, prob.N
    xlo = np.full((N, n), -np.inf)
    xhi = np.full((N, n), np.inf)
    xhi[knot][0] = level
    return xlo, xhi, np.full((N, m), -float(ubar)), np.full((N, m), float(ubar))


def infeasible_bounds(prob, ubar, knot, gap):
    """(xlo, xhi [N, n], ulo, uhi [N, m]): |u| <= ubar and x_knot[0] <= (its smallest reachable value) - gap: no point."""
    return _bounds(prob, ubar, knot, _reach(prob, ubar, knot) - gap)


def barely_feasible_bounds(prob, ubar, knot, gap):
    """the same with + gap: feasible (the inputs that reach the smallest value satisfy it), the bound active or nearly so"""
    return _bounds(prob, ubar, knot, _reach(prob, ubar, knot) + gap)


def farkas_check(prob, bounds, dlam, dmu_x, dmu_u, eps):
    """The certificate test in longdouble. bounds = (xlo, xhi, ulo, uhi), each [N, n] / [N, m]; dlam, dmu_x [N, n],
    dmu_u [N, m]. Returns a dict: the four conditions `nonzero` (||dmu||_inf > 0), `stationary` (||e||_inf <= eps ||dmu||_inf),
    `qualified` (no entry points to an infinite bound with |dmu_i| > eps ||dmu||_inf) and `negative` (S < -eps ||dmu||_inf),
    `ok` (all four), and the numbers e_inf, dmu_inf, S."""
    ld = np.longdouble
    n, m, N = prob.n, prob.m, prob.N
    xlo, xhi, ulo, uhi = [np.asarray(a, dtype=float) for a in bounds]
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    lo = np.concatenate([np.where(Mx > 0, xlo, -np.inf), np.where(Mu > 0, ulo, -np.inf)], axis=1)
    hi = np.concatenate([np.where(Mx > 0, xhi, np.inf), np.where(Mu > 0, uhi, np.inf)], axis=1)
    A, B = matrices(prob)
    A, B = A.astype(ld), B.astype(ld)
    dl = np.asarray(dlam, dtype=ld).reshape(N, n)
    dm = np.concatenate([np.asarray(dmu_x, dtype=ld).reshape(N, n), np.asarray(dmu_u, dtype=ld).reshape(N, m)], axis=1)
    e = dm.copy()
    e[:, :n] -= dl
    for k in range(N - 1):
        e[k, :n] += A[k].T @ dl[k + 1]
        e[k, n:] += B[k].T @ dl[k + 1]
    e_inf = np.abs(e).max()
    d_inf = np.abs(dm).max()
    tol = ld(eps) * d_inf
    S = -(prob.x0.astype(ld) @ dl[0])
    for k in range(N - 1):
        S -= prob.d[k].astype(ld) @ dl[k + 1]
    qualified = True
    for k in range(N):
        for j in range(n + m):
            v = dm[k, j]
            if v == 0:
                continue
            side = hi[k, j] if v > 0 else lo[k, j]
            if np.isfinite(side):
                S += ld(side) * v
            elif abs(v) > tol:
                qualified = False
    finite = bool(np.isfinite(e_inf) and np.isfinite(d_inf) and np.isfinite(S))
    out = {"nonzero": bool(finite and d_inf > 0), "stationary": bool(finite and e_inf <= tol), "qualified": qualified and finite,
           "negative": bool(finite and S < -tol), "e_inf": float(e_inf), "dmu_inf": float(d_inf), "S": float(S)}
    out["ok"] = out["nonzero"] and out["stationary"] and out["qualified"] and out["negative"]
    return out


def admm_infeas_reference(prob, solve, xlo, xhi, ulo, uhi, rho, alpha, eps_abs, eps_rel, max_iter, every, eps=1e-4,
                          trace=None):
    """box_support.admm_reference (fixed penalty, the operation order of strict mode) with the certificate test at the
    iterations it >= 2, it % every == 0, behind the update and the convergence test of that iteration. Returns
    (status, iters, dlam [N, n], dmu_x [N, n], dmu_u [N, m]): status 1 converged, 2 max_iter, 4 certified at `iters` (the
    differences are those of that iteration; zeros otherwise). trace: a list that takes (it, dlam, dmu_x, dmu_u) of
    every check."""
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
    lam_prev, mu_prev = None, None
    zero = (np.zeros((N, n)), np.zeros((N, n)), np.zeros((N, m)))
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
        conv = r_prim <= eps_abs + eps_rel * max(mx(zx), mx(vn)) and r_dual <= eps_abs + eps_rel * (rho * mx(yn))
        v, y = vn, yn
        if conv:
            return (1, it) + zero
        lam, mu = Z[:, :n].copy(), rho * y
        if every > 0 and it >= 2 and it % every == 0:
            dlam, dmu = lam - lam_prev, mu - mu_prev
            c = farkas_check(prob, (xlo, xhi, ulo, uhi), dlam, dmu[:, :n], dmu[:, n:], eps)
            if trace is not None:
                trace.append((it, dlam, dmu[:, :n], dmu[:, n:]))
            if c["ok"]:
                return 4, it, dlam, dmu[:, :n], dmu[:, n:]
        lam_prev, mu_prev = lam, mu
        t = y - v
        t = rho * t
        qt = np.where(M, q + t, q)
    return (2, max_iter) + zero
