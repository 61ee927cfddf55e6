"""Independent references for the box-constrained batch solve (ndlqr_SolveBatchBoxConstrained).

- condensed(): the problem in the inputs alone, x = c + G U over the stacked inputs U, cost 1/2 U'HU + g'U + const.
- bvls_inputs(): input bounds only -- the exact bound-constrained least squares of the condensed problem (scipy's bvls),
  sharing no code with ADMM.
- certificate(): optimality of (z, mu) with state and input bounds, in extended precision: stationarity of the KKT
  operator with mu added (support.kkt_residual_ld on q + mu_x, r + mu_u), feasibility, sign and complementarity.
- active_set_qp(): the equality-constrained QP with an identified active set, solved densely.
- admm_reference(): a numpy restatement of the iteration, each solve by a caller-given solver (the oracle on the shifted
  problem), in the operation order of strict mode.
Test infrastructure.
"""
import numpy as np

from support import Problem, kkt_residual_ld


def blocks(z, n, m, N):
    out = np.zeros(N * (2 * n + m))
    out[: z.size] = z
    return out.reshape(N, 2 * n + m)


def split(z, n, m, N):
    """(lam [N, n], x [N, n], u [N-1, m]) of a solution vector in the reference's order"""
    Z = blocks(z, n, m, N)
    return Z[:, :n], Z[:, n:2 * n], Z[: N - 1, 2 * n:]


def matrices(prob):
    n, m, N = prob.n, prob.m, prob.N
    A = prob.A.reshape(N, n, n).transpose(0, 2, 1)  # column-major storage -> A[k][i, j]
    B = prob.B.reshape(N, m, n).transpose(0, 2, 1)
    return A, B


def condensed(prob):
    """(G [N, n, (N-1) m], c [N, n], H, g): x_k = c_k + G_k U, cost 1/2 U'HU + g'U + const."""
    n, m, N = prob.n, prob.m, prob.N
    A, B = matrices(prob)
    nu = (N - 1) * m
    G = np.zeros((N, n, nu))
    c = np.zeros((N, n))
    c[0] = prob.x0
    for k in range(N - 1):
        G[k + 1] = A[k] @ G[k]
        G[k + 1][:, k * m:(k + 1) * m] += B[k]
        c[k + 1] = A[k] @ c[k] + prob.d[k]
    H = np.diag(prob.R[: N - 1].reshape(-1)).astype(float)
    g = prob.r[: N - 1].reshape(-1).astype(float).copy()
    for k in range(N):
        H += G[k].T @ (prob.Q[k][:, None] * G[k])
        g += G[k].T @ (prob.Q[k] * c[k] + prob.q[k])
    return G, c, H, g


def bvls_inputs(prob, ulo, uhi):
    """Exact minimiser over U of the condensed cost subject to ulo <= u_k <= uhi (k = 0 .. N-2; arrays [N, m], the last row
    ignored): scipy.optimize.lsq_linear(L, -L^-T g, bounds, method="bvls") with H = L'L. Returns (u [N-1, m], x [N, n])."""
    from scipy.optimize import lsq_linear
    n, m, N = prob.n, prob.m, prob.N
    G, c, H, g = condensed(prob)
    Lc = np.linalg.cholesky(H)  # H = Lc Lc'
    b = -np.linalg.solve(Lc, g)
    lo = np.asarray(ulo, dtype=float)[: N - 1].reshape(-1)
    hi = np.asarray(uhi, dtype=float)[: N - 1].reshape(-1)
    res = lsq_linear(Lc.T, b, bounds=(lo, hi), method="bvls", tol=1e-15, max_iter=10000)
    U = np.clip(res.x, lo, hi)
    x = c + np.einsum("kij,j->ki", G, U)
    return U.reshape(N - 1, m), x


def shifted_problem(prob, rho, Mx, Mu, qt, rt):
    """the problem with Q + rho M_x, R + rho M_u and right-hand side q~, r~ (x0, d as they are)"""
    return Problem(prob.n, prob.m, prob.N, prob.A, prob.B, prob.Q + rho * Mx, prob.R + rho * Mu, qt, rt, prob.d, prob.x0)


def masks(n, m, N, xlo, xhi, ulo, uhi):
    """bounded pattern [N, n], [N, m] (x of knot 0 and u of the last knot never)"""
    Mx = (np.isfinite(xlo) | np.isfinite(xhi)).astype(float)
    Mu = (np.isfinite(ulo) | np.isfinite(uhi)).astype(float)
    Mx[0] = 0.0
    Mu[N - 1] = 0.0
    return Mx, Mu


def admm_reference(prob, solve, xlo, xhi, ulo, uhi, rho, alpha, eps_abs, eps_rel, max_iter, start=None, trace=None):
    """The iteration of DESIGN.md section 3.9 in the operation order of strict mode; solve(problem) -> z (nvars).
    start: (v, y) [N, n+m] of a warm start (box_start: the entries bounded now keep them, y of the others is zero and
    their v is not read); None: cold. trace: a list that gets one dict per iteration -- it, Z (the re-solve as blocks),
    v, y after the update, resid = (r_prim, r_dual, sp, sd) and conv (box_update_support.py reads it).
    Returns (x, u from v as [N, n], [N, m]; mu_x, mu_u; lam of the last solve; iters; status)."""
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
    if start is not None:
        v = np.where(M, start[0], 0.0)
        y = np.where(M, start[1], 0.0)
        t = y - v
        t = rho * t
        qt = np.where(M, q + t, q)
    status, it = 0, 0
    Z = None
    for it in range(1, max_iter + 1):
        z = solve(shifted_problem(prob, rho, Mx, Mu, np.ascontiguousarray(qt[:, :n]), np.ascontiguousarray(qt[:, n:])))
        Z = blocks(z, n, m, N)
        zx = Z[:, n:]
        zh = alpha * zx + oma * v
        vn = np.minimum(np.maximum(zh + y, lo), hi)
        yn = (y + zh) - vn
        vn = np.where(M, vn, 0.0)
        yn = np.where(M, yn, 0.0)
        mx = lambda a: float(np.abs(a[M]).max()) if M.any() else 0.0
        r_prim = mx(zx - vn)
        r_dual = rho * mx(vn - v)
        sp = max(mx(zx), mx(vn))
        sd = rho * mx(yn)
        conv = r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        if trace is not None:
            trace.append(dict(it=it, Z=Z.copy(), v=v.copy(), y=y.copy(), resid=(r_prim, r_dual, sp, sd), conv=bool(conv)))
        if conv:
            status = 1
            break
        t = y - v
        t = rho * t
        qt = np.where(M, q + t, q)
    xu = np.where(M, v, Z[:, n:])
    mu = rho * y
    return xu[:, :n], xu[:, n:], mu[:, :n], mu[:, n:], Z[:, :n], it, status or 2


def certificate(prob, z, mu_x, mu_u, xlo, xhi, ulo, uhi, tol):
    """Largest violation, relative to the scale of the problem, of: stationarity with mu added, the bounds, and sign /
    complementarity of mu (mu >= 0 only at an upper bound, <= 0 only at a lower one, 0 inside). Returns a dict."""
    n, m, N = prob.n, prob.m, prob.N
    p2 = Problem(n, m, N, prob.A, prob.B, prob.Q, prob.R, prob.q + mu_x, prob.r + mu_u, prob.d, prob.x0)
    r_lam, r_x, r_u = kkt_residual_ld(p2, z)
    _, x, u = split(z, n, m, N)
    scale = max(1.0, float(np.abs(z).max()), float(np.abs(mu_x).max()), float(np.abs(mu_u).max()))
    out = {"stationarity": float(max(np.abs(r_lam).max(), np.abs(r_x).max(), np.abs(r_u[: N - 1]).max())) / scale}
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    viol = 0.0
    for val, lo, hi, M in ((x, xlo, xhi, Mx), (u, ulo[: N - 1], uhi[: N - 1], Mu[: N - 1])):
        viol = max(viol, float(np.max(np.where(M > 0, np.maximum(lo - val, val - hi), -np.inf), initial=0.0)))
    out["bounds"] = viol
    comp = 0.0
    for val, lo, hi, mu in ((x, xlo, xhi, mu_x), (u, ulo[: N - 1], uhi[: N - 1], mu_u[: N - 1])):
        at_hi = np.abs(val - hi) <= tol * scale
        at_lo = np.abs(val - lo) <= tol * scale
        bad_pos = np.where(at_hi, 0.0, np.maximum(mu, 0.0))   # mu > 0 away from the upper bound
        bad_neg = np.where(at_lo, 0.0, np.maximum(-mu, 0.0))  # mu < 0 away from the lower bound
        comp = max(comp, float(bad_pos.max(initial=0.0)), float(bad_neg.max(initial=0.0)))
    out["complementarity"] = comp / scale
    return out


def active_set_qp(prob, xlo, xhi, ulo, uhi, x, u, mu_x, mu_u, tol):
    """The active set identified from (x, u, mu) -- entries at a bound within tol, or with |mu| > tol -- fixed as
    equalities at that bound; the resulting equality-constrained QP solved densely in the condensed inputs. Returns
    (u [N-1, m], x [N, n], number of active constraints)."""
    n, m, N = prob.n, prob.m, prob.N
    G, c, H, g = condensed(prob)
    nu = (N - 1) * m
    rows, rhs = [], []
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    for k in range(N - 1):
        for i in range(m):
            if Mu[k, i] == 0:
                continue
            e = np.zeros(nu)
            e[k * m + i] = 1.0
            sc = tol * max(1.0, abs(u[k, i]))
            if abs(u[k, i] - uhi[k, i]) <= sc or mu_u[k, i] > tol:
                rows.append(e); rhs.append(uhi[k, i])
            elif abs(u[k, i] - ulo[k, i]) <= sc or mu_u[k, i] < -tol:
                rows.append(e); rhs.append(ulo[k, i])
    for k in range(1, N):
        for i in range(n):
            if Mx[k, i] == 0:
                continue
            sc = tol * max(1.0, abs(x[k, i]))
            if abs(x[k, i] - xhi[k, i]) <= sc or mu_x[k, i] > tol:
                rows.append(G[k][i]); rhs.append(xhi[k, i] - c[k][i])
            elif abs(x[k, i] - xlo[k, i]) <= sc or mu_x[k, i] < -tol:
                rows.append(G[k][i]); rhs.append(xlo[k, i] - c[k][i])
    na = len(rows)
    if na:
        C = np.array(rows)
        K = np.block([[H, C.T], [C, np.zeros((na, na))]])
        sol = np.linalg.lstsq(K, np.concatenate([-g, rhs]), rcond=None)[0]
        U = sol[:nu]
    else:
        U = np.linalg.solve(H, -g)
    return U.reshape(N - 1, m), c + np.einsum("kij,j->ki", G, U), na
