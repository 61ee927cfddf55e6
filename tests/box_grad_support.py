"""Independent references for the gradients through the box-constrained solve (ndlqr_SolveBatchBoxAdjoint,
ndlqr_BatchBoundGradients).

- kkt_sparse(): the KKT matrix K and right-hand side b of one problem (scipy.sparse), in the solution order [lam x u].
- active_codes(): the entry codes of the box adjoint from a constrained solution and its bounds (0 unbounded, 1 free,
  2 at the lower bound, 3 at the upper one; exact comparison, as the device does).
- active_adjoint(): the adjoint of the active-set system, [K E'; E 0] [w; nu] = [g; 0], solved directly.
- active_forward(): the equality-constrained forward, [K E'; E 0] [z; mu] = [b; c_A], solved directly.
- adjoint_admm_reference(): a numpy restatement of the box adjoint's iteration, each solve by a caller-given solver (the
  oracle on the shifted adjoint problem), in the operation order of strict mode.
- bound_grads(): nu split onto dL/d(xlo, xhi, ulo, uhi) by the codes.
Test infrastructure.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from box_support import blocks, masks, shifted_problem
from support import Problem


def kkt_sparse(prob):
    """(K, b): K z = b is the reference's KKT system (support.kkt_residual_ld gives b - K z)."""
    n, m, N = prob.n, prob.m, prob.N
    zb = 2 * n + m
    nv = zb * N - m
    A = prob.A.reshape(N, n, n).transpose(0, 2, 1)  # column-major storage -> A[k][i, j]
    B = prob.B.reshape(N, m, n).transpose(0, 2, 1)
    rows, cols, vals = [], [], []

    def put(r0, c0, M, sym=True):
        M = np.atleast_2d(M)
        ii, jj = np.nonzero(M != 0) if M.size > 1 else (np.array([0]), np.array([0]))
        for i, j in zip(ii, jj):
            rows.append(r0 + i); cols.append(c0 + j); vals.append(M[i, j])
            if sym:
                rows.append(c0 + j); cols.append(r0 + i); vals.append(M[i, j])

    b = np.zeros(nv)
    put(0, n, -np.eye(n))
    b[0:n] = -prob.x0
    for k in range(N):
        lo, xo, uo = k * zb, k * zb + n, k * zb + 2 * n
        put(xo, xo, np.diag(prob.Q[k]), sym=False)
        b[xo:xo + n] = -prob.q[k]
        if k == N - 1:
            break
        l1, x1 = (k + 1) * zb, (k + 1) * zb + n
        put(uo, uo, np.diag(prob.R[k]), sym=False)
        b[uo:uo + m] = -prob.r[k]
        put(l1, xo, A[k])
        put(l1, uo, B[k])
        put(l1, x1, -np.eye(n))
        b[l1:l1 + n] = -prob.d[k]
    K = sp.csc_matrix((vals, (rows, cols)), shape=(nv, nv))
    return K, b


def entry_index(n, m, N):
    """[N, n+m] -> index into the solution vector (-1 for u of the last knot)"""
    zb = 2 * n + m
    idx = np.zeros((N, n + m), dtype=np.int64)
    for k in range(N):
        idx[k, :n] = k * zb + n + np.arange(n)
        idx[k, n:] = k * zb + 2 * n + np.arange(m) if k < N - 1 else -1
    return idx


def full_bounds(n, m, N, xlo, xhi, ulo, uhi):
    """lo, hi [N, n+m] with -inf / inf where unbounded (x of knot 0, u of the last knot never bounded)"""
    inf = lambda k: np.full((N, k), np.inf)
    xlo = -inf(n) if xlo is None else np.asarray(xlo, dtype=float)
    xhi = inf(n) if xhi is None else np.asarray(xhi, dtype=float)
    ulo = -inf(m) if ulo is None else np.asarray(ulo, dtype=float)
    uhi = inf(m) if uhi is None else np.asarray(uhi, dtype=float)
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    M = np.concatenate([Mx, Mu], axis=1) > 0
    lo = np.where(M, np.concatenate([xlo, ulo], axis=1), -np.inf)
    hi = np.where(M, np.concatenate([xhi, uhi], axis=1), np.inf)
    return lo, hi, M


def active_codes(prob, z, xlo, xhi, ulo, uhi):
    """codes [N, n+m] of the box adjoint from the constrained solution z (its x, u are the projected iterate)"""
    n, m, N = prob.n, prob.m, prob.N
    lo, hi, M = full_bounds(n, m, N, xlo, xhi, ulo, uhi)
    Z = blocks(z, n, m, N)
    v = Z[:, n:]
    return np.where(~M, 0, np.where(v == hi, 3, np.where(v == lo, 2, 1))).astype(np.int8)


def _bordered(prob, codes):
    n, m, N = prob.n, prob.m, prob.N
    K, b = kkt_sparse(prob)
    idx = entry_index(n, m, N)
    act = np.argwhere(codes >= 2)
    cols = np.array([idx[k, j] for k, j in act], dtype=np.int64)
    na = cols.size
    E = sp.csc_matrix((np.ones(na), (np.arange(na), cols)), shape=(na, K.shape[0]))
    KK = sp.bmat([[K, E.T], [E, None]], format="csc")
    return KK, b, act


def _nu_blocks(prob, act, nu):
    n, m, N = prob.n, prob.m, prob.N
    out = np.zeros((N, n + m))
    for (k, j), val in zip(act, nu):
        out[k, j] = val
    return out


def active_adjoint(prob, codes, g):
    """(w [nvars], nu [N, n+m]) of K w + E_A' nu = g, E_A w = 0 (A: codes 2, 3)"""
    KK, _, act = _bordered(prob, codes)
    nv = g.size
    sol = spla.spsolve(KK, np.concatenate([g, np.zeros(len(act))]))
    return sol[:nv], _nu_blocks(prob, act, sol[nv:])


def active_forward(prob, codes, xlo, xhi, ulo, uhi):
    """(z [nvars], mu [N, n+m]) of K z + E_A' mu = b, E_A z = c_A"""
    n, m, N = prob.n, prob.m, prob.N
    KK, b, act = _bordered(prob, codes)
    lo, hi, _ = full_bounds(n, m, N, xlo, xhi, ulo, uhi)
    c = np.array([hi[k, j] if codes[k, j] == 3 else lo[k, j] for k, j in act])
    sol = spla.spsolve(KK, np.concatenate([b, c]))
    return sol[: b.size], _nu_blocks(prob, act, sol[b.size:])


def bound_grads(codes, nu, n):
    """dict xlo, xhi, ulo, uhi -> [N, n] / [N, m]: nu where the code says that bound, 0 elsewhere"""
    lo = np.where(codes == 2, nu, 0.0)
    hi = np.where(codes == 3, nu, 0.0)
    return {"xlo": lo[:, :n], "xhi": hi[:, :n], "ulo": lo[:, n:], "uhi": hi[:, n:]}


def adjoint_problem(prob, g):
    """the problem whose right-hand side is g (same A, B, Q, R): x0' = -g_lam0, q' = -g_x, r' = -g_u, d' = -g_lam(k+1)"""
    n, m, N = prob.n, prob.m, prob.N
    G = blocks(g, n, m, N)
    r = -G[:, 2 * n:]
    r[N - 1] = 0.0
    d = np.zeros((N, n))
    d[: N - 1] = -G[1:, :n]
    return Problem(n, m, N, prob.A, prob.B, prob.Q, prob.R, -G[:, n:2 * n], r, d, -G[0, :n])


def adjoint_admm_reference(prob, solve, codes, g, rho, alpha, eps_abs, eps_rel, max_iter, trace=None):
    """The box adjoint's iteration in the operation order of strict mode: box_support's
    admm_reference on the adjoint problem with lo = hi = 0 on the fixed entries (codes 2, 3) and the identity as the clip
    of the free ones (code 1). trace: as for admm_reference. Returns (w [nvars], nu [N, n+m], iters, status)."""
    n, m, N = prob.n, prob.m, prob.N
    ap = adjoint_problem(prob, g)
    M = codes > 0
    fixed = codes >= 2
    Mx, Mu = M[:, :n].astype(float), M[:, n:].astype(float)
    lo = np.where(fixed, 0.0, -np.inf)
    hi = np.where(fixed, 0.0, np.inf)
    q = np.concatenate([ap.q, ap.r], axis=1)
    v = np.zeros((N, n + m))
    y = np.zeros((N, n + m))
    oma = 1.0 - alpha
    qt = q.copy()
    status, it = 0, 0
    Z = None
    for it in range(1, max_iter + 1):
        z = solve(shifted_problem(ap, rho, Mx, Mu, np.ascontiguousarray(qt[:, :n]), np.ascontiguousarray(qt[:, n:])))
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
    W = Z.copy()
    W[:, n:] = np.where(M, v, Z[:, n:])
    w = W.reshape(-1)[: prob.nvars]
    return w, rho * y, it, status or 2
