"""Independent reference for the gradients through the solve with linear inequality constraints
(ndlqr_SolveBatchLinAdjoint, ndlqr_BatchConstraintGradients), on top of lin_support.py and
cost_support.py: numpy on the dense KKT system, in float64 or in longdouble (one code path: `dtype` decides).

- codes_of(): the row codes from a forward's projected iterate v and the bounds (0 unbounded, 1 free, 2 at lo, 3 at hi;
  exact comparison, as the device does).
- active_rows(): G_A, the active rows of [C D] as a dense matrix on the packed vector, and their (knot, row) list.
- direct(): the active-set system [K G_A'; G_A 0] [x; mult] = [rhs; c] solved directly, refined in longdouble.
- adjoint_admm(): the adjoint's iteration restated -- lin_support.admm with the codes in place of the bounds.
- constraint_grads(): dL/d(C, D, lo, hi) from z*, w, mu, nu and the codes; cost_support.gradient_reference has the nine
  others.
- seeded_g(), case(): the shared, read-only references of one (shape, horizon).
Test infrastructure.
"""
import functools

import numpy as np

import cost_support as cs
import lin_support as ls

EPS = np.finfo(float).eps
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5)]
CASES = [(n, m, N) for (n, m) in SHAPES for N in (2, 5, 8, 16)]
# the four forwards the float64 restatement ends as status 2 at rho = 1 within 2000 iterations: (n, m, N) -> problems
NOT_CONVERGED = {(12, 4, 2): (1, 2), (20, 5, 2): (0, 2)}


def skipped(n, m, N, i):
    """is problem i of the case one of the four whose forward does not converge (value checks leave it out, by name)?"""
    return i in NOT_CONVERGED.get((n, m, N), ())


def codes_of(v, lo, hi):
    M = np.isfinite(lo) | np.isfinite(hi)
    return np.where(~M, 0, np.where(v == hi, 3, np.where(v == lo, 2, 1))).astype(np.uint8)


def active_rows(p, C, D, codes, dtype=np.float64):
    """(G_A [na, nvars] in dtype, act: list of (k, r)) -- row (k, r) of G = [C D] as it acts on the packed vector"""
    n, m, N = cs.dims(p)
    act = [(int(k), int(r)) for k, r in np.argwhere(codes >= 2)]
    nv = N * (2 * n + m) - m
    G = np.zeros((len(act), nv), dtype)
    for a, (k, r) in enumerate(act):
        t = np.zeros(codes.shape, dtype)
        t[k, r] = 1
        G[a] = ls.perturbation(p, C, D, t)
    return G, act


def bordered(p, C, D, codes, dtype=np.float64):
    """(the active-set KKT matrix [K G_A'; G_A 0] in dtype, b, act)"""
    pl = {k: np.asarray(p[k], dtype=dtype) for k in cs.NAMES}
    K, b = ls.kkt_ld(pl)
    G, act = active_rows(p, C, D, codes, dtype)
    na = len(act)
    KK = np.zeros((K.shape[0] + na, K.shape[0] + na), dtype)
    KK[: K.shape[0], : K.shape[0]] = K
    KK[: K.shape[0], K.shape[0]:] = G.T
    KK[K.shape[0]:, : K.shape[0]] = G
    return KK, b, act


def scatter(act, vals, shape, dtype):
    out = np.zeros(shape, dtype)
    for (k, r), val in zip(act, vals):
        out[k, r] = val
    return out


def direct(p, C, D, codes, rhs, c=None, dtype=np.float64):
    """(x [nvars], mult [N, p]) of K x + G_A' mult = rhs, G_A x = c (None: 0; else [N, p], read on the active rows)"""
    KK, _, act = bordered(p, C, D, codes, dtype)
    nv = KK.shape[0] - len(act)
    full = np.zeros(KK.shape[0], dtype)
    full[:nv] = rhs
    if c is not None:
        full[nv:] = [c[k, r] for k, r in act]
    sol = ls.Solver(KK)(full)
    return sol[:nv], scatter(act, sol[nv:], codes.shape, dtype)


def adjoint_admm(p, C, D, lo, hi, codes, g, rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=2000,
                 dtype=np.float64, trace=None):
    """The adjoint's iteration: lin_support.admm on the same shifted matrix with the right-hand
    side g, lo = hi = 0 on the fixed rows (codes 2, 3) and the identity as the clip of the free ones (code 1). Returns
    dict(w, v, y, nu, iters, status, resid); trace as for lin_support.admm (its z is w)."""
    M = codes > 0
    fixed = codes >= 2
    ps = ls.shifted_problem(p, C, D, lo, hi, rho, dtype)
    K, _ = ls.kkt_ld(ps)
    solve = ls.Solver(K)
    g_ = np.asarray(g, dtype=dtype)
    rho_, alpha_ = dtype(rho), dtype(alpha)
    oma = dtype(1.0 - alpha)
    v = np.zeros(codes.shape, dtype)
    y = np.zeros_like(v)
    mx = lambda a: a.dtype.type(np.abs(a).max()) if a.size else dtype(0)
    status, it, w, resid = 0, 0, None, None
    for it in range(1, max_iter + 1):
        w = solve(g_ - ls.perturbation(p, C, D, np.where(M, rho_ * (y - v), 0).astype(dtype)))
        s = ls.rows_of(p, C, D, w)
        sh = alpha_ * s + oma * v
        t = sh + y
        vn = np.where(M, np.where(fixed, np.minimum(np.maximum(t, 0), 0), t), 0).astype(dtype)
        yn = np.where(M, (y + sh) - vn, 0).astype(dtype)
        gd = ls.perturbation(p, C, D, vn - v)
        gy = ls.perturbation(p, C, D, yn)
        r_prim = mx((s - vn)[M])
        r_dual = rho_ * mx(gd)
        sp = max(mx(s[M]), mx(vn[M]))
        sd = rho_ * mx(gy)
        resid = (r_prim, r_dual, sp, sd)
        finite = all(np.isfinite(float(a)) for a in resid)
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        if trace is not None:
            trace.append(dict(it=it, z=w.copy(), v=v.copy(), y=y.copy(), resid=resid))
        if conv or not finite:
            status = 1 if conv else 3
            break
    return dict(w=w, v=v, y=y, nu=np.where(fixed, rho_ * y, 0), iters=it, status=status or 2, resid=resid)


def constraint_grads(p, codes, z, w, mu, nu):
    """dict C [N, p, n], D [N, p, m], lo, hi [N, p] (math convention) in the dtype of z: row r of knot k gives
    -(mu_r w_x' + nu_r x') and -(mu_r w_u' + nu_r u'), zero outside the active set and for D of knot N-1; nu goes to hi
    on code 3, to lo on code 2."""
    n, m, N = cs.dims(p)
    _, x, u = cs.split(z, n, m, N)
    _, wx, wu = cs.split(w, n, m, N)
    act = codes >= 2
    mu_ = np.where(act, mu, 0).astype(z.dtype)
    nu_ = np.where(act, nu, 0).astype(z.dtype)
    gC = -(mu_[:, :, None] * wx[:, None, :] + nu_[:, :, None] * x[:, None, :])
    gD = -(mu_[:, :, None] * wu[:, None, :] + nu_[:, :, None] * u[:, None, :])
    gD[N - 1] = 0
    return dict(C=gC, D=gD, lo=np.where(codes == 2, nu_, 0), hi=np.where(codes == 3, nu_, 0))


def seeded_g(n, m, N, i):
    """g of problem i of a case: standard normal over the whole packed vector, lambda rows included"""
    return np.random.default_rng([n, m, N, i, 23]).standard_normal(N * (2 * n + m) - m)


@functools.lru_cache(maxsize=None)
def case(n, m, N):
    """The shared, read-only reference of one (shape, horizon): the entries of lin_support.case, each with its seeded g,
    the codes of the float64 forward, the float64 adjoint restatement run to eps = 1e-8 within 2000 iterations (with its
    first three iterates) and -- where the forward converged -- the direct active-set solve w_direct, nu_direct and
    |M_A^-1|_inf, the smallest-to-largest singular value ratio of the active-set KKT matrix."""
    out = []
    for i, c in enumerate(ls.case(n, m, N)):
        g = seeded_g(n, m, N, i)
        codes = codes_of(c["ref"]["v"], c["lo"], c["hi"])
        e = dict(c, g=g, codes=codes)
        if c["ref"]["status"] == 1:
            trace = []
            e["adj"] = adjoint_admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], codes, g, trace=trace)
            e["adj_first"] = trace[:3]
            e["w_direct"], e["nu_direct"] = direct(c["p"], c["C"], c["D"], codes, g)
            KK, _, _ = bordered(c["p"], c["C"], c["D"], codes)
            sv = np.linalg.svd(KK, compute_uv=False)
            e["sv_ratio"] = float(sv[-1] / sv[0])
            e["inv_norm"] = float(np.abs(np.linalg.inv(KK)).sum(axis=1).max())
        out.append(e)
    return out


def adjoint_bar(c, w, resid, rho=ls.RHO, alpha=ls.ALPHA):
    """What a converged adjoint iterate may leave of K w + G'nu = g and G_A w = 0, from its residual row: the bounds of
    lin_support.kkt_bar (stationarity, feasibility) with w in the place of z, and their sum times |M_A^-1|_inf: the bar on
    |w - w_direct|_inf."""
    bar = ls.kkt_bar(c["p"], c["C"], c["D"], w, resid, rho, alpha)
    return dict(bar, w=c["inv_norm"] * (bar["stationarity"] + bar["feasibility"]))

