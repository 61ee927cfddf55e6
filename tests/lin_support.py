"""Independent reference for the solve with linear inequality constraints lo <= C x + D u <= hi
(ndlqr_SolveBatchLinConstrained): a numpy restatement of the iteration on the dense KKT system of
cost_support.dense_kkt, in float64 or in longdouble (one code path: `dtype` decides).

- constraint_rows(): the seeded rows of the tests -- the m input rows (C = 0, D = I) plus two dense rows with entries
  N(0,1)/sqrt(n) and N(0,1)/sqrt(m) -- with bounds +-0.6 x the largest |w| of the unconstrained solution, per row.
- selector_rows(): rows that select every x and u entry (the box special case).
- shifted_problem(): the problem with Q + rho C'MC, H + rho C'MD, R + rho D'MD.
- admm(): the iteration. Every re-solve is K^ z = b^ on the shifted dense KKT matrix in the caller's variables -- what the
  device computes as S^ K~^-1 S^' b^ --, by an LU in float64, refined against the longdouble matrix when dtype is longdouble.
- kkt_violation(): the KKT conditions of the constrained QP for (z, mu).
Test infrastructure.
"""
import functools

import numpy as np
import scipy.linalg as sla

import cost_support as cs

RHO, ALPHA = 1.0, 1.6


def rows_of(p, C, D, z):
    """w [N, p] = C x + D u of a packed solution (knot N-1: C x), in the dtype of z"""
    n, m, N = cs.dims(p)
    _, x, u = cs.split(z, n, m, N)
    w = np.einsum("krj,kj->kr", C.astype(z.dtype), x)
    w[: N - 1] += np.einsum("krj,kj->kr", D[: N - 1].astype(z.dtype), u[: N - 1])
    return w


def constraint_rows(p, z_unc, seed):
    """(C [N, p, n], D [N, p, m], lo, hi [N, p]) with p = m + 2 for the problem `p` whose unconstrained solution is z_unc"""
    n, m, N = cs.dims(p)
    rng = np.random.default_rng([seed, n, m, N, 17])
    C = np.zeros((N, m + 2, n))
    D = np.zeros((N, m + 2, m))
    D[:, :m, :] = np.eye(m)
    C[:, m:, :] = rng.standard_normal((N, 2, n)) / np.sqrt(n)
    D[:, m:, :] = rng.standard_normal((N, 2, m)) / np.sqrt(m)
    w = rows_of(p, C, D, np.asarray(z_unc, dtype=np.float64))
    bound = 0.6 * np.abs(w).max(axis=0)  # per row, over the knots
    hi = np.broadcast_to(bound, (N, m + 2)).copy()
    return C, D, -hi, hi


def selector_rows(n, m, N, xlo, xhi, ulo, uhi):
    """rows w = [x; u]: C = [I; 0], D = [0; I]; bounds as box_support.masks leaves them (x of knot 0, u of knot N-1 never)"""
    C = np.zeros((N, n + m, n))
    D = np.zeros((N, n + m, m))
    C[:, :n, :] = np.eye(n)
    D[:, n:, :] = np.eye(m)
    lo = np.concatenate([xlo, ulo], axis=1).astype(float)
    hi = np.concatenate([xhi, uhi], axis=1).astype(float)
    lo[0, :n] = -np.inf; hi[0, :n] = np.inf
    lo[N - 1, n:] = -np.inf; hi[N - 1, n:] = np.inf
    return C, D, lo, hi


def shifted_problem(p, C, D, lo, hi, rho, dtype=np.float64):
    """the problem dict with the shifted costs, in `dtype` (knot N-1: Q alone)"""
    n, m, N = cs.dims(p)
    M = (np.isfinite(lo) | np.isfinite(hi)).astype(dtype)
    out = {k: np.asarray(p[k], dtype=dtype).copy() for k in cs.NAMES}
    Cd, Dd = C.astype(dtype), D.astype(dtype)
    rho = dtype(rho)
    for k in range(N):
        CM = Cd[k].T * (rho * M[k])
        out["Q"][k] = 0.5 * (out["Q"][k] + out["Q"][k].T) + CM @ Cd[k]
        if k < N - 1:
            out["H"][k] = out["H"][k] + CM @ Dd[k]
            out["R"][k] = 0.5 * (out["R"][k] + out["R"][k].T) + (Dd[k].T * (rho * M[k])) @ Dd[k]
    return out


def kkt_ld(p):
    """(K, b) of cost_support.dense_kkt assembled from a problem dict of any dtype, in that dtype: the structure (the
    entries 0 and +-1 and the positions) from the float64 assembly, the cost blocks and the right-hand side added in dtype"""
    n, m, N = cs.dims(p)
    dtype = p["Q"].dtype
    zero = {k: np.zeros_like(np.asarray(p[k], dtype=np.float64)) for k in ("Q", "H", "R", "q", "r", "d", "x0")}
    base = dict(A=np.asarray(p["A"], dtype=np.float64), B=np.asarray(p["B"], dtype=np.float64), **zero)
    K0, _ = cs.dense_kkt(base)
    # the A, B entries in dtype: K0 holds them rounded to float64, which they are (the inputs are float64 data)
    K = K0.astype(dtype)
    b = np.zeros(K.shape[0], dtype)
    zb = 2 * n + m
    b[:n] = -p["x0"]
    for k in range(N):
        xo, uo = k * zb + n, k * zb + 2 * n
        K[xo:xo + n, xo:xo + n] += 0.5 * (p["Q"][k] + p["Q"][k].T)
        b[xo:xo + n] = -p["q"][k]
        if k == N - 1:
            break
        K[uo:uo + m, uo:uo + m] += 0.5 * (p["R"][k] + p["R"][k].T)
        K[xo:xo + n, uo:uo + m] += p["H"][k]
        K[uo:uo + m, xo:xo + n] += p["H"][k].T
        b[uo:uo + m] = -p["r"][k]
        l1 = (k + 1) * zb
        b[l1:l1 + n] = -p["d"][k]
    return K, b


class Solver:
    """K^-1 g in the dtype of K: an LU of float64(K); for longdouble refined with residuals against K itself"""

    def __init__(self, K):
        self.K = K
        self.lu = sla.lu_factor(np.asarray(K, dtype=np.float64))

    def __call__(self, g):
        if self.K.dtype == np.float64:
            return sla.lu_solve(self.lu, g)
        z = sla.lu_solve(self.lu, np.asarray(g, dtype=np.float64)).astype(np.longdouble)
        for _ in range(5):
            r = g - self.K @ z
            z = z + sla.lu_solve(self.lu, np.asarray(r, dtype=np.float64))
        return z


def perturbation(p, C, D, t):
    """the packed vector with C' t in the x rows and D' t in the u rows (knot N-1: C' t alone); t [N, p]"""
    n, m, N = cs.dims(p)
    dt = t.dtype
    px = np.einsum("krj,kr->kj", C.astype(dt), t)
    pu = np.einsum("krj,kr->kj", D.astype(dt), t)
    pu[N - 1] = 0
    return cs.join(np.zeros((N, n), dt), px, pu)


def admm(p, C, D, lo, hi, rho=RHO, alpha=ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=2000, dtype=np.float64, start=None,
         trace=None):
    """The iteration of DESIGN.md section 3.17. Returns dict(z, v, y, mu, iters, status, resid). trace: a list that gets one
    dict per iteration (it, z, v, y, resid). start: (v, y) of a warm start."""
    n, m, N = cs.dims(p)
    M = np.isfinite(lo) | np.isfinite(hi)
    ps = shifted_problem(p, C, D, lo, hi, rho, dtype)
    K, b = kkt_ld(ps)
    solve = Solver(K)
    rho_, alpha_ = dtype(rho), dtype(alpha)
    oma = dtype(1.0 - alpha)  # (1 - alpha computed once in double, as the host does)
    lo_, hi_ = lo.astype(dtype), hi.astype(dtype)
    v = np.zeros((N, C.shape[1]), dtype)
    y = np.zeros_like(v)
    if start is not None:
        v = np.where(M, start[0], 0).astype(dtype)
        y = np.where(M, start[1], 0).astype(dtype)
    mx = lambda a: a.dtype.type(np.abs(a).max()) if a.size else dtype(0)
    status, it, z, resid = 0, 0, None, None
    for it in range(1, max_iter + 1):
        z = solve(b - perturbation(p, C, D, np.where(M, rho_ * (y - v), 0).astype(dtype)))
        w = rows_of(p, C, D, z)
        wh = alpha_ * w + oma * v
        vn = np.where(M, np.minimum(np.maximum(wh + y, lo_), hi_), 0).astype(dtype)
        yn = np.where(M, (y + wh) - vn, 0).astype(dtype)
        gd = perturbation(p, C, D, vn - v)
        gy = perturbation(p, C, D, yn)
        r_prim = mx((w - vn)[M])
        r_dual = rho_ * mx(gd)
        sp = max(mx(w[M]), mx(vn[M]))
        sd = rho_ * mx(gy)
        resid = (r_prim, r_dual, sp, sd)
        finite = all(np.isfinite(float(a)) for a in resid)
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        if trace is not None:
            trace.append(dict(it=it, z=z.copy(), v=v.copy(), y=y.copy(), resid=resid))
        if conv or not finite:
            status = 1 if conv else 3
            break
    return dict(z=z, v=v, y=y, mu=rho_ * y, iters=it, status=status or 2, resid=resid)


def kkt_violation(p, C, D, lo, hi, z, mu, tol):
    """Largest violation of the KKT conditions of the constrained QP by (z, mu), evaluated in longdouble:
    stationarity |K z - b + G' mu| (G = [C D] on the x and u rows), feasibility of w = C x + D u, and sign /
    complementarity of mu (mu > 0 only where w is within tol of hi, mu < 0 only within tol of lo). A dict."""
    pl = {k: np.asarray(p[k], dtype=np.longdouble) for k in cs.NAMES}
    K, b = kkt_ld(pl)
    zl = np.asarray(z, dtype=np.longdouble)
    mul = np.asarray(mu, dtype=np.longdouble)
    stat = K @ zl - b + perturbation(p, C, D, mul)
    w = rows_of(p, C, D, zl)
    feas = float(np.max(np.maximum(lo - w, w - hi), initial=0.0))
    at_hi = np.abs(w - hi) <= tol
    at_lo = np.abs(w - lo) <= tol
    comp = max(float(np.where(at_hi, 0, np.maximum(mul, 0)).max(initial=0.0)),
               float(np.where(at_lo, 0, np.maximum(-mul, 0)).max(initial=0.0)))
    return dict(stationarity=float(np.abs(stat).max()), feasibility=feas, complementarity=comp)


def kkt_bar(p, C, D, z, resid, rho=RHO, alpha=ALPHA, cond=1e3):
    """What a converged iterate may leave of the KKT conditions, from its residual row (r_prim, r_dual, sp, sd). The
    re-solve satisfies K z - b = -rho G'M(w + y - v), so with mu = rho y+ and y+ = y + alpha w + (1 - alpha) v - v+
        K z - b + G' mu = (alpha - 1) rho G'M(w - v+) + (alpha - 2) rho G'M(v+ - v):
    at most |alpha - 1| rho c r_prim + |2 - alpha| r_dual per entry, c the largest absolute column sum of G = [C D]. On top
    comes the rounding of the delivered z: a solve of condition `cond` (the family's) leaves |K| |z| cond eps per entry, taken
    64 times. Feasibility: v+ is feasible and |w - v+| <= r_prim. Complementarity: y+ != 0 only where v+ sits on the bound,
    so w is within r_prim of it (`tol`); both with the same rounding of w added."""
    r_prim, r_dual, sp, _ = (float(a) for a in resid)
    eps = np.finfo(np.float64).eps
    colsum = max(float(np.abs(C).sum(axis=1).max()), float(np.abs(D).sum(axis=1).max()))
    kmax = max(float(np.abs(p[k]).max()) for k in ("A", "B", "Q", "H", "R"))
    zmax = float(np.abs(z).max())
    rounding = 64 * cond * eps * max(1.0, kmax) * zmax
    w_round = 64 * cond * eps * max(1.0, colsum) * zmax
    return dict(stationarity=abs(alpha - 1) * rho * colsum * r_prim + abs(2 - alpha) * r_dual + rounding,
                feasibility=r_prim + w_round, tol=r_prim + w_round)


@functools.lru_cache(maxsize=None)
def case(n, m, N, name="moderate"):
    """The shared, read-only reference of one (shape, horizon): the problems of cost_support.family, their constraint rows,
    and the float64 restatement run to eps = 1e-8 within 2000 iterations (with its first three iterates)."""
    fam = cs.family(n, m, N, name)
    out = []
    for i, p in enumerate(fam["probs"]):
        C, D, lo, hi = constraint_rows(p, fam["z"][i], 300 + i)
        trace = []
        ref = admm(p, C, D, lo, hi, trace=trace)
        out.append(dict(p=p, C=C, D=D, lo=lo, hi=hi, ref=ref, first=trace[:3]))
    return out


def flat_rows(cases):
    """list of case() entries -> C [batch, N, p*n], D [batch, N, p*m] column-major per knot, lo, hi [batch, N, p]"""
    col = lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1))
    return (col(np.stack([c["C"] for c in cases])), col(np.stack([c["D"] for c in cases])),
            np.ascontiguousarray(np.stack([c["lo"] for c in cases])), np.ascontiguousarray(np.stack([c["hi"] for c in cases])))
