"""Independent references for the dense-cost reduction (ndlqr_InitializeBatchFlatDense).

A dense-cost problem is a dict of arrays in the ordinary math convention: A [N, n, n], B [N, n, m], Q [N, n, n],
H [N, n, m], R [N, m, m], q [N, n], r [N, m], d [N, n], x0 [n] (A, B, H, R, r, d of knot N-1 are not part of it).

- dense_problem(): the seeded families -- Q' = Q - H R^-1 H' and R with random orthogonal bases and a log-spaced spectrum
  of a given condition number, H = 0.3 randn, Q = Q' + H R^-1 H'.
- flat(): a list of problems in the flat layout of BatchSolver.initialize_flat_dense (column-major per knot).
- dense_kkt(): K and b of one problem -- box_grad_support.kkt_sparse plus the H blocks and the full Q, R -- in the
  solution order [lam x u], signs of support.kkt_residual_ld.
- refined_solve(): K^-1 g by a dense LU, refined with residuals in longdouble (as support.refined_solution does).
- reduce(): the reduction restated in numpy, in float64 or longdouble (one code path: the dtype of the input decides).
- apply_S(), apply_St(): z = S z~ and g~ = S' g on packed vectors.
Test infrastructure.
"""
import functools

import numpy as np
import scipy.linalg as sla

import rslqr_amd
from box_grad_support import kkt_sparse
from support import Problem

FAMILIES = {"moderate": 1e3, "hard": 1e6}
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5), (32, 8)]
HORIZONS = [2, 5, 8, 16]
BATCH = 3
NAMES = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")


def _spd(rng, k, cond):
    """random orthogonal basis, log-spaced spectrum of condition number `cond` around 1"""
    U, _ = np.linalg.qr(rng.standard_normal((k, k)))
    h = 0.5 * np.log10(cond)
    ev = np.logspace(-h, h, k) if k > 1 else np.ones(1)
    M = (U * ev) @ U.T
    return 0.5 * (M + M.T)


def dense_problem(n, m, N, cond, seed):
    """One problem of the family with cond(Q'_k) = cond(R_k) = cond; A, B, q, r, d, x0 those of the synthetic generator."""
    g = rslqr_amd.generate_synthetic(n, m, N, seed)
    rng = np.random.default_rng([seed, n, m, N])
    p = dict(A=g["A"].reshape(N, n, n).transpose(0, 2, 1).copy(), B=g["B"].reshape(N, m, n).transpose(0, 2, 1).copy(),
             q=g["q"].copy(), r=g["r"].copy(), d=g["d"].copy(), x0=g["x0"].copy(),
             Q=np.zeros((N, n, n)), H=np.zeros((N, n, m)), R=np.zeros((N, m, m)))
    for k in range(N):
        Qp = _spd(rng, n, cond)
        p["R"][k] = _spd(rng, m, cond)
        p["H"][k] = 0.3 * rng.standard_normal((n, m))
        if k < N - 1:
            Qk = Qp + p["H"][k] @ np.linalg.solve(p["R"][k], p["H"][k].T)
            p["Q"][k] = 0.5 * (Qk + Qk.T)
        else:
            p["Q"][k] = Qp
    return p


def diagonal_problem(n, m, N, seed):
    """The synthetic generator's diagonal-cost problem as a dense one (H = 0), and its diagonals (Qd [N, n], Rd [N, m])."""
    g = rslqr_amd.generate_synthetic(n, m, N, seed)
    p = dict(A=g["A"].reshape(N, n, n).transpose(0, 2, 1).copy(), B=g["B"].reshape(N, m, n).transpose(0, 2, 1).copy(),
             q=g["q"].copy(), r=g["r"].copy(), d=g["d"].copy(), x0=g["x0"].copy(),
             Q=np.stack([np.diag(v) for v in g["Q"]]), H=np.zeros((N, n, m)), R=np.stack([np.diag(v) for v in g["R"]]))
    return p, g["Q"].copy(), g["R"].copy()


def flat(probs, names=NAMES):
    """list of problems -> tuple of [batch, N, ..] arrays (x0 [batch, n]) in the flat layout, matrices column-major"""
    out = []
    for k in names:
        a = np.stack([p[k] for p in probs])
        if a.ndim == 4:
            a = a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1)
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    return tuple(out)


def dims(p):
    N, n, m = p["B"].shape
    return n, m, N


def dense_kkt(p):
    """(K [nvars, nvars] dense float64, b [nvars]) of the dense-cost problem"""
    n, m, N = dims(p)
    zb = 2 * n + m
    col = lambda M: M.transpose(0, 2, 1).reshape(N, -1)
    base = Problem(n, m, N, col(p["A"]), col(p["B"]), np.zeros((N, n)), np.zeros((N, m)), p["q"], p["r"], p["d"], p["x0"])
    Ks, b = kkt_sparse(base)
    K = Ks.toarray()
    for k in range(N):
        xo, uo = k * zb + n, k * zb + 2 * n
        K[xo:xo + n, xo:xo + n] += 0.5 * (p["Q"][k] + p["Q"][k].T)
        if k == N - 1:
            break
        K[uo:uo + m, uo:uo + m] += 0.5 * (p["R"][k] + p["R"][k].T)
        K[xo:xo + n, uo:uo + m] += p["H"][k]
        K[uo:uo + m, xo:xo + n] += p["H"][k].T
        # (kkt_sparse writes r and d of the rows that exist only; A, B of the last knot are not in K)
    return K, b


def refined_solve(K, g, iters=4):
    """K^-1 g: LU in float64, `iters` refinement steps with the residual in longdouble"""
    lu = sla.lu_factor(K)
    Kl = K.astype(np.longdouble)
    gl = np.asarray(g, dtype=np.longdouble)
    z = sla.lu_solve(lu, np.asarray(g, dtype=np.float64)).astype(np.longdouble)
    for _ in range(iters):
        r = gl - Kl @ z
        z = z + sla.lu_solve(lu, r.astype(np.float64))
    return z.astype(np.float64)


# ---------------------------------------------------------------------------- the reduction, restated

def _chol(a):
    """lower Cholesky factor, in the dtype of a (column by column; reads the lower triangle only)"""
    a = np.tril(a).copy()
    k = a.shape[0]
    for j in range(k):
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] /= a[j, j]
        for c in range(j + 1, k):
            a[c:, c] -= a[c:, j] * a[c, j]
    return a


def _fwd(L, Bm):
    """L^-1 Bm (L lower), in the dtype of the inputs"""
    X = np.array(Bm, dtype=L.dtype, copy=True)
    X = X.reshape(X.shape[0], -1)
    for j in range(L.shape[0]):
        X[j] = X[j] / L[j, j]
        X[j + 1:] -= np.outer(L[j + 1:, j], X[j])
    return X.reshape(np.shape(Bm))


def _bwd(L, Bm):
    """L^-T Bm"""
    X = np.array(Bm, dtype=L.dtype, copy=True)
    X = X.reshape(X.shape[0], -1)
    for j in range(L.shape[0] - 1, -1, -1):
        X[j] = X[j] / L[j, j]
        X[:j] -= np.outer(L[j, :j], X[j])
    return X.reshape(np.shape(Bm))


def reduce(p, dtype=np.float64):
    """The reduction of one problem in `dtype`: dict of L [N, n, n], LR [N, m, m], G [N, m, n] (LR = 1, G = 0 at knot
    N-1), At [N, n, n], Bt [N, n, m] (zero at knot N-1), qt, rt, dt, x0t."""
    n, m, N = dims(p)
    P = {k: np.asarray(p[k], dtype=dtype) for k in NAMES}
    L = np.zeros((N, n, n), dtype); LR = np.zeros((N, m, m), dtype); G = np.zeros((N, m, n), dtype)
    At = np.zeros((N, n, n), dtype); Bt = np.zeros((N, n, m), dtype)
    qt = np.zeros((N, n), dtype); rt = np.zeros((N, m), dtype); dt = np.zeros((N, n), dtype)
    for k in range(N):
        if k == N - 1:
            L[k] = _chol(P["Q"][k]); LR[k] = np.eye(m, dtype=dtype)
            qt[k] = _fwd(L[k], P["q"][k])
            break
        LR[k] = _chol(P["R"][k])
        W = _fwd(LR[k], P["H"][k].T).T        # H L_R^-T
        G[k] = _bwd(LR[k], W.T)               # L_R^-T W' = R^-1 H'
        L[k] = _chol(P["Q"][k] - W @ W.T)
        qt[k] = _fwd(L[k], P["q"][k] - G[k].T @ P["r"][k])
        rt[k] = _fwd(LR[k], P["r"][k])
    for k in range(N - 1):
        At[k] = L[k + 1].T @ _fwd(L[k], (P["A"][k] - P["B"][k] @ G[k]).T).T
        Bt[k] = L[k + 1].T @ _fwd(LR[k], P["B"][k].T).T
        dt[k] = L[k + 1].T @ P["d"][k]
    return dict(L=L, LR=LR, G=G, At=At, Bt=Bt, qt=qt, rt=rt, dt=dt, x0t=L[0].T @ P["x0"])


def reduction_flat(reds):
    """list of reduce() results -> dict of arrays in the layout of BatchSolver.cost_reduction()"""
    out = {}
    for k in ("L", "LR", "G", "At", "Bt", "qt", "rt", "dt", "x0t"):
        a = np.stack([r[k] for r in reds])
        if a.ndim == 4:
            a = a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1)
        out[k] = a
    return out


def split(z, n, m, N):
    """packed [nvars] -> lam [N, n], x [N, n], u [N, m] (u of knot N-1: zero)"""
    full = np.zeros(N * (2 * n + m), dtype=np.asarray(z).dtype)
    full[: z.size] = z
    Z = full.reshape(N, 2 * n + m)
    return Z[:, :n].copy(), Z[:, n:2 * n].copy(), Z[:, 2 * n:].copy()


def join(lam, x, u):
    N, n = lam.shape
    m = u.shape[1]
    return np.concatenate([lam, x, u], axis=1).reshape(-1)[: N * (2 * n + m) - m]


def apply_S(red, zt):
    """z = S z~"""
    N, n, _ = red["L"].shape
    m = red["LR"].shape[1]
    lam, x, u = split(np.asarray(zt, dtype=red["L"].dtype), n, m, N)
    for k in range(N):
        lam[k] = red["L"][k] @ lam[k]
        x[k] = _bwd(red["L"][k], x[k])
        if k < N - 1:
            u[k] = _bwd(red["LR"][k], u[k]) - red["G"][k] @ x[k]
    return join(lam, x, u)


def apply_St(red, g):
    """g~ = S' g"""
    N, n, _ = red["L"].shape
    m = red["LR"].shape[1]
    lam, x, u = split(np.asarray(g, dtype=red["L"].dtype), n, m, N)
    for k in range(N):
        lam[k] = red["L"][k].T @ lam[k]
        if k < N - 1:
            x[k] = _fwd(red["L"][k], x[k] - red["G"][k].T @ u[k])
            u[k] = _fwd(red["LR"][k], u[k])
        else:
            x[k] = _fwd(red["L"][k], x[k])
    return join(lam, x, u)


def reduced_problem(red):
    """the unit-cost problem of a reduction as a dense problem dict (float64)"""
    N, n, _ = red["L"].shape
    m = red["LR"].shape[1]
    f = lambda a: np.asarray(a, dtype=np.float64)
    return dict(A=f(red["At"]), B=f(red["Bt"]), Q=np.stack([np.eye(n)] * N), H=np.zeros((N, n, m)),
                R=np.stack([np.eye(m)] * N), q=f(red["qt"]), r=f(red["rt"]), d=f(red["dt"]), x0=f(red["x0t"]))


def reduced_flat_diag(reds):
    """list of reduce() results -> the eight arrays of BatchSolver.initialize_flat (Q = R = 1)"""
    ps = [reduced_problem(r) for r in reds]
    A, B, q, r, d, x0 = flat(ps, ("A", "B", "q", "r", "d", "x0"))
    return A, B, np.ones_like(q), np.ones_like(r), q, r, d, x0


def field_errors(z, ref, n, m, N):
    """max-abs difference over max-abs of the field, for lam, x, u"""
    out = []
    for a, b in zip(split(z, n, m, N), split(ref, n, m, N)):
        out.append(float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(float).tiny)))
    return out


@functools.lru_cache(maxsize=None)
def family(n, m, N, name):
    """The shared, read-only reference of one (shape, horizon, family): BATCH seeded problems, their refined dense
    solutions z, a seeded adjoint right-hand side g per problem and the refined w = K^-1 g."""
    cond = FAMILIES[name]
    probs = [dense_problem(n, m, N, cond, 100 + 7 * i + (0 if name == "moderate" else 1000)) for i in range(BATCH)]
    rng = np.random.default_rng([n, m, N, int(cond)])
    zs, gs, ws = [], [], []
    for p in probs:
        K, b = dense_kkt(p)
        zs.append(refined_solve(K, b))
        g = rng.standard_normal(b.size)
        gs.append(g)
        ws.append(refined_solve(K, g))
    out = dict(probs=probs, z=np.stack(zs), g=np.stack(gs), w=np.stack(ws))
    for a in (out["z"], out["g"], out["w"]):
        a.setflags(write=False)
    return out


def gradient_reference(p, z, w):
    """dL/dtheta = -(dK/dtheta z - db/dtheta)' w for the nine arguments, read off the block positions of K and b
    (dense_kkt), from z = K^-1 b and w = K^-1 g. Q and R move as symmetric matrices: their gradients are the symmetric
    parts. Zero for A, B, H, R, r, d of the last knot. Math convention, the shapes of the problem dict."""
    n, m, N = dims(p)
    zb = 2 * n + m
    out = {k: np.zeros_like(np.asarray(p[k], dtype=np.float64)) for k in NAMES}
    out["x0"] = -w[0:n]                                   # b[0:n] = -x0
    for k in range(N):
        xo, uo = k * zb + n, k * zb + 2 * n
        zx, wx = z[xo:xo + n], w[xo:xo + n]
        S = np.outer(wx, zx)                              # K[xo+i, xo+j] = Q[i, j]
        out["Q"][k] = -0.5 * (S + S.T)
        out["q"][k] = -wx                                 # b[xo] = -q
        if k == N - 1:
            break
        l1 = (k + 1) * zb
        zu, wu, zl, wl = z[uo:uo + m], w[uo:uo + m], z[l1:l1 + n], w[l1:l1 + n]
        S = np.outer(wu, zu)                              # K[uo+i, uo+j] = R[i, j]
        out["R"][k] = -0.5 * (S + S.T)
        out["H"][k] = -(np.outer(wx, zu) + np.outer(zx, wu))   # K[xo+i, uo+j] = K[uo+j, xo+i] = H[i, j]
        out["A"][k] = -(np.outer(wl, zx) + np.outer(zl, wx))   # K[l1+i, xo+j] = K[xo+j, l1+i] = A[i, j]
        out["B"][k] = -(np.outer(wl, zu) + np.outer(zl, wu))   # K[l1+i, uo+j] = K[uo+j, l1+i] = B[i, j]
        out["r"][k] = -wu                                 # b[uo] = -r
        out["d"][k] = -wl                                 # b[l1] = -d
    return out
