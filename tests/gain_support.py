"""Independent references for the feedback gains and cost-to-go matrices (ndlqr_BatchFeedbackGains).

Problems are the dense-cost dicts of cost_support.py (math convention); diagonal-cost problems go through
cost_support.diagonal_problem.

- gains(): the backward recursion restated in numpy, in float64 or longdouble (one code path: the dtype argument decides),
  with its own column-by-column Cholesky and substitutions in that dtype, dense Q, H, R:
      P_{N-1} = Q_{N-1}, p_{N-1} = q_{N-1};  for k = N-2 .. 0:
      g = P+ d + p+,  M = [A|B]' P+ [A|B] + [[Q, H], [H', R]],  v = [q; r] + [A|B]' g,
      Quu = L L', W = L^-1 Qux, w = L^-1 Qu,  K = -L^-T W, k = -L^-T w, P = Qxx - W'W, p = Qx - W'w.
- gains_reduced(): the second float64 restatement of dense-cost mode -- cost_support.reduce, the recursion on the unit-cost
  problem, the map back K = L_R^-T K~ L' - G, k = L_R^-T k~, P = L P~ L', p = L p~: the yardstick there.
- reference(): the shared, read-only references of one (shape, horizon, kind): BATCH problems, their gains in longdouble
  and in float64.
- bar(): the per-array bound of the device tests.
Test infrastructure.
"""
import functools

import numpy as np

import cost_support as cs

SHAPES = cs.SHAPES
HORIZONS = [2, 5, 8, 16, 33]
BATCH = cs.BATCH
NAMES = ("K", "k", "P", "p")
EPS = np.finfo(float).eps


def _chol(a):
    """lower Cholesky factor in the dtype of a, a column per step; reads the lower triangle only"""
    a = np.tril(a).copy()
    for j in range(a.shape[0]):
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] = a[j + 1:, j] / a[j, j]
        for c in range(j + 1, a.shape[0]):
            a[c:, c] = a[c:, c] - a[c:, j] * a[c, j]
    return a


def _fwd(L, X):
    """L^-1 X (L lower, X [k, cols]) in the dtype of the inputs"""
    X = X.copy()
    for j in range(L.shape[0]):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    return X


def _bwd(L, X):
    """L^-T X"""
    X = X.copy()
    for j in range(L.shape[0] - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def _mirror(M):
    """the lower triangle, mirrored"""
    return np.tril(M) + np.tril(M, -1).T


def gains(p, dtype=np.float64):
    """dict K [N, m, n], k [N, m], P [N, n, n], p [N, n] of one problem in `dtype` (K, k of knot N-1: zero)"""
    n, m, N = cs.dims(p)
    A, B, Q, H, R, q, r, d = [np.asarray(p[k], dtype=dtype) for k in ("A", "B", "Q", "H", "R", "q", "r", "d")]
    K = np.zeros((N, m, n), dtype); kf = np.zeros((N, m), dtype); P = np.zeros((N, n, n), dtype); pv = np.zeros((N, n), dtype)
    P[N - 1] = _mirror(Q[N - 1])
    pv[N - 1] = q[N - 1]
    for t in range(N - 2, -1, -1):
        AB = np.concatenate([A[t], B[t]], axis=1)
        g = P[t + 1] @ d[t] + pv[t + 1]
        M = AB.T @ (P[t + 1] @ AB) + np.block([[_mirror(Q[t]), H[t]], [H[t].T, _mirror(R[t])]])
        v = np.concatenate([q[t], r[t]]) + AB.T @ g
        L = _chol(M[n:, n:])
        Ww = _fwd(L, np.concatenate([M[n:, :n], v[n:, None]], axis=1))
        Kk = -_bwd(L, Ww)
        K[t], kf[t] = Kk[:, :n], Kk[:, n]
        P[t] = _mirror(M[:n, :n] - Ww[:, :n].T @ Ww[:, :n])
        pv[t] = v[:n] - Ww[:, :n].T @ Ww[:, n]
    return dict(K=K, k=kf, P=P, p=pv)


def gains_reduced(p):
    """float64: reduce -> recursion on the unit-cost problem -> map back"""
    red = cs.reduce(p, np.float64)
    t = gains(cs.reduced_problem(red), np.float64)
    n, m, N = cs.dims(p)
    out = {k: np.zeros_like(v) for k, v in t.items()}
    for k in range(N):
        L, LR, G = red["L"][k], red["LR"][k], red["G"][k]
        Kk = _bwd(LR, np.concatenate([t["K"][k] @ L.T, t["k"][k][:, None]], axis=1))
        out["K"][k], out["k"][k] = Kk[:, :n] - G, Kk[:, n]
        out["P"][k] = _mirror(L @ (t["P"][k] @ L.T))
        out["p"][k] = L @ t["p"][k]
    return out


def stack(gs):
    return {k: np.stack([g[k] for g in gs]) for k in NAMES}


@functools.lru_cache(maxsize=None)
def reference(n, m, N, kind):
    """kind "diagonal": generate_synthetic problems (and their diagonals Qd, Rd); "dense": cost_support's moderate family.
    exact: the longdouble gains [BATCH, N, ..]; f64: the float64 restatement (dense: the reduce / map-back one)."""
    if kind == "diagonal":
        probs, Qd, Rd = zip(*[cs.diagonal_problem(n, m, N, 300 + 11 * i) for i in range(BATCH)])
        f64 = stack([gains(p, np.float64) for p in probs])
    else:
        probs, Qd, Rd = cs.family(n, m, N, "moderate")["probs"], None, None
        f64 = stack([gains_reduced(p) for p in probs])
    exact = stack([gains(p, np.longdouble) for p in probs])
    for a in list(exact.values()) + list(f64.values()):
        a.setflags(write=False)
    return dict(probs=list(probs), Qd=Qd, Rd=Rd, exact=exact, f64=f64)


def bar(exact, f64, name):
    """max(8 x the float64 restatement's own largest error against the longdouble one, 16 eps x the array's largest entry):
    the margin covers another operation order and FMA contraction (the bar of test_gpu_cost.test_reduction_per_entry)"""
    own = float(np.abs(f64[name] - exact[name]).max())
    return max(8 * own, 16 * EPS * float(np.abs(exact[name]).max())), own


def solver(ndlqr, ref, kind, flags=0, probs=None):
    """a BatchSolver holding the problems of `ref` (or `probs`, same kind)"""
    probs = ref["probs"] if probs is None else probs
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    if kind == "diagonal":
        A, B, q, r, d, x0 = cs.flat(probs, ("A", "B", "q", "r", "d", "x0"))
        Qd = np.stack([np.stack([np.diag(Qk) for Qk in p["Q"]]) for p in probs])
        Rd = np.stack([np.stack([np.diag(Rk) for Rk in p["R"]]) for p in probs])
        bs.initialize_flat(A, B, Qd, Rd, q, r, d, x0)
    else:
        bs.initialize_flat_dense(*cs.flat(probs))
    return bs


def closed_loop_errors(g, z, n, m, N):
    """(max_k |u_k - (K_k x_k + k_k)| / max|u|, max_k |lam_k - (P_k x_k + p_k)| / max|lam|) of the gains g (one problem,
    math convention) on the packed solution z; the identities are applied knot by knot, nothing is amplified"""
    lam, x, u = cs.split(np.asarray(z, dtype=g["K"].dtype), n, m, N)
    eu = max(float(np.abs(u[k] - (g["K"][k] @ x[k] + g["k"][k])).max()) for k in range(N - 1))
    el = max(float(np.abs(lam[k] - (g["P"][k] @ x[k] + g["p"][k])).max()) for k in range(N))
    tiny = np.finfo(float).tiny
    return eu / max(float(np.abs(u).max()), tiny), el / max(float(np.abs(lam).max()), tiny)
