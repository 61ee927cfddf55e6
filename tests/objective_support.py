"""Independent references for the objective values and stage costs (ndlqr_BatchObjective).

Problems are the dense-cost dicts of cost_support.py (math convention); diagonal-cost problems go through
cost_support.diagonal_problem. A solution is a packed vector z [nvars] = [lam_k x_k u_k] per knot.

- exact(): l_k and J with fractions.Fraction on the float64 bits of the inputs and of z, rounded once to float64, and the
  sizes S_k = sum |term|, S = sum_k S_k with every product of the sum counted once in absolute value. (numpy longdouble
  is not good enough: over a few thousand terms its own error reaches an ulp of float64.) Q and R are read through their
  lower triangles, as the library reads them:
      l_k = sum_i x_i (Q_ii x_i / 2 + sum_{j<i} Q_ij x_j + sum_j H_ij u_j + q_i) + sum_i u_i (R_ii u_i / 2 + sum_{j<i} R_ij u_j + r_i)
  and the last knot contributes its Q and q terms alone.
- reduced_f64(): the float64 restatement of dense-cost mode -- cost_support.reduce, the delivered (x, u) mapped to
  xi = L'x, nu = L_R'(u + G x), the unit-cost stage cost |xi|^2 / 2 + |nu|^2 / 2 + q~'xi + r~'nu: the conditioning
  yardstick there.
- families(): the shared, read-only problems of one (shape, horizon, kind).
- envelope(): dJ*/dtheta of the optimal value from a solution, in numpy.
- kkt_value_torch(): J* through torch.linalg.solve of the dense KKT matrix, differentiable by torch autograd.
Test infrastructure.
"""
import functools
from fractions import Fraction

import numpy as np

import cost_support as cs

EPS = np.finfo(float).eps
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5)]
HORIZONS = [2, 5, 8, 16, 33]
BATCH = cs.BATCH


def exact(p, z):
    """dict ell [N], J, S_k [N], S of one problem at the packed solution z (float64 each, rounded once)"""
    n, m, N = cs.dims(p)
    _, x, u = cs.split(np.asarray(z, dtype=np.float64), n, m, N)
    F = Fraction
    ell, Sk = [], []
    Jx, Sx = F(0), F(0)
    for k in range(N):
        xs = [F(float(v)) for v in x[k]]
        us = [F(float(v)) for v in u[k]]
        terms = []
        Q, q = p["Q"][k], p["q"][k]
        for i in range(n):
            if Q[i, i] != 0.0:
                terms.append(F(float(Q[i, i])) * xs[i] * xs[i] / 2)
            for j in range(i):
                if Q[i, j] != 0.0:
                    terms.append(F(float(Q[i, j])) * xs[i] * xs[j])
            terms.append(F(float(q[i])) * xs[i])
        if k < N - 1:
            H, R, r = p["H"][k], p["R"][k], p["r"][k]
            for i in range(n):
                for j in range(m):
                    if H[i, j] != 0.0:
                        terms.append(F(float(H[i, j])) * xs[i] * us[j])
            for i in range(m):
                if R[i, i] != 0.0:
                    terms.append(F(float(R[i, i])) * us[i] * us[i] / 2)
                for j in range(i):
                    if R[i, j] != 0.0:
                        terms.append(F(float(R[i, j])) * us[i] * us[j])
                terms.append(F(float(r[i])) * us[i])
        lk, sk = sum(terms, F(0)), sum((abs(t) for t in terms), F(0))
        ell.append(float(lk)); Sk.append(float(sk))
        Jx += lk; Sx += sk
    return dict(ell=np.array(ell), J=float(Jx), S_k=np.array(Sk), S=float(Sx))


def exact_batch(probs, Z):
    """exact() of every problem, stacked: ell, S_k [batch, N], J, S [batch]"""
    ex = [exact(p, z) for p, z in zip(probs, Z)]
    return {k: np.stack([np.asarray(e[k]) for e in ex]) for k in ("ell", "J", "S_k", "S")}


def reduced_f64(p, z):
    """dict ell [N], J of one problem at z by the unit-cost form, everything in float64"""
    n, m, N = cs.dims(p)
    red = cs.reduce(p, np.float64)
    _, x, u = cs.split(np.asarray(z, dtype=np.float64), n, m, N)
    ell = np.zeros(N)
    for k in range(N):
        xi = red["L"][k].T @ x[k]
        ell[k] = 0.5 * (xi @ xi) + red["qt"][k] @ xi
        if k < N - 1:
            nu = red["LR"][k].T @ (u[k] + red["G"][k] @ x[k])
            ell[k] += 0.5 * (nu @ nu) + red["rt"][k] @ nu
    return dict(ell=ell, J=float(ell.sum()))


def dense_bar(probs, Z, ex):
    """(bars for J [batch], bars for l_k [batch, N], the restatement's own errors likewise): max(8 x the float64
    restatement's own error against exact, 16 eps S) -- the bar of test_gpu_gains and test_gpu_cost"""
    f64 = [reduced_f64(p, z) for p, z in zip(probs, Z)]
    ownJ = np.array([abs(f["J"] - j) for f, j in zip(f64, ex["J"])])
    ownl = np.abs(np.stack([f["ell"] for f in f64]) - ex["ell"])
    return np.maximum(8 * ownJ, 16 * EPS * ex["S"]), np.maximum(8 * ownl, 16 * EPS * ex["S_k"]), ownJ, ownl


def without_H(probs):
    out = []
    for p in probs:
        c = dict(p)
        c["H"] = np.zeros_like(p["H"])
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def families(n, m, N, kind, batch=BATCH):
    """kind "diagonal": generate_synthetic problems as dense dicts; "dense": cost_support's moderate family (cond 1e3);
    "dense-noH": the same with H = 0. Read-only."""
    if kind == "diagonal":
        probs = [cs.diagonal_problem(n, m, N, 500 + 13 * i)[0] for i in range(batch)]
    else:
        probs = list(cs.family(n, m, N, "moderate")["probs"][:batch])
        if batch > cs.BATCH:
            raise ValueError("the dense family holds %d problems" % cs.BATCH)
        if kind == "dense-noH":
            probs = without_H(probs)
    return probs


def diagonals(probs):
    """Qd [batch, N, n], Rd [batch, N, m] of diagonal-cost problems given as dense dicts"""
    return (np.stack([np.stack([np.diag(M) for M in p["Q"]]) for p in probs]),
            np.stack([np.stack([np.diag(M) for M in p["R"]]) for p in probs]))


def diagonal_solver(ndlqr, probs, flags=0):
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    A, B, q, r, d, x0 = cs.flat(probs, ("A", "B", "q", "r", "d", "x0"))
    Qd, Rd = diagonals(probs)
    bs.initialize_flat(A, B, Qd, Rd, q, r, d, x0)
    return bs


def dense_solver(ndlqr, probs, flags=0):
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat_dense(*cs.flat(probs))
    return bs


# ---------------------------------------------------------------------------- the envelope theorem

def envelope(z, n, m, N, dense):
    """dJ*/d(name) of one problem from its solution z, math convention: dict over A, B, Q, (H,) R, q, r, d, x0. With
    L = J - lam_0'(x_0 - x_init) + sum_k lam_(k+1)'(A_k x_k + B_k u_k + d_k - x_(k+1)), the Lagrangian of the library's KKT
    rows. Zero for A, B, H, R, r, d of the last knot; diagonal costs: Q [N, n], R [N, m]."""
    lam, x, u = cs.split(np.asarray(z, dtype=np.float64), n, m, N)
    g = dict(A=np.zeros((N, n, n)), B=np.zeros((N, n, m)), q=x.copy(), r=np.zeros((N, m)), d=np.zeros((N, n)), x0=lam[0].copy())
    g["r"][:N - 1] = u[:N - 1]
    g["d"][:N - 1] = lam[1:]
    for k in range(N - 1):
        g["A"][k] = np.outer(lam[k + 1], x[k])
        g["B"][k] = np.outer(lam[k + 1], u[k])
    if dense:
        g["Q"] = np.stack([0.5 * np.outer(x[k], x[k]) for k in range(N)])
        g["H"] = np.zeros((N, n, m)); g["R"] = np.zeros((N, m, m))
        for k in range(N - 1):
            g["H"][k] = np.outer(x[k], u[k])
            g["R"][k] = 0.5 * np.outer(u[k], u[k])
    else:
        g["Q"] = 0.5 * x * x
        g["R"] = np.zeros((N, m))
        g["R"][:N - 1] = 0.5 * u[:N - 1] ** 2
    return g


def kkt_value_torch(t, n, m, N, dense):
    """(J* [b], z [b, nvars]) of the problems in the dict of CPU torch tensors t (math convention, [b, N, ..]; diagonal
    costs: Q [b, N, n], R [b, N, m]) through torch.linalg.solve of the dense KKT matrix -- rows
        -x_0 = -x_init;   Q x + H u - lam_k + A' lam_(k+1) = -q;   H' x + R u + B' lam_(k+1) = -r;   A x + B u - x_(k+1) = -d
    -- every entry of the last knot's A, B, H, R, r, d left out. Differentiable by torch autograd."""
    import torch
    b = t["A"].shape[0]
    zb = 2 * n + m
    nv = zb * N - m
    K = torch.zeros((b, nv, nv), dtype=torch.float64)
    rhs = torch.zeros((b, nv), dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    Q = t["Q"] if dense else torch.diag_embed(t["Q"])
    R = t["R"] if dense else torch.diag_embed(t["R"])
    for k in range(N):
        lo, xo, uo, l1 = k * zb, k * zb + n, k * zb + 2 * n, (k + 1) * zb
        K[:, lo:lo + n, xo:xo + n] = -eye
        K[:, xo:xo + n, lo:lo + n] = -eye
        K[:, xo:xo + n, xo:xo + n] = Q[:, k]
        rhs[:, xo:xo + n] = -t["q"][:, k]
        rhs[:, lo:lo + n] = -(t["x0"] if k == 0 else t["d"][:, k - 1])
        if k == N - 1:
            break
        K[:, uo:uo + m, uo:uo + m] = R[:, k]
        rhs[:, uo:uo + m] = -t["r"][:, k]
        if dense:
            K[:, xo:xo + n, uo:uo + m] = t["H"][:, k]
            K[:, uo:uo + m, xo:xo + n] = t["H"][:, k].transpose(-1, -2)
        K[:, l1:l1 + n, xo:xo + n] = t["A"][:, k]
        K[:, xo:xo + n, l1:l1 + n] = t["A"][:, k].transpose(-1, -2)
        K[:, l1:l1 + n, uo:uo + m] = t["B"][:, k]
        K[:, uo:uo + m, l1:l1 + n] = t["B"][:, k].transpose(-1, -2)
    z = torch.linalg.solve(K, rhs.unsqueeze(-1)).squeeze(-1)
    return value_torch(t, z, n, m, N, dense), z


def value_torch(t, z, n, m, N, dense):
    """J [b] of the packed solutions z [b, nvars] written in torch (any device): what autograd differentiates"""
    import torch
    zb = 2 * n + m
    full = torch.nn.functional.pad(z, (0, m)).reshape(z.shape[0], N, zb)
    x, u = full[:, :, n:2 * n], full[:, :N - 1, 2 * n:]
    if dense:
        J = 0.5 * torch.einsum("bki,bkij,bkj->b", x, t["Q"], x) + (t["q"] * x).sum((1, 2))
        J = J + 0.5 * torch.einsum("bki,bkij,bkj->b", u, t["R"][:, :N - 1], u) + (t["r"][:, :N - 1] * u).sum((1, 2))
        J = J + torch.einsum("bki,bkij,bkj->b", x[:, :N - 1], t["H"][:, :N - 1], u)
    else:
        J = (0.5 * t["Q"] * x * x + t["q"] * x).sum((1, 2)) + (0.5 * t["R"][:, :N - 1] * u * u + t["r"][:, :N - 1] * u).sum((1, 2))
    return J
