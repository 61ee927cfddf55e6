"""Reference for horizons that are no power of two ("Padded horizon"): the problem padded on the
host to the next power of two, P, with decoupled unit knots, solved by the oracle. The caller's last knot N - 1 becomes an
interior knot with [A | B] = 0, R = 1 and a zero r slot; the knots behind it have [A | B] = 0, Q = R = 1 and a zero
right-hand side. The first nvars entries of the padded solution are the solution of the N-knot problem, the rest is
exactly zero. Test infrastructure."""
import numpy as np

from support import Problem

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def next_pow2(N):
    P = 1
    while P < N:
        P *= 2
    return P


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def pad_problem(prob, P=None):
    """the host-padded problem of horizon P (default: the next power of two); A, B, R, r, d of the caller's last knot are
    not read"""
    n, m, N = prob.n, prob.m, prob.N
    P = next_pow2(N) if P is None else P
    assert P >= N
    if P == N:
        return prob
    A = np.zeros((P, n * n)); B = np.zeros((P, n * m))
    Q = np.ones((P, n)); R = np.ones((P, m))
    q = np.zeros((P, n)); r = np.zeros((P, m)); d = np.zeros((P, n))
    A[: N - 1] = prob.A[: N - 1]; B[: N - 1] = prob.B[: N - 1]
    R[: N - 1] = prob.R[: N - 1]; r[: N - 1] = prob.r[: N - 1]; d[: N - 1] = prob.d[: N - 1]
    Q[:N] = prob.Q; q[:N] = prob.q
    return Problem(n, m, P, A, B, Q, R, q, r, d, prob.x0)


def poisoned(prob):
    """the same problem with NaN where an N-knot problem has no data: A, B, R, r, d of the last knot"""
    c = Problem(prob.n, prob.m, prob.N, *[a.copy() for a in prob.arrays()])
    for a in (c.A, c.B, c.R, c.r, c.d):
        a[prob.N - 1] = np.nan
    return c


def reference(oracle, prob):
    """(solution of the N-knot problem [nvars], the tail of the padded solution, pivot failures): the oracle on
    pad_problem(prob)"""
    z, _, _, fails = oracle.solve(pad_problem(prob), 1)
    return z[: prob.nvars].copy(), z[prob.nvars:].copy(), fails


def pad_vector(v, prob, P=None):
    """a vector over the caller's nvars, zero-extended to the padded problem's"""
    P = next_pow2(prob.N) if P is None else P
    out = np.zeros(v.shape[:-1] + ((2 * prob.n + prob.m) * P - prob.m,))
    out[..., : v.shape[-1]] = v
    return out


def stack(probs, keys=ARGS):
    return [np.stack([getattr(p, k) for p in probs]) for k in keys]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def kkt_inf(prob, z):
    """infinity norm of the extended-precision KKT residual of the N-knot system (support.kkt_residual_ld)"""
    from support import kkt_residual_ld
    r_lam, r_x, r_u = kkt_residual_ld(prob, z)
    return float(max(np.abs(r_lam).max(), np.abs(r_x).max(), np.abs(r_u[: prob.N - 1]).max()))


def kkt_bar(prob, z):
    """64 eps (rows of K per knot) max|z| max(1, max|A|, max|B|, max Q, max R) over the data the N-knot problem uses"""
    N = prob.N
    scale = max(1.0, float(np.abs(prob.A[: N - 1]).max()), float(np.abs(prob.B[: N - 1]).max()), float(prob.Q.max()),
                float(prob.R[: N - 1].max()))
    return 64 * np.finfo(np.float64).eps * (2 * prob.n + prob.m) * float(np.abs(z).max()) * scale
