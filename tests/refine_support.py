"""Test infrastructure of the iterative refinement (ndlqr_RefineBatch): a numpy restatement of the device's double-double
residual -- the same rows, the same term order, the same error-free transformations, so it matches the device bit for bit
-- and the refinement loop with its acceptance rule, driving the CPU oracle on the correction problem the way
support.refined_solution does.

Term order of a row of r = b - K z (b: the negated right-hand side of src/solver.c:188-190): the right-hand-side entry,
then the identity and diagonal terms, then j ascending (lambda rows: the columns of A, then those of B):
    lambda_0:      -x0          + x_0
    lambda_(k+1):  -d_k         + x_(k+1)            - sum_j A_k[i, j] x_k[j] - sum_j B_k[i, j] u_k[j]
    x_k:           -q_k         + lambda_k - Q_k x_k  - sum_j A_k[j, i] lambda_(k+1)[j]        (no sum at the last knot)
    u_k:           -r_k                    - R_k u_k  - sum_j B_k[j, i] lambda_(k+1)[j]        (k < N - 1)
Every product is split into its rounded value p and its exact error e (the device: e = fma(a, z, -p); here: Dekker's
splitting, which gives the same e, both being exact), p is added to hi by TwoSum, and lo = lo + (e + e_sum). The row's
value is hi + lo, rounded once. The scale of a row, |b_i| + sum_j |K_ij| |z_j|, is accumulated in plain fp64 in the same
order from the rounded products."""
import numpy as np

from support import Problem

EPS = np.finfo(np.float64).eps
_SPLIT = 134217729.0  # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class _Rows:
    """Double-double accumulators of a set of rows, started at the right-hand-side entries b."""

    def __init__(self, b):
        self.hi = np.array(b, dtype=np.float64)
        self.lo = np.zeros_like(self.hi)
        self.scale = np.abs(self.hi)

    def _add(self, p, e):
        s, es = _two_sum(self.hi, p)
        self.hi = s
        self.lo = self.lo + (e + es)

    def term(self, v):
        self._add(v, 0.0)
        self.scale = self.scale + np.abs(v)

    def fma(self, a, z):
        p, e = _two_prod(a, z)
        self._add(p, e)
        self.scale = self.scale + np.abs(p)

    def value(self):
        return self.hi + self.lo


def blocks(prob, v):
    out = np.zeros(prob.N * (2 * prob.n + prob.m))
    out[: v.size] = v
    return out.reshape(prob.N, 2 * prob.n + prob.m)


def residual_dd(prob, z, delta=None):
    """(r [nvars], rho, scale): r = b - K (z (+) delta) as kkt_residual_dd evaluates it, rho = ||r||_inf and
    scale = max_i (|b_i| + sum_j |K_ij| |z_j|). z, delta: packed [nvars] in the reference's [lambda x u] order."""
    n, m, N = prob.n, prob.m, prob.N
    z = np.asarray(z, dtype=np.float64)
    Z = blocks(prob, z if delta is None else z + np.asarray(delta, dtype=np.float64))
    lam, x, u = Z[:, :n], Z[:, n:2 * n], Z[:, 2 * n:]
    A = prob.A.reshape(N, n, n).transpose(0, 2, 1)  # column-major storage -> A[k][i, j]
    B = prob.B.reshape(N, m, n).transpose(0, 2, 1)
    # lambda rows
    rl = _Rows(np.concatenate([-prob.x0[None, :], -prob.d[: N - 1]]))
    rl.term(x)
    head = _Rows(rl.hi[1:])
    head.lo, head.scale = rl.lo[1:], rl.scale[1:]
    for j in range(n):
        head.fma(-A[: N - 1, :, j], x[: N - 1, j][:, None])
    for j in range(m):
        head.fma(-B[: N - 1, :, j], u[: N - 1, j][:, None])
    r_lam = np.concatenate([rl.value()[:1], head.value()])
    s_lam = np.concatenate([rl.scale[:1], head.scale])
    # x rows
    rx = _Rows(-prob.q)
    rx.term(lam)
    rx.fma(-prob.Q, x)
    head = _Rows(rx.hi[: N - 1])
    head.lo, head.scale = rx.lo[: N - 1], rx.scale[: N - 1]
    for j in range(n):
        head.fma(-A[: N - 1, j, :], lam[1:, j][:, None])
    r_x = np.concatenate([head.value(), rx.value()[N - 1:]])
    s_x = np.concatenate([head.scale, rx.scale[N - 1:]])
    # u rows (none at the last knot)
    ru = _Rows(-prob.r[: N - 1])
    ru.fma(-prob.R[: N - 1], u[: N - 1])
    for j in range(n):
        ru.fma(-B[: N - 1, j, :], lam[1:, j][:, None])
    r_u = np.concatenate([ru.value(), np.zeros((1, m))])
    s_u = np.concatenate([ru.scale, np.zeros((1, m))])
    r = np.concatenate([r_lam, r_x, r_u], axis=1).reshape(-1)[: prob.nvars]
    s = np.concatenate([s_lam, s_x, s_u], axis=1).reshape(-1)[: prob.nvars]
    with np.errstate(invalid="ignore"):
        return r, np.max(np.abs(r)), np.max(s)


def split_rows(prob, v):
    """(lambda [N, n], x [N, n], u [N, m]) of a packed vector."""
    V = blocks(prob, v)
    return V[:, : prob.n], V[:, prob.n: 2 * prob.n], V[:, 2 * prob.n:]


def correction_problem(prob, r):
    """K delta = r as a problem of the same A, B, Q, R: the right-hand side (x0, q, r, d) = -(the rows of r)."""
    r_lam, r_x, r_u = split_rows(prob, r)
    d = np.zeros((prob.N, prob.n))
    d[: prob.N - 1] = -r_lam[1:]
    ru = -r_u
    ru[prob.N - 1] = 0.0
    return Problem(prob.n, prob.m, prob.N, prob.A, prob.B, prob.Q, prob.R, -r_x, ru, d, -r_lam[0])


def eta(rho, scale):
    return 0.0 if rho == 0.0 else rho / scale


def refine_loop(oracle, prob, z, max_steps):
    """The refinement of ndlqr_RefineBatch on one problem with the oracle as the re-solve: (z refined, steps,
    eta_before, eta_after). Step s is accepted iff the residual norm fell strictly at every step up to s."""
    z = np.array(z, dtype=np.float64)
    r, rho, scale = residual_dd(prob, z)
    before = eta(rho, scale)
    steps = 0
    for _ in range(max_steps):
        delta = oracle.solve(correction_problem(prob, r), 1)[0][: prob.nvars]
        r2, rho2, scale2 = residual_dd(prob, z, delta)
        if not rho2 < rho:
            break  # (a rejection is permanent: the device's later steps change nothing)
        z, r, rho, scale = z + delta, r2, rho2, scale2
        steps += 1
    return z, steps, before, eta(rho, scale)


def field_errors(prob, z, truth):
    """Normwise error per field (lambda, x, u): ||z_f - truth_f||_inf, and ||truth_f||_inf."""
    err, size = [], []
    for a, b in zip(split_rows(prob, z), split_rows(prob, truth)):
        err.append(float(np.max(np.abs(a - b))))
        size.append(float(np.max(np.abs(b))))
    return np.array(err), np.array(size)


def hard_problem(synthetic, n, m, N, seed, a_scale=1.05, q_scale=1e-2, r_scale=1e-4):
    """A synthetic problem (synthetic: rslqr_amd.generate_synthetic) with A, Q, R scaled: weak input cost, slightly
    unstable dynamics -- the families on which the solve paths lose digits."""
    g = synthetic(n, m, N, seed)
    return Problem(n, m, N, g["A"] * a_scale, g["B"], g["Q"] * q_scale, g["R"] * r_scale, g["q"], g["r"], g["d"], g["x0"])
