"""Test infrastructure of the per-iteration tests of the box ADMM update kernels (box_update, box_adjoint_update and the
element-wise kernels around them; tests/test_gpu_box_update.py, tests/test_box_update_host.py):

- mixed_bounds(): the bound pattern of those tests -- every class of entry in every knot (two-sided, upper only, lower
  only, unbounded) and one entry with lo == hi.
- forward_trace() / adjoint_trace(): the state after EVERY iteration -- z, v, y, the four numbers of the read-out
  (ndlqr_CopyBatchBoxResiduals) and whether the problem converged there. They wrap box_support.admm_reference and
  box_grad_support.adjoint_admm_reference through their `trace` argument: one arithmetic, not two. Everything is on
  [N, n+m] arrays in the caller's layout; nothing here indexes the device layout except update_launch() and
  padded_offset(), which restate the launcher so that the cases can be held to the loop passes they were chosen for.
- planted(): the "every entry counted once" problem family (all entries loose inside +-B, one entry pinned far away).
"""
import numpy as np

from box_grad_support import adjoint_admm_reference, full_bounds
from box_support import admm_reference, blocks, shifted_problem
from residual_support import padded_dims

RHO, ALPHA = 0.37, 1.6  # the settings of every strict bit-for-bit test of the box solve


def oracle_solve(oracle):
    return lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]


def unconstrained_xu(oracle, prob):
    """x [N, n], u [N, m] of the unconstrained oracle solution (u of the last knot taken as 0)"""
    n, m, N = prob.n, prob.m, prob.N
    Z = blocks(oracle.solve(prob, 1)[0][: prob.nvars], n, m, N)
    return Z[:, n:2 * n].copy(), Z[:, 2 * n:].copy()


def entry_class(n, m, N):
    """c = (k + j) % 4 over knot k and entry j of [x | u], [N, n+m]"""
    return (np.arange(N)[:, None] + np.arange(n + m)[None, :]) % 4


def addressable(n, m, N):
    """[N, n+m] bool: the entries a bound can apply to (not x of knot 0, not u of the last knot)"""
    A = np.ones((N, n + m), dtype=bool)
    A[0, :n] = False
    A[N - 1, n:] = False
    return A


def pinned_entry(n, m, N):
    """(k, j) of the entry that gets lo == hi: the first addressable two-sided input in knot order (an input can take
    any value, so the pin leaves the problem as feasible as it was)"""
    c = entry_class(n, m, N)
    ok = (c == 0) & addressable(n, m, N)
    ok[:, :n] = False
    k, j = np.argwhere(ok)[0]
    return int(k), int(j)


def mixed_bounds(oracle, prob, pin=True, scale=1.0, release=False):
    """(xlo, xhi, ulo, uhi) [N, n] / [N, m] of one problem: cap = 0.7 max_{k>=1} |x_k| per state and 0.5 mean_k |u_k| per
    input of the unconstrained solution, hi = cap, lo = -cap at every knot; then by c = (k + j) % 4: 1 upper bound only,
    2 lower bound only, 3 unbounded, 0 both. pin: the entry pinned_entry() gets lo == hi == cap / 2. scale: every finite
    bound times that (the pattern stays). release: the last two-sided entry of every knot, other than the pinned one,
    becomes unbounded where the knot has one (the pattern changes; the last ones are mostly inputs, which sit on their
    bounds more often than the states do)."""
    n, m, N = prob.n, prob.m, prob.N
    x, u = unconstrained_xu(oracle, prob)
    cap = np.concatenate([0.7 * np.abs(x[1:]).max(axis=0), 0.5 * np.abs(u).mean(axis=0)])
    hi = np.tile(cap, (N, 1))
    lo = -hi
    c = entry_class(n, m, N)
    lo[(c == 1) | (c == 3)] = -np.inf
    hi[(c == 2) | (c == 3)] = np.inf
    if pin:
        k, j = pinned_entry(n, m, N)
        lo[k, j] = hi[k, j] = 0.5 * cap[j]
    if release:
        pk = pinned_entry(n, m, N) if pin else None
        for k in range(N):
            for j in np.nonzero((c[k] == 0) & addressable(n, m, N)[k])[0][::-1]:
                if (k, int(j)) != pk:
                    lo[k, j], hi[k, j] = -np.inf, np.inf
                    break
    lo, hi = lo * scale, hi * scale
    return lo[:, :n].copy(), hi[:, :n].copy(), lo[:, n:].copy(), hi[:, n:].copy()


def stack_bounds(per_problem):
    """[(xlo, xhi, ulo, uhi)] per problem -> four arrays [batch, N, .]"""
    return tuple(np.stack([b[i] for b in per_problem]) for i in range(4))


def classes(prob, bounds, v):
    """how many bounded entries with lo < hi have v on lo / on hi / strictly inside, how many addressable entries are
    unbounded, and how many entries with lo == hi sit there: (on_lo, on_hi, inside, unbounded, pinned)"""
    n, m, N = prob.n, prob.m, prob.N
    lo, hi, M = full_bounds(n, m, N, *bounds)
    open_ = M & (lo < hi)
    return (int((open_ & (v == lo)).sum()), int((open_ & (v == hi)).sum()), int((open_ & (v > lo) & (v < hi)).sum()),
            int((~M & addressable(n, m, N)).sum()), int((M & (lo == hi) & (v == lo)).sum()))


# ------------------------------------------------------------------------------------------------ the restatement, per iteration

class Trace:
    """its: one dict per iteration (it, Z [N, 2n+m], v, y [N, n+m], resid (r_prim, r_dual, sp, sd), conv);
    x, u, mu_x, mu_u, lam, iters, status: what the solve delivers after the last of them."""

    def __init__(self, its, result):
        self.its = its
        self.x, self.u, self.mu_x, self.mu_u, self.lam, self.iters, self.status = result

    @property
    def resid(self):
        return np.array(self.its[-1]["resid"])

    def state(self):
        """(v, y) as the device keeps them for the next warm start: v = z on the unbounded entries (box_finish)"""
        return np.concatenate([self.x, self.u], axis=1), self.its[-1]["y"]

    def argmax_r_prim(self, M, it):
        s = self.its[it - 1]
        n = self.x.shape[1]
        return int(np.argmax(np.where(M, np.abs(s["Z"][:, n:] - s["v"]), -1.0)))


def forward_trace(prob, solve, bounds, max_iter, eps=1e-300, rho=RHO, alpha=ALPHA, start=None):
    its = []
    res = admm_reference(prob, solve, *bounds, rho, alpha, eps, eps, max_iter, start=start, trace=its)
    return Trace(its, res)


class AdjointTrace:
    def __init__(self, its, result):
        self.its = its
        self.w, self.nu, self.iters, self.status = result

    @property
    def resid(self):
        return np.array(self.its[-1]["resid"])


def adjoint_trace(prob, solve, codes, g, max_iter, eps=1e-300, rho=RHO, alpha=ALPHA):
    its = []
    res = adjoint_admm_reference(prob, solve, codes, g, rho, alpha, eps, eps, max_iter, trace=its)
    return AdjointTrace(its, res)


# ------------------------------------------------------------------------------------------------ the launcher, restated

def update_launch(n, m, N):
    """(padded (n, m), N * w, passes of the 256-thread entry loop of box_update / box_adjoint_update, passes of the
    64-thread per-knot loop over the 2n+m rows of box_start / box_finish) at this shape"""
    pn, pm = padded_dims(n, m, N)
    w = pn + pm
    return (pn, pm), N * w, -(-(N * w) // 256), -(-(2 * pn + pm) // 64)


def padded_offset(n, m, N, k, j):
    """offset of entry j of [x | u] of knot k in the device's [N][w] arrays of one problem"""
    pn, pm = padded_dims(n, m, N)
    return k * (pn + pm) + (j if j < n else pn + (j - n))


def nearest_live(n, m, N, offset):
    """(k, j) of the addressable entry whose padded offset is nearest to `offset` (the lower one on a tie)"""
    A = addressable(n, m, N)
    best = None
    for k, j in np.argwhere(A):
        dist = abs(padded_offset(n, m, N, int(k), int(j)) - offset)
        if best is None or dist < best[0]:
            best = (dist, int(k), int(j))
    return best[1], best[2]


def planted_positions(n, m, N):
    """the (k, j) a pinned entry is planted at: first and last column of x at knots 1, N/2, N-1 and of u at knots 0, N/2,
    N-2, and the live entries nearest to padded offsets 255 and 256 and to the start of the last pass of the entry loop"""
    pos = []
    for k in (1, N // 2, N - 1):
        pos += [(k, 0), (k, n - 1)]
    for k in (0, N // 2, N - 2):
        pos += [(k, n), (k, n + m - 1)]
    passes = update_launch(n, m, N)[2]
    for off in (255, 256, 256 * (passes - 1)):
        pos.append(nearest_live(n, m, N, off))
    return sorted(set(pos))


# ------------------------------------------------------------------------------------------------ every entry counted once

PLANT_RHO = 0.25


def planted(oracle, prob):
    """(z [N, n+m], D, B) of the planted family of one problem: z = [x | u] of the oracle's solution with Q + rho,
    R + rho on every addressable entry (the first re-solve of a cold start, whatever the bounds' values), D the power of
    two with D >= 16 max |z|, B = 4 D"""
    n, m, N = prob.n, prob.m, prob.N
    A = addressable(n, m, N).astype(float)
    z = oracle.solve(shifted_problem(prob, PLANT_RHO, A[:, :n], A[:, n:], prob.q, prob.r), 1)[0][: prob.nvars]
    zx = blocks(z, n, m, N)[:, n:].copy()
    D = 2.0 ** int(np.ceil(np.log2(16.0 * np.abs(zx).max())))
    return zx, D, 4.0 * D


def loose_bounds(prob, B):
    n, m, N = prob.n, prob.m, prob.N
    return (np.full((N, n), -B), np.full((N, n), B), np.full((N, m), -B), np.full((N, m), B))


def plant(bounds, n, k, j, c):
    """the bounds with lo == hi == c at entry j of [x | u] of knot k (copies)"""
    out = [a.copy() for a in bounds]
    if j < n:
        out[0][k, j] = out[1][k, j] = c
    else:
        out[2][k, j - n] = out[3][k, j - n] = c
    return tuple(out)
