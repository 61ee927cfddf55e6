"""Reference for the per-problem adaptive penalty of the solve with linear inequality constraints (DESIGN.md section
3.19): lin_support.admm with the rule of box_adaptive_support.penalty_step.

- admm_adaptive(): the iteration of lin_support.admm, in float64 or longdouble, in which a running problem may move its
  penalty at the iterations it % every == 0, it < max_iter. A move multiplies y by rho / rho+ (mu = rho y is kept) and
  rebuilds the shifted KKT matrix and its LU. every == 0: lin_support.admm, operation for operation.
- margin(): how far the decisions of a run were from going the other way. The rule looks at ilogb of the two normalised
  residuals r_prim / sp and r_dual / sd, so a decision can change only where one of them crosses a power of two: the
  margin is the smallest relative distance of their frexp mantissas from 1/2 and 1 over all adapt iterations. A case is
  DECIDED when its margin is at least DECIDED (1e-3). That is a condition on the inputs, not a tolerance: the device's
  re-solve is not the restatement's bit for bit (section 3.17 allows +-2 iterations already), and a residual next to a
  power of two may fall either way.
- case(): the shared, read-only runs of one (shape, horizon) of lin_support.case.
Test infrastructure.
"""
import functools
import math

import numpy as np

import cost_support as cs
import lin_support as ls
from box_adaptive_support import RHO_MAX, RHO_MIN, penalty_step

EVERY = 25
DECIDED = 1e-3
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5)]
HORIZONS = (2, 5, 8, 16)
UNDECIDED_CAP = 6  # of the 48 cases


def admm_adaptive(p, C, D, lo, hi, rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=2000, every=EVERY,
                  rho_min=RHO_MIN, rho_max=RHO_MAX, dtype=np.float64, start=None, trace=None, iterates=False):
    """The iteration of DESIGN.md sections 3.17 and 3.19. Returns dict(z, v, y, mu, iters, status, resid, rho, moves).
    rho: the start penalty; the result's rho is the final one. moves: one dict per move -- it, rho, rho_new, clamped (the
    clamp [rho_min, rho_max] cut the step), mu_before, mu_after. start: (v, y) of a warm start. trace: a list that gets
    one dict per iteration -- it, resid, rho (the penalty the iteration ran with), adapt (the rule was evaluated after
    it), and with `iterates` z, v, y."""
    n, m, N = cs.dims(p)
    M = np.isfinite(lo) | np.isfinite(hi)
    alpha_ = dtype(alpha)
    oma = dtype(1.0 - alpha)  # (1 - alpha computed once in double, as the host does)
    lo_, hi_ = lo.astype(dtype), hi.astype(dtype)
    v = np.zeros((N, C.shape[1]), dtype)
    y = np.zeros_like(v)
    if start is not None:
        v = np.where(M, start[0], 0).astype(dtype)
        y = np.where(M, start[1], 0).astype(dtype)
    mx = lambda a: a.dtype.type(np.abs(a).max()) if a.size else dtype(0)

    def factor(r):
        K, b = ls.kkt_ld(ls.shifted_problem(p, C, D, lo, hi, r, dtype))
        return ls.Solver(K), b

    rho = float(rho)
    solve, b = factor(rho)
    rho_ = dtype(rho)
    status, it, z, resid, moves = 0, 0, None, None, []
    for it in range(1, max_iter + 1):
        z = solve(b - ls.perturbation(p, C, D, np.where(M, rho_ * (y - v), 0).astype(dtype)))
        w = ls.rows_of(p, C, D, z)
        wh = alpha_ * w + oma * v
        vn = np.where(M, np.minimum(np.maximum(wh + y, lo_), hi_), 0).astype(dtype)
        yn = np.where(M, (y + wh) - vn, 0).astype(dtype)
        gd = ls.perturbation(p, C, D, vn - v)
        gy = ls.perturbation(p, C, D, yn)
        r_prim = mx((w - vn)[M])
        r_dual = rho_ * mx(gd)
        sp = max(mx(w[M]), mx(vn[M]))
        sd = rho_ * mx(gy)
        resid = (r_prim, r_dual, sp, sd)
        finite = all(np.isfinite(float(a)) for a in resid)
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        frozen = conv or not finite
        adapt = every > 0 and it % every == 0 and it < max_iter and not frozen
        if trace is not None:
            entry = dict(it=it, resid=resid, rho=rho, adapt=adapt)
            if iterates:
                entry.update(z=z.copy(), v=v.copy(), y=y.copy())
            trace.append(entry)
        if frozen:
            status = 1 if conv else 3
            break
        if adapt:
            new = penalty_step(rho, *(float(a) for a in resid), rho_min, rho_max)
            if new != rho:
                mu_before = rho_ * y
                y = np.where(M, y * dtype(rho / new), 0).astype(dtype)
                moves.append(dict(it=it, rho=rho, rho_new=new, clamped=new in (rho_min, rho_max),
                                  mu_before=mu_before, mu_after=dtype(new) * y))
                rho, rho_ = new, dtype(new)
                solve, b = factor(rho)
    return dict(z=z, v=v, y=y, mu=rho_ * y, iters=it, status=status or 2, resid=resid, rho=rho, moves=moves)


def mantissa_margin(x):
    """relative distance of the frexp mantissa f in [1/2, 1) of x > 0 from the two ends"""
    f = math.frexp(float(x))[0]
    return min((f - 0.5) / 0.5, 1.0 - f)


def margin(trace):
    """the smallest mantissa_margin of r_prim / sp and r_dual / sd over the adapt iterations of a trace (inf: the rule was
    never evaluated, or never on four finite positive numbers -- there is nothing a rounding could turn)"""
    out = math.inf
    for t in trace:
        if not t["adapt"]:
            continue
        r_prim, r_dual, sp, sd = (float(a) for a in t["resid"])
        if not all(math.isfinite(a) and a > 0.0 for a in (r_prim, r_dual, sp, sd)):
            continue
        out = min(out, mantissa_margin(r_prim / sp), mantissa_margin(r_dual / sd))
    return out


def adapt_rounds(runs):
    """the adapt iterations at which some problem of a batch moved (runs: admm_adaptive results): one factorisation each"""
    return sorted({mv["it"] for r in runs for mv in r["moves"]})


@functools.lru_cache(maxsize=None)
def case(n, m, N, max_iter=2000, every=EVERY):
    """The shared, read-only adaptive runs of lin_support.case(n, m, N) in float64 at eps = 1e-8: per problem
    dict(run, margin, decided)."""
    out = []
    for c in ls.case(n, m, N):
        trace = []
        run = admm_adaptive(c["p"], c["C"], c["D"], c["lo"], c["hi"], max_iter=max_iter, every=every, trace=trace)
        mg = margin(trace)
        out.append(dict(run=run, margin=mg, decided=mg >= DECIDED))
    return out
