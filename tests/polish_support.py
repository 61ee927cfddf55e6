"""Test infrastructure of the active-set polish (ndlqr_PolishBatchBoxConstrained): a numpy
restatement of the whole polish of one problem in the operation order of strict mode -- refine_support.residual_dd for the
residual, a caller-given solver (the oracle on the shifted correction problem) for every re-solve -- and the helpers the
host and device tests share.

One problem at a time; every array is in the caller's block sizes, entries [N, n+m] for (x | u). Entry codes: 0
unbounded, 1 free, 2 active at the lower bound, 3 active at the upper one (an equality reports on the upper bound)."""
import numpy as np

from box_grad_support import full_bounds
from box_support import blocks
from refine_support import correction_problem, residual_dd
from support import Problem

DEFAULT_SIGMA = 1e8  # NDLQR_POLISH_DEFAULT_SIGMA
DEFAULT_MAX_STEPS = 8
DEFAULT_MAX_ROUNDS = 3


def initial_codes(lo, hi, M, v, y):
    """step 1 of the polish: exact comparisons of the ADMM iterate with its bounds"""
    at_hi = ((v == hi) & (y > 0.0)) | (lo == hi)
    at_lo = (v == lo) & (y < 0.0)
    return np.where(~M, 0, np.where(at_hi, 3, np.where(at_lo, 2, 1))).astype(np.int8)


def sigma_of(prob, sigma):
    """sigma times the largest diagonal entry of Q and R (R of the last knot is not part of the problem)"""
    big = 0.0
    for a in (prob.Q, prob.R[: prob.N - 1]):
        for val in a.reshape(-1):
            big = val if (val > big or val != val) else big
    return sigma * big


def entries_of(prob, z):
    """(x | u) [N, n+m] of a packed vector (u of the last knot: 0)"""
    return blocks(z, prob.n, prob.m, prob.N)[:, prob.n:]


def with_entries(prob, z, xu):
    Z = blocks(z, prob.n, prob.m, prob.N).copy()
    Z[:, prob.n:] = xu
    return Z.reshape(-1)[: prob.nvars]


def systems_of(prob, codes, sig, mu):
    """(residual problem, re-solve problem, c is not needed by either): the residual is that of the active-set system,
    r = (b - E_A' mu) - K z on the unshifted Q, R -- equal to b~(mu) - K~ z because z_A = c exactly, without the roundings
    of sig c and Q + sig --; the re-solve is against Q, R + sig on the active entries."""
    n, m, N = prob.n, prob.m, prob.N
    act = codes >= 2
    b = -np.concatenate([prob.q, prob.r], axis=1)
    with np.errstate(invalid="ignore"):
        bt = np.where(act, b - mu, b)
    QR = np.concatenate([prob.Q, prob.R], axis=1)
    QRs = np.where(act, QR + sig, QR)
    cols = lambda a: (np.ascontiguousarray(a[:, :n]), np.ascontiguousarray(a[:, n:]))
    resid = Problem(n, m, N, prob.A, prob.B, prob.Q, prob.R, *cols(-bt), prob.d, prob.x0)
    shifted = Problem(n, m, N, prob.A, prob.B, *cols(QRs), prob.q, prob.r, prob.d, prob.x0)
    return resid, shifted


def polish_reference(prob, solve, bounds, z0, v, y, rho, sigma=0.0, max_steps=0, max_rounds=0, forward_status=1):
    """The polish of DESIGN.md section 3.13 on one problem. solve(problem) -> z (nvars): the re-solve. bounds: (xlo, xhi,
    ulo, uhi), each [N, n] / [N, m] or None; z0: the resident (ADMM) solution, packed; v, y [N, n+m]: the ADMM iterate;
    rho: the problem's penalty. Returns a dict: z (packed), mu [N, n+m], codes [N, n+m], sig (sigma_p), steps, status, rounds (the
    factorisations), v, y (what a warm start finds), norms (per round: the residual norms of its slots)."""
    n, m, N = prob.n, prob.m, prob.N
    sigma = sigma if sigma > 0.0 else DEFAULT_SIGMA
    max_steps = max_steps or DEFAULT_MAX_STEPS
    max_rounds = max_rounds or DEFAULT_MAX_ROUNDS
    lo, hi, M = full_bounds(n, m, N, *bounds)
    z0 = np.array(z0, dtype=np.float64)
    out = {"z": z0, "mu": rho * y, "v": v, "y": y, "steps": 0, "rounds": 0, "norms": [], "sig": sigma_of(prob, sigma)}
    codes = initial_codes(lo, hi, M, v, y)
    out["codes"] = codes
    if forward_status == 3:
        out["status"] = 3
        return out
    sig = sigma_of(prob, sigma)
    z = z0.copy()
    mu = np.where(codes >= 2, rho * y, 0.0)
    steps = 0
    status = 2
    for rnd in range(max_rounds + 1):
        out["rounds"] = rnd + 1
        p2, pshift = systems_of(prob, codes, sig, mu)
        act = codes >= 2
        c = np.where(codes == 3, hi, np.where(codes == 2, lo, 0.0))
        r, norm, _ = residual_dd(p2, z)
        norms = [norm]
        here = 0
        for _ in range(max_steps):
            delta = solve(correction_problem(pshift, r))[: prob.nvars]
            zc = z + delta
            xu = entries_of(prob, zc)
            with np.errstate(invalid="ignore", over="ignore"):
                t = sig * entries_of(prob, delta)
                muc = np.where(act, mu + t, 0.0)
            zc = with_entries(prob, zc, np.where(act, c, xu))
            if not (np.isfinite(zc).all() and np.isfinite(muc).all()):
                out["status"] = 3
                out["codes"] = codes
                return out
            pc, _ = systems_of(prob, codes, sig, muc)
            rc, normc, _ = residual_dd(pc, zc)
            norms.append(normc)
            if not normc < norm:
                break
            z, mu, r, norm, p2 = zc, muc, rc, normc, pc
            here += 1
        out["norms"].append(norms)
        steps += here
        # validation of the last accepted iterate, exact comparisons
        xu = entries_of(prob, z)
        wrong3 = (codes == 3) & (lo < hi) & (mu < 0.0)
        wrong2 = (codes == 2) & (mu > 0.0)
        above = (codes == 1) & (xu > hi)
        below = (codes == 1) & (xu < lo)
        valid = not (wrong3.any() or wrong2.any() or above.any() or below.any())
        if valid or rnd == max_rounds:
            status = 1 if valid and here >= 1 else 2
            break
        codes = np.where(wrong3 | wrong2, 1, np.where(above, 3, np.where(below, 2, codes))).astype(np.int8)
        mu = np.where(wrong3 | wrong2 | above | below, 0.0, mu)
        z = with_entries(prob, z, np.where(above, hi, np.where(below, lo, xu)))
    out["codes"] = codes
    out["steps"] = steps
    out["status"] = status
    if status == 1:
        xu = entries_of(prob, z)
        out.update(z=z, mu=mu, v=xu, y=np.where(M, mu / rho, y))
    return out



def polished_adjoint_reference(prob, solve, codes, sig, g, max_steps=0, polish_status=1):
    """The adjoint of DESIGN.md section 3.13 on one problem: K w + E_A' nu = g, E_A w = 0 by the loop of the polish on
    the final codes and sigma_p = sig -- right-hand side g, c = 0, start w = nu = 0, no rounds. Returns (w packed,
    nu [N, n+m], steps, status); a problem whose polish status is not 1 reports it and keeps the zeros."""
    from box_grad_support import adjoint_problem
    n, m, N = prob.n, prob.m, prob.N
    max_steps = max_steps or DEFAULT_MAX_STEPS
    w, nu = np.zeros(prob.nvars), np.zeros((N, n + m))
    if polish_status != 1:
        return w, nu, 0, polish_status
    ap = adjoint_problem(prob, np.asarray(g, dtype=np.float64))
    act = codes >= 2
    p2, pshift = systems_of(ap, codes, sig, nu)
    r, norm, _ = residual_dd(p2, w)
    norm0, steps = norm, 0
    for _ in range(max_steps):
        delta = solve(correction_problem(pshift, r))[: prob.nvars]
        wc = w + delta
        with np.errstate(invalid="ignore", over="ignore"):
            t = sig * entries_of(prob, delta)
            nuc = np.where(act, nu + t, 0.0)
        wc = with_entries(prob, wc, np.where(act, 0.0, entries_of(prob, wc)))
        if not (np.isfinite(wc).all() and np.isfinite(nuc).all()):
            return w, nu, steps, 3
        pc, _ = systems_of(ap, codes, sig, nuc)
        rc, normc, _ = residual_dd(pc, wc)
        if not normc < norm:
            break
        w, nu, r, norm = wc, nuc, rc, normc
        steps += 1
    return w, nu, steps, 1 if steps >= 1 or norm0 == 0.0 else 2


# ---------------------------------------------------------------------------------------------- shared test problems

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
SWEEP_FAMILIES = [(3, 2, 8), (4, 2, 16), (7, 9, 16)]
SWEEP_SEEDS = (1, 2)
SWEEP_SIGMAS = [1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8]
ROUNDS_CASE = dict(shape=(4, 2, 16), seeds=(700, 702, 704), admm_iters=5, max_rounds=5)      # rounds 4, 3, 2; all status 1
INFEASIBLE_CASE = dict(shape=(4, 2, 16), seeds=(700, 701), admm_iters=1, max_rounds=1)        # status 2 for both


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def oracle_solve(oracle):
    return lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]


def boxes(oracle, prob, fu=0.5, fx=0.7):
    """(xlo, xhi, ulo, uhi) [N, n] / [N, m]: input bounds at fu of the mean unconstrained |u| of each channel, state bounds
    at fx of the largest unconstrained |x| of each state, widened where the trajectory of u = 0 needs more (feasible)"""
    n, m, N = prob.n, prob.m, prob.N
    Z = blocks(oracle_solve(oracle)(prob), n, m, N)
    x, u = Z[:, n:2 * n], Z[: N - 1, 2 * n:]
    uh = np.tile(fu * np.abs(u).mean(axis=0), (N, 1))
    roll = np.zeros_like(x)
    roll[0] = prob.x0
    for k in range(N - 1):
        roll[k + 1] = prob.A[k].reshape(n, n).T @ roll[k] + prob.d[k]
    xh = np.maximum(np.tile(fx * np.abs(x[1:]).max(axis=0), (N, 1)), 1.5 * np.abs(roll))
    return -xh, xh, -uh, uh


def admm_state(prob, solve, bounds, rho, alpha, eps, max_iter):
    """(z packed, v, y [N, n+m], iters, status) of box_support.admm_reference: what the device holds after the solve"""
    from box_support import admm_reference
    x, u, mx, mu_, lam, it, st = admm_reference(prob, solve, *bounds, rho, alpha, eps, eps, max_iter)
    z = np.concatenate([lam, x, u], axis=1).reshape(-1)[: prob.nvars]
    return z, np.concatenate([x, u], axis=1), np.concatenate([mx, mu_], axis=1) / rho, it, st


def admm_step_from(prob, solve, bounds, rho, alpha, v, y):
    """(z packed, mu [N, n+m]) after ONE warm-started iteration of box_support.admm_reference's loop from (v, y): what a
    constrained solve with warm_start and max_iter = 1 delivers, in the operation order of strict mode"""
    from box_support import masks, shifted_problem
    n, m, N = prob.n, prob.m, prob.N
    lo, hi, M = full_bounds(n, m, N, *bounds)
    Mx, Mu = masks(n, m, N, *bounds)
    q = np.concatenate([prob.q, prob.r], axis=1)
    v, y = np.where(M, v, 0.0), np.where(M, y, 0.0)
    t = y - v
    t = rho * t
    qt = np.where(M, q + t, q)
    Z = blocks(solve(shifted_problem(prob, rho, Mx, Mu, np.ascontiguousarray(qt[:, :n]), np.ascontiguousarray(qt[:, n:]))), n, m, N)
    zx = Z[:, n:]
    zh = alpha * zx + (1.0 - alpha) * v
    vn = np.minimum(np.maximum(zh + y, lo), hi)
    yn = np.where(M, (y + zh) - vn, 0.0)
    out = Z.copy()
    out[:, n:] = np.where(M, vn, zx)
    return out.reshape(-1)[: prob.nvars], rho * yn


def stationarity(prob, z, mu, bounds):
    from box_support import certificate
    return certificate(prob, z, mu[:, : prob.n], mu[:, prob.n:], *bounds, 0.0)


def sigma_sweep(ndlqr, oracle):
    """rows (sigma, total steps, worst ratio of the final stationarity to that of active_forward's solution on the same
    set, all status 1) over SWEEP_FAMILIES x SWEEP_SEEDS, each started from ADMM at eps 1e-3, default steps and rounds"""
    from box_grad_support import active_forward
    solve = oracle_solve(oracle)
    starts = []
    for n, m, N in SWEEP_FAMILIES:
        for seed in SWEEP_SEEDS:
            prob = synth(ndlqr, n, m, N, seed)
            b = boxes(oracle, prob)
            rho = float(prob.Q.mean())
            starts.append((prob, b, rho) + admm_state(prob, solve, b, rho, 1.6, 1e-3, 4000)[:3])
    rows = []
    for sg in SWEEP_SIGMAS:
        total, worst, ok = 0, 0.0, True
        for prob, b, rho, z, v, y in starts:
            o = polish_reference(prob, solve, b, z, v, y, rho, sigma=sg)
            zt, mt = active_forward(prob, o["codes"], *b)
            ratio = stationarity(prob, o["z"], o["mu"], b)["stationarity"] / stationarity(prob, zt, mt, b)["stationarity"]
            total += o["steps"]
            worst = max(worst, ratio)
            ok = ok and o["status"] == 1
        rows.append((sg, total, worst, ok))
    return rows


def sweep_winner(rows, bar=4.0):
    """the sigma with the fewest total steps among those within the bar (ties: the smaller sigma)"""
    good = [r for r in rows if r[3] and r[2] <= bar]
    return min(good, key=lambda r: (r[1], r[0]))[0] if good else None
