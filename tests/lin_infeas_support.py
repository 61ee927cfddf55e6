"""Independent references for the infeasibility detection of the solve with linear inequality constraints
(ndlqr_BatchSetConstraintInfeasibilityDetection, ndlqr_CopyBatchConstraintInfeasibilityCertificate).

Problems are the dicts of cost_support (math convention); rows C [N, p, n], D [N, p, m], lo, hi [N, p] as in lin_support.

- farkas_check_rows(): the four conditions of the certificate test and the four numbers behind them, evaluated in numpy
  longdouble from the problem data alone; it shares no code with the kernel. It also returns the sizes the rounding
  bounds of the tests are made of: the largest sum of absolute terms of an entry of e, and the sum of absolute terms of S.
- admm_infeas(): lin_support.admm (fixed rho, the operation order of strict mode) with the test behind the update and the
  convergence test of iteration `it`.
- check_kept_lambda(): a check as a function of the two iterates two cold solves deliver, through a solver handed in.
- family_a() -- "travelling": the m input rows |u| <= ubar plus one dense row c'x_knot <= level, with level `gap` below
  (infeasible) or above (the barely feasible twin) the SMALLEST value c'x_knot takes over the input box, from the condensed
  dynamics x_k = c_k + G_k U: c'c_k - ||c'G_k||_1 ubar. (A level below the largest reachable value would exclude nothing.)
  The certificate has to travel from the knot back to x0 through every input row on the way.
- family_b() -- "local": two rows with the same dense a at one knot, a'x <= -1 and a'x >= 1; the certificate is dlam = 0,
  dmu = (t, -t). Its feasible twin is the band -1.5 <= a'x - a'x_free <= -0.5 as two one-sided rows.
- instance(): the batch of the GPU tests -- problem 1 of cost_support.family infeasible, problems 0 and 2 twins -- with the
  float64 restatement of every member, computed once per (shape, horizon, family) and shared.
Test infrastructure.
"""
import functools

import numpy as np

import cost_support as cs
import lin_support as ls

RHO, ALPHA = ls.RHO, ls.ALPHA
EPS_ABS = EPS_REL = 1e-6
EVERY, EPS = 10, 1e-4
MAX_ITER = 1500

# knot, gap, ubar and seed of family A, and knot and seed of family B, per (n, m, N): chosen on the CPU so that the float64
# restatement certifies the infeasible member within MAX_ITER iterations and the twins converge within it (DESIGN.md
# section 3.20 tabulates them with the certification iterations)
CHOICE_A = {(6, 3, 5): dict(knot=2, gap=2.0, ubar=0.5, seed=1), (12, 4, 8): dict(knot=4, gap=1.0, ubar=0.3, seed=1),
            (7, 9, 16): dict(knot=2, gap=2.0, ubar=0.5, seed=1), (20, 5, 8): dict(knot=4, gap=2.0, ubar=0.5, seed=1)}
CHOICE_B = {(6, 3, 5): dict(knot=4, seed=2), (7, 9, 16): dict(knot=8, seed=2)}


def farkas_check_rows(prob, C, D, lo, hi, dlam, dmu, eps):
    """The certificate test in longdouble. C [N, p, n], D [N, p, m], lo, hi [N, p]; dlam [N, n], dmu [N, p]. Returns a dict:
    the four conditions `nonzero` (||dmu||_inf > 0), `stationary` (||e||_inf <= eps ||dmu||_inf), `qualified` (no row points
    to an infinite bound with |dmu_i| > eps ||dmu||_inf) and `negative` (S < -eps ||dmu||_inf), `ok` (all four, every number
    finite), the numbers e_inf, dmu_inf, inf_max (the largest |dmu_i| toward an infinite bound) and S, and the rounding
    sizes e_scale (largest sum of absolute terms of an entry of e) and S_scale (sum of absolute terms of S)."""
    ld = np.longdouble
    n, m, N = cs.dims(prob)
    p = C.shape[1]
    A, B = np.asarray(prob["A"], dtype=ld), np.asarray(prob["B"], dtype=ld)
    Cl, Dl = np.asarray(C, dtype=ld), np.asarray(D, dtype=ld)
    dl = np.asarray(dlam, dtype=ld).reshape(N, n)
    dm = np.asarray(dmu, dtype=ld).reshape(N, p)
    lo = np.asarray(lo, dtype=float).reshape(N, p)
    hi = np.asarray(hi, dtype=float).reshape(N, p)
    e_all, e_scale = [], ld(0)
    for k in range(N):
        ex = -dl[k] + Cl[k].T @ dm[k]
        sx = np.abs(dl[k]) + np.abs(Cl[k]).T @ np.abs(dm[k])
        if k < N - 1:
            ex = ex + A[k].T @ dl[k + 1]
            sx = sx + np.abs(A[k]).T @ np.abs(dl[k + 1])
            eu = B[k].T @ dl[k + 1] + Dl[k].T @ dm[k]
            su = np.abs(B[k]).T @ np.abs(dl[k + 1]) + np.abs(Dl[k]).T @ np.abs(dm[k])
            ex, sx = np.concatenate([ex, eu]), np.concatenate([sx, su])
        e_all.append(ex)
        e_scale = max(e_scale, sx.max())
    e_inf = np.abs(np.concatenate(e_all)).max()  # (numpy's max keeps a NaN)
    d_inf = np.abs(dm).max()
    tol = ld(eps) * d_inf
    x0, d = np.asarray(prob["x0"], dtype=ld), np.asarray(prob["d"], dtype=ld)
    S = -(x0 @ dl[0])
    S_scale = np.abs(x0) @ np.abs(dl[0])
    for k in range(N - 1):
        S -= d[k] @ dl[k + 1]
        S_scale += np.abs(d[k]) @ np.abs(dl[k + 1])
    inf_max = ld(0)
    for k in range(N):
        for r in range(p):
            v = dm[k, r]
            if v == 0:
                continue
            side = hi[k, r] if v > 0 else lo[k, r]
            if np.isfinite(side) and v == v:
                S += ld(side) * v
                S_scale += abs(ld(side) * v)
            elif abs(v) > inf_max or v != v:
                inf_max = abs(v)
    finite = bool(np.isfinite(e_inf) and np.isfinite(d_inf) and np.isfinite(S) and np.isfinite(inf_max))
    out = {"nonzero": bool(finite and d_inf > 0), "stationary": bool(finite and e_inf <= tol),
           "qualified": bool(finite and inf_max <= tol), "negative": bool(finite and S < -tol),
           "e_inf": e_inf, "dmu_inf": d_inf, "inf_max": inf_max, "S": S, "e_scale": e_scale, "S_scale": S_scale}
    out["ok"] = out["nonzero"] and out["stationary"] and out["qualified"] and out["negative"]
    return out


def admm_infeas(p, C, D, lo, hi, rho=RHO, alpha=ALPHA, eps_abs=EPS_ABS, eps_rel=EPS_REL, max_iter=MAX_ITER, every=EVERY,
                eps=EPS, trace=None):
    """lin_support.admm in float64 with the certificate test at the iterations it >= 2, it % every == 0, behind the update
    and the convergence test of that iteration. Returns dict(status, iters, dlam [N, n], dmu [N, p], z, v, y): status 1
    converged, 2 max_iter, 3 not finite, 4 certified at `iters` (dlam, dmu are the differences of that iteration; zeros
    otherwise). trace: a list that takes (it, dlam, dmu, check) of every check."""
    n, m, N = cs.dims(p)
    M = np.isfinite(lo) | np.isfinite(hi)
    K, b = ls.kkt_ld(ls.shifted_problem(p, C, D, lo, hi, rho))
    solve = ls.Solver(K)
    oma = 1.0 - alpha
    v = np.zeros((N, C.shape[1]))
    y = np.zeros_like(v)
    mx = lambda a: float(np.abs(a).max()) if a.size else 0.0
    zero = dict(dlam=np.zeros((N, n)), dmu=np.zeros_like(v))
    lam_prev = mu_prev = z = None
    for it in range(1, max_iter + 1):
        z = solve(b - ls.perturbation(p, C, D, np.where(M, rho * (y - v), 0.0)))
        w = ls.rows_of(p, C, D, z)
        wh = alpha * w + oma * v
        vn = np.where(M, np.minimum(np.maximum(wh + y, lo), hi), 0.0)
        yn = np.where(M, (y + wh) - vn, 0.0)
        r_prim = mx((w - vn)[M])
        r_dual = rho * mx(ls.perturbation(p, C, D, vn - v))
        sp = max(mx(w[M]), mx(vn[M]))
        sd = rho * mx(ls.perturbation(p, C, D, yn))
        finite = all(np.isfinite(a) for a in (r_prim, r_dual, sp, sd))
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v, y = vn, yn
        if conv or not finite:
            return dict(status=1 if conv else 3, iters=it, z=z, v=v, y=y, **zero)
        lam, mu = cs.split(z, n, m, N)[0], rho * y
        if every > 0 and it >= 2 and it % every == 0:
            dlam, dmu = lam - lam_prev, mu - mu_prev
            c = farkas_check_rows(p, C, D, lo, hi, dlam, dmu, eps)
            if trace is not None:
                trace.append((it, dlam, dmu, c))
            if c["ok"]:
                return dict(status=4, iters=it, z=z, v=v, y=y, dlam=dlam, dmu=dmu)
        lam_prev, mu_prev = lam, mu
    return dict(status=2, iters=max_iter, z=z, v=v, y=y, **zero)


def check_kept_lambda(bs, inst, it, every, eps, settings, label=()):
    """The body of test_kept_lambda_is_the_delivered_one (test_gpu_lin_infeas.py), shared with test_gpu_lin_shapes.py. bs:
    a solver in constrained mode with the batch `inst` (dicts p, C, D, lo, hi), detection off. Two cold solves stopped at
    it - 1 and it deliver the iterates whose differences a check at `it` judges; a third with a check every `every`
    iterations (it % every == 0, no other check before it) leaves the measures: D and the infinite-side maximum bit for
    bit, ||e||_inf within (n + p + 2) eps x the largest sum of absolute terms of an entry, S within
    4 eps^2 sum |terms| + eps |S|. Every solve must end as status 2 at its max_iter. Returns the checks per problem."""
    ld, eps64 = np.longdouble, np.finfo(float).eps
    n, m, N = cs.dims(inst[0]["p"])
    stop = []
    for mi in (it - 1, it):
        iters, status = bs.solve_constrained(max_iter=mi, **settings)
        assert (iters == mi).all() and (status == 2).all()
        stop.append((np.stack([cs.split(z, n, m, N)[0] for z in bs.solutions()]), bs.constraint_multipliers()))
    bs.set_constraint_infeasibility(every, eps)
    iters, status = bs.solve_constrained(max_iter=it, **settings)
    assert (iters == it).all() and (status == 2).all()
    meas, at = bs.constraint_infeasibility_measures()
    bs.set_constraint_infeasibility(0)
    assert (at == it).all()
    p_rows = inst[0]["C"].shape[1]
    out = []
    for i, c in enumerate(inst):
        dlam, dmu = stop[1][0][i] - stop[0][0][i], stop[1][1][i] - stop[0][1][i]
        chk = farkas_check_rows(c["p"], c["C"], c["D"], c["lo"], c["hi"], dlam, dmu, eps)
        print(*label, "problem", i, "device", ["%.17e" % x for x in meas[i]], "from the iterates",
              ["%.17e" % float(chk[k]) for k in ("e_inf", "dmu_inf", "inf_max", "S")])
        assert meas[i][1] == float(chk["dmu_inf"]) and chk["dmu_inf"] > 0
        assert meas[i][2] == float(chk["inf_max"])
        assert abs(ld(meas[i][0]) - chk["e_inf"]) <= (n + p_rows + 2) * eps64 * chk["e_scale"]
        assert abs(ld(meas[i][3]) - chk["S"]) <= 4 * eps64 * eps64 * chk["S_scale"] + eps64 * abs(chk["S"])
        out.append(chk)
    return out


def condensed(p):
    """(G [N, n, (N-1) m], c [N, n]): x_k = c_k + G_k U of the dynamics of a problem dict"""
    n, m, N = cs.dims(p)
    G = np.zeros((N, n, (N - 1) * m))
    c = np.zeros((N, n))
    c[0] = p["x0"]
    for k in range(N - 1):
        G[k + 1] = p["A"][k] @ G[k]
        G[k + 1][:, k * m:(k + 1) * m] += p["B"][k]
        c[k + 1] = p["A"][k] @ c[k] + p["d"][k]
    return G, c


def family_a(p, knot, gap, ubar, seed, feasible):
    """(C, D, lo, hi) with m + 1 rows per knot: |u_k| <= ubar for k < N-1 and c'x_knot <= level; level = (the smallest
    c'x_knot over the input box) - gap, or + gap when `feasible`. c: seeded, N(0, 1) / sqrt(n)."""
    n, m, N = cs.dims(p)
    rng = np.random.default_rng([seed, n, m, N, 41])
    c = rng.standard_normal(n) / np.sqrt(n)
    G, c0 = condensed(p)
    reach = float(c @ c0[knot] - np.abs(c @ G[knot]).sum() * ubar)
    C = np.zeros((N, m + 1, n))
    D = np.zeros((N, m + 1, m))
    D[:, :m, :] = np.eye(m)
    C[knot, m] = c
    lo = np.full((N, m + 1), -np.inf)
    hi = np.full((N, m + 1), np.inf)
    lo[: N - 1, :m] = -float(ubar)
    hi[: N - 1, :m] = float(ubar)
    hi[knot, m] = reach + gap if feasible else reach - gap
    return C, D, lo, hi


def family_b(p, knot, seed, feasible, z_free=None):
    """(C, D, lo, hi) with two rows per knot, both a'x at `knot`: a'x <= -1 and a'x >= 1 (no point), or, when `feasible`,
    a'x <= t - 0.5 and a'x >= t - 1.5 with t = a'x_knot of the unconstrained solution z_free (the upper row active). a: seeded, N(0, 1) / sqrt(n)."""
    n, m, N = cs.dims(p)
    rng = np.random.default_rng([seed, n, m, N, 43])
    a = rng.standard_normal(n) / np.sqrt(n)
    C = np.zeros((N, 2, n))
    D = np.zeros((N, 2, m))
    C[knot, 0] = a
    C[knot, 1] = a
    lo = np.full((N, 2), -np.inf)
    hi = np.full((N, 2), np.inf)
    t = float(a @ cs.split(np.asarray(z_free, dtype=float), n, m, N)[1][knot]) if feasible else 0.0
    hi[knot, 0] = t - 0.5 if feasible else -1.0
    lo[knot, 1] = t - 1.5 if feasible else 1.0
    return C, D, lo, hi


@functools.lru_cache(maxsize=None)
def instance(n, m, N, fam):
    """The batch of the GPU tests for one (shape, horizon, family 'A' | 'B'): a list of three dicts (p, C, D, lo, hi, ref)
    -- problem 1 infeasible, problems 0 and 2 its feasible twins -- with ref = admm_infeas() of each. Read-only."""
    probs = cs.family(n, m, N, "moderate")
    out = []
    for i, p in enumerate(probs["probs"]):
        if fam == "A":
            rows = family_a(p, feasible=i != 1, **CHOICE_A[(n, m, N)])
        else:
            rows = family_b(p, feasible=i != 1, z_free=probs["z"][i], **CHOICE_B[(n, m, N)])
        for a in rows:
            a.setflags(write=False)
        out.append(dict(p=p, C=rows[0], D=rows[1], lo=rows[2], hi=rows[3], ref=admm_infeas(p, *rows)))
    return out
