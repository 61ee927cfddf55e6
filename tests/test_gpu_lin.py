"""General linear inequality constraints lo <= C x + D u <= hi on the device (ndlqr_InitializeBatchFlatConstrained,
ndlqr_SolveBatchLinConstrained) against lin_support.py: the numpy restatement of the iteration in
float64 and in longdouble. Batch 3, the "moderate" family of cost_support.py, shapes (6,3), (12,4), (7,9) (m > n, padded
block size), (20,5); horizons 2 (one dynamics knot), 5 (padded), 8, 16; default and strict mode; rho = 1, alpha = 1.6.
Rows per knot: the m input rows plus two dense rows (lin_support.constraint_rows).

Bars. Shifted costs, records and reduced problem, per array and entry: 8 x the float64 restatement's own largest error
against the longdouble one, at least 16 eps of the array's largest entry (test 1 of test_gpu_cost.py). First iterations,
per field and entry: FIRST_MULT (strict mode: FIRST_MULT_STRICT) x the float64 restatement's own error on the same case,
at least 16 eps of the field's largest entry; the multiples are twice the largest ratio measured over all cases on the
MI355X, at least 8 (the table is in DESIGN.md section 3.17). The restatement's re-solve is a dense LU with partial pivoting,
the device's the nested-dissection solve on the reduced problem, whose plain solutions sit at 1e-13 .. 2e-11 of the refined
ones on this family: the ratios of 100 .. 1400 are that distance, not the update kernel's. Converged solves: status and iteration count of the float64 restatement +-2, the KKT conditions
to lin_support.kkt_bar, the dynamics rows to the parity contract 1e-9."""
import functools

import numpy as np
import pytest

import cost_support as cs
import lin_support as ls

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5)]
CASES = [(n, m, N) for (n, m) in SHAPES for N in (2, 5, 8, 16)]
SET = dict(rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8)
# twice the largest ratio measured over all cases on the MI355X, at least 8 (DESIGN.md section 3.17 has the table): the
# default mode, whose re-solve is the fast separator-only schedule, and strict mode
FIRST_MULT = 2830.0         # (largest ratio 1414.59, (6,3,16))
FIRST_MULT_STRICT = 1820.0  # (largest ratio 909.82, (12,4,8))


def first_mult(ndlqr, flags):
    return FIRST_MULT_STRICT if flags & ndlqr.FLAG_STRICT_FP else FIRST_MULT


REL_TOL = 1e-9
RED_NAMES = ("Qs", "Hs", "Rs", "L", "LR", "G", "At", "Bt", "qt", "rt", "dt", "x0t")


def modes(ndlqr):
    return [0, ndlqr.FLAG_STRICT_FP]


def constrained_solver(ndlqr, cases, flags=0, lo=None, hi=None):
    probs = [c["p"] for c in cases]
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    C, D, l, h = ls.flat_rows(cases)
    bs.initialize_flat_constrained(*cs.flat(probs), C, D, l if lo is None else lo, h if hi is None else hi)
    assert bs.is_constrained() and bs.cost_is_dense()
    return bs


@functools.lru_cache(maxsize=None)
def first_ld(n, m, N):
    """the first three iterates of the longdouble restatement, per problem of the case"""
    out = []
    for c in ls.case(n, m, N):
        trace = []
        ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], max_iter=3, dtype=np.longdouble, trace=trace)
        out.append(trace)
    return out


def fields(z, n, m, N):
    return dict(zip(("lam", "x", "u"), cs.split(z, n, m, N)))


# ---------------------------------------------------------------------------- 1: shifted costs and records, entry by entry
def restated_reduction(cases, dtype):
    """the shifted costs Qs, Hs, Rs and the reduction of the shifted problem of every case, restated in `dtype`, in the
    layout of constraint_reduction()"""
    reds, costs = [], []
    for c in cases:
        ps = ls.shifted_problem(c["p"], c["C"], c["D"], c["lo"], c["hi"], ls.RHO, dtype)
        reds.append(cs.reduce(ps, dtype))
        costs.append(ps)
    out = cs.reduction_flat(reds)
    for k, name in (("Q", "Qs"), ("H", "Hs"), ("R", "Rs")):
        a = np.stack([p[k] for p in costs])
        out[name] = a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1)
    return out


def check_shifted_reduction(got, cases, label):
    """the rule of test 1: per array, the largest error against the longdouble restatement within 8 x the float64
    restatement's own, at least 16 eps of the array's largest entry"""
    N = cases[0]["C"].shape[0]
    exact, f64 = restated_reduction(cases, np.longdouble), restated_reduction(cases, np.float64)
    for k in RED_NAMES:
        # (H, R of the last knot are not part of the problem: the device writes 0 and 1 there)
        cut = slice(0, N - 1) if k in ("Hs", "Rs") else slice(0, N)
        g, e, f = got[k][:, cut], exact[k][:, cut], f64[k][:, cut]
        own = float(np.abs(f - e).max())
        bar = max(8 * own, 16 * EPS * float(np.abs(e).max()))
        err = float(np.abs(g - e).max())
        print("shifted", label, k, "device %.3e numpy %.3e ratio to bar %.3f" % (err, own, err / bar))
        assert g.shape == e.shape and np.isfinite(g).all()
        assert err <= bar, (k, err, bar)


@pytest.mark.parametrize("n,m,N", CASES)
def test_shifted_reduction_per_entry(ndlqr, n, m, N):
    cases = ls.case(n, m, N)
    bs = constrained_solver(ndlqr, cases)
    bs.solve_constrained(max_iter=1, **SET)
    got = bs.constraint_reduction()
    bs.close()
    check_shifted_reduction(got, cases, (n, m, N))


# ---------------------------------------------------------------------------- 2: the first iterations
def ratio_of(got, ref, own):
    """largest error of `got` / error of `own` against `ref` over the fields (dicts of arrays), among the fields whose
    error is above the floor of 16 eps of the field's largest entry (0: all below it)"""
    worst = 0.0
    for k in got:
        floor = 16 * EPS * float(np.abs(ref[k]).max())
        err, mine = float(np.abs(got[k] - ref[k]).max()), float(np.abs(own[k] - ref[k]).max())
        if err > floor:  # (below the floor the entry passes whatever the multiple)
            worst = max(worst, err / mine if mine > 0 else np.inf)
    return worst


def first_iteration_ratios(ndlqr, n, m, N, flags):
    """(largest device error / the float64 restatement's own error over v, mu and the fields of z after max_iter = 1, 2, 3;
    the same for z of max_iter = 1 alone; the same for the PLAIN dense-cost solve of the shifted problem, which is what
    the first re-solve of a cold start computes: y = v = 0)"""
    cases = ls.case(n, m, N)
    exact = first_ld(n, m, N)
    bs = constrained_solver(ndlqr, cases, flags)
    worst, z1 = 0.0, 0.0
    for it in (1, 2, 3):
        iters, status = bs.solve_constrained(max_iter=it, **SET)
        assert (iters == it).all() and (status == 2).all()
        Z, mu, v = bs.solutions(), bs.constraint_multipliers(), bs.constraint_reduction()["v"]
        for i, c in enumerate(cases):
            e, f = exact[i][it - 1], c["first"][it - 1]
            got = dict(v=v[i], mu=mu[i], **fields(Z[i], n, m, N))
            ref = dict(v=e["v"], mu=ls.RHO * e["y"], **fields(e["z"], n, m, N))
            own = dict(v=f["v"], mu=ls.RHO * f["y"], **fields(f["z"], n, m, N))
            worst = max(worst, ratio_of(got, ref, own))
            if it == 1:
                z1 = max(z1, ratio_of(fields(Z[i], n, m, N), fields(e["z"], n, m, N), fields(f["z"], n, m, N)))
    bs.close()
    shifted = [ls.shifted_problem(c["p"], c["C"], c["D"], c["lo"], c["hi"], ls.RHO) for c in cases]
    ps = ndlqr.BatchSolver(n, m, N, len(cases), flags=flags)
    ps.initialize_flat_dense(*cs.flat(shifted))
    assert ps.solve() == 0
    Zp = ps.solutions()
    ps.close()
    plain = max(ratio_of(fields(Zp[i], n, m, N), fields(exact[i][0]["z"], n, m, N), fields(c["first"][0]["z"], n, m, N))
                for i, c in enumerate(cases))
    return worst, z1, plain


@pytest.mark.parametrize("n,m,N", CASES)
def test_first_iterations_per_entry(ndlqr, n, m, N):
    ratios = {flags: first_iteration_ratios(ndlqr, n, m, N, flags) for flags in modes(ndlqr)}
    for flags, (ratio, z1, plain) in ratios.items():
        print("first iterations", (n, m, N), "flags", flags, "largest error / restatement's own: %.2f" % ratio,
              "| z after one iteration: %.2f | plain solve of the shifted problem: %.2f" % (z1, plain))
    for flags, (ratio, _, _) in ratios.items():
        assert ratio <= first_mult(ndlqr, flags), (flags, ratio)


# ---------------------------------------------------------------------------- 3: converged solves
def check_converged(c, z, mu, res):
    """what test 3 asks of a converged solution: the KKT conditions in the caller's variables to lin_support.kkt_bar and
    the dynamics rows of the delivered z to the parity contract"""
    p = c["p"]
    n, m, N = cs.dims(p)
    bar = ls.kkt_bar(p, c["C"], c["D"], z, res)
    got = ls.kkt_violation(p, c["C"], c["D"], c["lo"], c["hi"], z, mu, bar["tol"])
    assert got["stationarity"] <= bar["stationarity"], (got, bar)
    assert got["feasibility"] <= bar["feasibility"], (got, bar)
    assert got["complementarity"] == 0.0, got
    _, x, u = cs.split(z.astype(np.longdouble), n, m, N)
    dyn = [np.abs(x[0] - p["x0"]).max()]
    for k in range(N - 1):
        dyn.append(np.abs(x[k + 1] - (p["A"][k] @ x[k] + p["B"][k] @ u[k] + p["d"][k])).max())
    assert float(max(dyn)) <= REL_TOL * float(np.abs(x).max()), max(dyn)


@pytest.mark.parametrize("n,m,N", CASES)
def test_converged_solves(ndlqr, n, m, N):
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        iters, status = bs.solve_constrained(max_iter=2000, **SET)
        Z, mu, res = bs.solutions(), bs.constraint_multipliers(), bs.constraint_residuals()
        bs.close()
        print("converged", (n, m, N), "flags", flags, "device", list(iters), list(status), "restatement",
              [c["ref"]["iters"] for c in cases], [c["ref"]["status"] for c in cases])
        for i, c in enumerate(cases):
            if c["ref"]["status"] != 1:
                continue  # (a seed ADMM does not converge on at rho = 1: reported above, run by test_statuses)
            assert status[i] == 1 and abs(int(iters[i]) - c["ref"]["iters"]) <= 2
            check_converged(c, Z[i], mu[i], res[i])
        assert sum(c["ref"]["status"] == 1 for c in cases) >= 1


# ---------------------------------------------------------------------------- 4: the box special case
@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8), (7, 9, 16)])
def test_selector_rows_against_solve_box(ndlqr, n, m, N):
    """Rows that select every x and u entry on a diagonal cost, against solve_box on a diagonal context with the same rho,
    alpha, eps. After 1, 2, 3 iterations the bounded entries (v), the rest of the re-solve (lambda and the unbounded
    entries) and the multipliers of the two solvers agree to the bar of test 2: first_mult x the float64 restatement's own
    error, at least 16 eps of the field's largest entry; the measured ratio is printed. At convergence: the same statuses,
    iteration counts within 2 of each other and of the restatement, and the constrained solve's solution passes what test
    3 checks (KKT conditions to lin_support.kkt_bar, dynamics to 1e-9)."""
    import rslqr_amd
    cases, diag = [], []
    for i in range(cs.BATCH):
        p, Qd, Rd = cs.diagonal_problem(n, m, N, 41 + i)
        K, b = cs.dense_kkt(p)
        _, x, u = cs.split(cs.refined_solve(K, b), n, m, N)
        # (inputs at 0.6 of the unconstrained range, states at 0.9: tighter state bounds are infeasible on these seeds)
        xhi = 0.9 * np.abs(x).max(axis=0) * np.ones((N, n)); uhi = 0.6 * np.abs(u).max(axis=0) * np.ones((N, m))
        C, D, lo, hi = ls.selector_rows(n, m, N, -xhi, xhi, -uhi, uhi)
        cases.append(dict(p=p, C=C, D=D, lo=lo, hi=hi))
        diag.append((rslqr_amd.generate_synthetic(n, m, N, 41 + i), xhi, uhi))
    M = np.stack([np.isfinite(c["lo"]) | np.isfinite(c["hi"]) for c in cases])
    for flags in modes(ndlqr):
        lin = constrained_solver(ndlqr, cases, flags)
        box = ndlqr.BatchSolver(n, m, N, cs.BATCH, flags=flags)
        box.initialize_flat(*[np.stack([g[k] for g, _, _ in diag]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")])
        box.set_bounds(np.stack([-a for _, a, _ in diag]), np.stack([a for _, a, _ in diag]),
                       np.stack([-a for _, _, a in diag]), np.stack([a for _, _, a in diag]))
        for max_iter in (1, 2, 3, 2000):
            il, sl = lin.solve_constrained(max_iter=max_iter, **SET)
            ib, sb = box.solve_box(max_iter=max_iter, **SET)
            Zl, vl, mul = lin.solutions(), lin.constraint_reduction()["v"], lin.constraint_multipliers()
            Zb = box.solutions()
            mux, muu = box.bound_multipliers()
            print("box case", (n, m, N), flags, max_iter, "lin", list(il), list(sl), "box", list(ib), list(sb))
            assert (sl == sb).all() and (np.abs(il.astype(int) - ib.astype(int)) <= (2 if max_iter > 3 else 0)).all(), (il, ib, sl, sb)
            res = lin.constraint_residuals()
            for i, c in enumerate(cases):
                if max_iter > 3:
                    if sl[i] != 1:
                        continue  # (a seed ADMM does not converge on at rho = 1: both solvers say so, above)
                    ref = ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"])
                    assert ref["status"] == 1 and abs(int(il[i]) - ref["iters"]) <= 2, (il[i], ref["iters"], ref["status"])
                    check_converged(c, Zl[i], mul[i], res[i])
                    continue
                trace, trace_ld = [], []
                ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], max_iter=max_iter, trace=trace)
                ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], max_iter=max_iter, dtype=np.longdouble, trace=trace_ld)
                e, f = trace_ld[-1], trace[-1]
                dz = cs.split(f["z"] - e["z"], n, m, N)
                own = dict(lam=dz[0], xu=np.concatenate(dz[1:], axis=1), mu=ls.RHO * (f["y"] - e["y"]))
                lam_l, x_l, u_l = cs.split(Zl[i], n, m, N)
                lam_b, x_b, u_b = cs.split(Zb[i], n, m, N)
                xu_l = np.where(M[i], vl[i], np.concatenate([x_l, u_l], axis=1))  # (what box_finish delivers)
                xu_b = np.concatenate([x_b, u_b], axis=1)
                mu_b = np.concatenate([mux[i], muu[i]], axis=1)
                for k, (a, b_) in dict(lam=(lam_l, lam_b), xu=(xu_l, xu_b), mu=(mul[i], mu_b)).items():
                    mine = float(np.abs(own[k]).max())
                    bar = max(first_mult(ndlqr, flags) * mine, 16 * EPS * float(np.abs(b_).max()))
                    err = float(np.abs(a - b_).max())
                    print("box case", (n, m, N), flags, max_iter, i, k, "lin - box %.3e, / restatement's own %.2f, bar %.3e"
                          % (err, err / mine if mine > 0 else np.inf, bar))
                    assert err <= bar, (k, err, bar)
        lin.close(); box.close()


# ---------------------------------------------------------------------------- 5: statuses
def test_statuses(ndlqr):
    n, m, N = 6, 3, 8
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        iters, status = bs.solve_constrained(max_iter=2000, **SET)
        Z, mu = bs.solutions(), bs.constraint_multipliers()
        assert (status == 1).all()
        # a warm start after convergence takes one iteration
        it2, st2 = bs.solve_constrained(max_iter=2000, warm_start=True, **SET)
        assert (it2 == 1).all() and (st2 == 1).all(), (it2, st2)
        bs.close()
        # a NaN in one problem: status 3 there, the others bit for bit as without it
        bad = [dict(c) for c in cases]
        bad[1] = dict(bad[1], p=dict(bad[1]["p"], q=bad[1]["p"]["q"].copy()))
        bad[1]["p"]["q"][3, 2] = np.nan
        bs = constrained_solver(ndlqr, bad, flags)
        itn, stn = bs.solve_constrained(max_iter=2000, **SET)
        Zn, mun = bs.solutions(), bs.constraint_multipliers()
        bs.close()
        assert stn[1] == 3 and list(stn[[0, 2]]) == [1, 1] and list(itn[[0, 2]]) == list(iters[[0, 2]])
        for i in (0, 2):
            assert np.array_equal(Zn[i], Z[i]) and np.array_equal(mun[i], mu[i])
        # all bounds infinite: converged in iteration 1 with the unconstrained solution
        inf = np.full((cs.BATCH, N, m + 2), np.inf)
        bs = constrained_solver(ndlqr, cases, flags, lo=-inf, hi=inf)
        assert bs.solve() == 0
        Zu = bs.solutions()
        it1, st1 = bs.solve_constrained(max_iter=50, **SET)
        assert (it1 == 1).all() and (st1 == 1).all()
        fam = cs.family(n, m, N, "moderate")
        for i in range(cs.BATCH):
            assert max(cs.field_errors(bs.solutions()[i], fam["z"][i], n, m, N)) <= REL_TOL
            assert max(cs.field_errors(Zu[i], fam["z"][i], n, m, N)) <= REL_TOL
        assert np.array_equal(bs.constraint_multipliers(), np.zeros((cs.BATCH, N, m + 2)))
        bs.close()


def test_max_iter_and_a_seed_that_does_not_converge(ndlqr):
    """(12,4,2): two of the three seeds do not converge within 2000 iterations at rho = 1 in the restatement. At max_iter =
    150 every problem still running reports status 2 and iters = 150, and its residual row is the restatement's at that
    iteration (the iterates agree to test 2's bars and the four numbers are maxima of them times rho and column sums of
    [C D] of order 1: 1e-6 of each number, floor 1e-12)."""
    n, m, N = 12, 4, 2
    cases = ls.case(n, m, N)
    assert sum(c["ref"]["status"] == 2 for c in cases) == 2
    traces = []
    for c in cases:
        t = []
        ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], max_iter=150, trace=t)
        traces.append(t)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        iters, status = bs.solve_constrained(max_iter=150, check_every=7, **SET)
        res = bs.constraint_residuals()
        bs.close()
        for i, c in enumerate(cases):
            t = traces[i]
            if len(t) < 150:  # (this seed converges)
                assert status[i] == 1 and abs(int(iters[i]) - len(t)) <= 2, (i, iters, status)
                continue
            assert status[i] == 2 and int(iters[i]) == 150, (i, iters, status)
            ref = np.array([float(a) for a in t[-1]["resid"]])
            print("resid", i, res[i], ref)
            assert (np.abs(res[i] - ref) <= 1e-6 * np.abs(ref) + 1e-12).all(), (res[i], ref)


# ---------------------------------------------------------------------------- 6: state
def test_state(ndlqr):
    n, m, N = 12, 4, 8
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        assert bs.solve() == 0
        Z0 = bs.solutions()
        iters, status = bs.solve_constrained(max_iter=2000, **SET)
        Zc = bs.solutions()
        assert not np.array_equal(Zc, Z0)
        assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z0)  # a plain solve before and after: the same bits
        # a new right-hand side: S^' of it and the iterations, no factorisation
        iters, status = bs.solve_constrained(max_iter=2000, **SET)
        assert np.array_equal(bs.solutions(), Zc)
        fc = bs.factor_count()
        rng = np.random.default_rng(5)
        new = [dict(c, p=dict(c["p"], q=c["p"]["q"] + 0.1 * rng.standard_normal((N, n)), x0=c["p"]["x0"] * 1.1)) for c in cases]
        _, _, _, _, _, q, r, d, x0 = cs.flat([c["p"] for c in new])
        bs.set_rhs_flat(q, r, d, x0)
        it2, st2 = bs.solve_constrained(max_iter=2000, **SET)
        assert bs.factor_count() == fc
        for i, c in enumerate(new):
            ref = ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"])
            assert st2[i] == ref["status"] and abs(int(it2[i]) - ref["iters"]) <= 2, (it2, st2, ref["iters"])
        # new bounds, the same pattern: the factorisation is kept; a new pattern drops it
        C, D, lo, hi = ls.flat_rows(cases)
        bs.set_constraint_bounds(1.1 * lo, 1.1 * hi)
        bs.solve_constrained(max_iter=5, **SET)
        assert bs.factor_count() == fc
        lo2 = lo.copy(); hi2 = hi.copy()
        lo2[:, :, 0] = -np.inf; hi2[:, :, 0] = np.inf
        bs.set_constraint_bounds(lo2, hi2)
        bs.solve_constrained(max_iter=5, **SET)
        assert bs.factor_count() == fc + 1
        assert np.array_equal(bs.constraint_multipliers()[:, :, 0], np.zeros((cs.BATCH, N)))
        # the dense initialiser leaves constrained mode
        bs.initialize_flat_dense(*cs.flat([c["p"] for c in cases]))
        assert bs.cost_is_dense() and not bs.is_constrained()
        with pytest.raises(RuntimeError, match="ndlqr_hip_solve_constrained: the solver is not in constrained mode"):
            bs.solve_constrained(max_iter=5, **SET)
        assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z0)
        bs.close()


# ---------------------------------------------------------------------------- 7: refusals by name
def test_refusals_by_name(ndlqr):
    n, m, N = 6, 3, 5
    cases = ls.case(n, m, N)
    probs = [c["p"] for c in cases]
    arrs = cs.flat(probs)
    C, D, lo, hi = ls.flat_rows(cases)
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    z = lambda *s: np.zeros(s)
    with pytest.raises(RuntimeError, match=r"ndlqr_hip_init_constrained: p = 0"):
        bs.initialize_flat_constrained(*arrs, z(cs.BATCH, N, 0), z(cs.BATCH, N, 0), z(cs.BATCH, N, 0), z(cs.BATCH, N, 0))
    with pytest.raises(RuntimeError, match="ndlqr_hip_solve_constrained: the solver is not in constrained mode"):
        bs.solve_constrained()
    hi_bad = hi.copy(); hi_bad[1, 2, 0] = lo[1, 2, 0] - 1.0
    with pytest.raises(RuntimeError, match="ndlqr_hip_init_constrained: a lower bound exceeds its upper bound"):
        bs.initialize_flat_constrained(*arrs, C, D, lo, hi_bad)
    assert not bs.is_constrained()
    P = 4000  # rows per knot whose staging exceeds the LDS of a workgroup
    with pytest.raises(RuntimeError, match="ndlqr_hip_init_constrained: lin_update stages .* beyond the 163840 bytes of LDS"):
        bs.initialize_flat_constrained(*arrs, z(cs.BATCH, N, P * n), z(cs.BATCH, N, P * m), z(cs.BATCH, N, P), z(cs.BATCH, N, P))
    bs.initialize_flat_constrained(*arrs, C, D, lo, hi)
    with pytest.raises(RuntimeError, match="ndlqr_hip_set_constraint_bounds: a lower bound exceeds its upper bound"):
        bs.set_constraint_bounds(lo, hi_bad)
    nan = lo.copy(); nan[0, 0, 0] = np.nan
    with pytest.raises(RuntimeError, match="ndlqr_hip_set_constraint_bounds: a lower bound exceeds its upper bound"):
        bs.set_constraint_bounds(nan, hi)
    with pytest.raises(RuntimeError, match="ndlqr_hip_solve_constrained: the adaptive penalty"):
        bs.solve_constrained(adapt_every=5, **SET)
    # the refused bounds replaced nothing: the solve is that of the bounds of the initialiser
    iters, status = bs.solve_constrained(max_iter=2000, **SET)
    assert [int(i) for i in iters] == [c["ref"]["iters"] for c in cases] or (np.abs(iters - [c["ref"]["iters"] for c in cases]) <= 2).all()
    # no adjoint through the constrained solve, and no MPC step in this mode
    with pytest.raises(RuntimeError, match="ndlqr_hip_solve_constrained"):
        if bs.solve_adjoint(np.zeros((cs.BATCH, bs.nvars))) != 0:
            raise RuntimeError(bs.L.ndlqr_hip_last_error().decode())
    # the box entry points stay refused: constrained mode is a dense-cost mode
    with pytest.raises(RuntimeError, match="ndlqr_hip_set_bounds"):
        bs.set_bounds(ulo=-np.ones(m), uhi=np.ones(m))
    with pytest.raises(RuntimeError, match="ndlqr_hip_solve_box"):
        bs.solve_box()
    # memory of another device: needs a second GPU. On a box with one MI355X, where the suite usually runs, these two
    # refusals are NOT exercised; the CallerArrays path they take is the one test_gpu_cost.py and test_gpu_box.py share.
    if ndlqr.device_count() > 1:
        import torch

        class Foreign:
            def __init__(self, a):
                self.t = torch.from_numpy(a).to("cuda:1")
                self.ptr, self.size = self.t.data_ptr(), self.t.numel()
        with pytest.raises(RuntimeError, match="ndlqr_hip_init_constrained: an input lies in the memory of another device"):
            bs.initialize_flat_constrained(*arrs, Foreign(C), D, lo, hi)
        with pytest.raises(RuntimeError, match="ndlqr_hip_set_constraint_bounds: bounds lie in the memory of another device"):
            bs.set_constraint_bounds(Foreign(lo), Foreign(hi))
    bs.close()
