"""The active-set polish of the solve with linear inequality rows on the device (ndlqr_PolishBatchLinConstrained;
DESIGN.md section 3.23) against lin_polish_support.py: the numpy restatement in float64 and in longdouble, and the direct
solve of the bordered active-set system. Batch 3, the "moderate" family of cost_support.py with the rows of
lin_support.constraint_rows, shapes (6,3), (12,4), (7,9) (m > n, padded block size), (20,5); horizons 2 (one dynamics
knot), 5 (padded), 8, 16; default and strict mode.

Bars. Residual kernel and first steps, per field and entry: a multiple M of the float64 restatement's own error against the
longdouble one on the same input, at least 16 eps of the field's largest entry. Converged: the stationarity of a status-1
problem at most M x that of active_direct, both evaluated in longdouble. The multiples are twice the largest ratio measured
over all cases and both modes on the MI355X, at least 8 (section 3.17's practice; DESIGN.md section 3.23 and
profiles/lin_polish_accuracy.txt have the table):
    RESIDUAL_MULT   the residual kernel alone. The device accumulates every row in double-double and rounds once; the
                    longdouble restatement's rows are exact rational sums rounded once, the float64 restatement's longdouble
                    sums rounded once: the device stays below the floor in 15 of 16 cases (largest ratio 0.39)
    STEP_MULT       the candidate z, mu of max_steps = 1, 2: the device's re-solve (nested dissection on the reduced problem)
                    against the restatement's dense LU, as FIRST_MULT of test_gpu_lin.py
    STEP_NORM_MULT  the norm slots of the same runs. Slot 0 is a residual kernel's output; the norm AFTER a step is what the
                    re-solve left of a right-hand side of size sigma_p |r_c| (1e5 here): its backward error, 1e-11 .. 1e-10
                    on the device and two to five orders below that for the dense LU of the float64 restatement, whose own
                    error against the longdouble restatement is then 1e-16 .. 1e-13. The ratio of the two is not a property of
                    the kernels under test; twice the largest measured is what the rule gives, and the candidate's fields
                    carry the check
    DIRECT_MULT     final stationarity over that of the direct solve: 1.00 in every case -- both sit at the rounding of z
Every restatement starts from the DEVICE's own ADMM iterate (z, v, y, status), so the codes and sigma_p are compared
exactly. Statuses, final codes and rounds equal the restatement's in all 96 runs (16 cases x 3 problems x 2 modes), the
accepted steps within one (the largest difference measured: 1), 4 of 48 problems stay unpolished (cap 6)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cost_support as cs
import lin_polish_support as lp
import lin_support as ls

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
CASES = lp.CASES
SET = dict(rho=ls.RHO, alpha=ls.ALPHA)
REL_TOL = 1e-9
RESIDUAL_MULT = 8.0         # (largest ratio 0.39, (20,5,2))
STEP_MULT = 24.0            # (candidate z and mu: largest ratio 11.72, (6,3,5) in strict mode)
STEP_NORM_MULT = 1094318.0  # (norm slots: largest ratio 547158.93, (6,3,2), slot 1 of one problem; see above)
DIRECT_MULT = 8.0           # (largest ratio 1.00)
STEP_TOLERANCE = 1     # accepted steps against the restatement's


def modes(ndlqr):
    return [0, ndlqr.FLAG_STRICT_FP]


def constrained_solver(ndlqr, cases, flags=0, mutate=None):
    probs = [c["p"] for c in cases]
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    C_, D_, lo, hi = ls.flat_rows(cases)
    arrays = list(cs.flat(probs))
    if mutate:
        mutate(arrays, D_)
    bs.initialize_flat_constrained(*arrays, C_, D_, lo, hi)
    return bs


def admm_state(bs, eps, max_iter=2000):
    """the device's own ADMM at `eps`: dict(iters, status, Z, v, y, mu)"""
    iters, status = bs.solve_constrained(eps_abs=eps, eps_rel=eps, max_iter=max_iter, **SET)
    red = bs.constraint_reduction()
    return dict(iters=iters, status=status, Z=bs.solutions(), v=red["v"], y=red["y"], mu=bs.constraint_multipliers())


def restate(c, st, i, dtype=np.float64, **kw):
    return lp.polish_reference(c["p"], c["C"], c["D"], c["lo"], c["hi"], st["Z"][i], st["v"][i], st["y"][i], ls.RHO,
                               forward_status=int(st["status"][i]), dtype=dtype, **kw)


def fields(z, n, m, N):
    return dict(zip(("lam", "x", "u"), cs.split(z, n, m, N)))


def worst_ratio(got, ref, own, label):
    """per field: the device's largest error against `ref` over the float64 restatement's own, among the fields whose error
    is above the floor of 16 eps of the field's largest entry (0: all below it); asserts nothing"""
    worst = 0.0
    for k in got:
        g, r, o = np.asarray(got[k], dtype=LD), np.asarray(ref[k], dtype=LD), np.asarray(own[k], dtype=LD)
        assert g.shape == r.shape and np.isfinite(np.asarray(g, dtype=np.float64)).all(), (label, k)
        if not r.size:
            continue
        floor = 16 * EPS * float(np.abs(r).max())
        err, mine = float(np.abs(g - r).max()), float(np.abs(o - r).max())
        if err > floor:
            worst = max(worst, err / mine if mine > 0 else np.inf)
    return worst


# ---------------------------------------------------------------------------- 1: the residual kernel alone
@functools.lru_cache(maxsize=None)
def residual_inputs(n, m, N):
    """two inputs per problem of the case: the restatement's ADMM iterate at 1e-3 with the codes read off it, and the
    restatement's polished point with its final codes; with the residuals of both restatements"""
    out = []
    for i, c in enumerate(ls.case(n, m, N)):
        a = lp.admm_start(n, m, N)[i]
        o = lp.polish_case(n, m, N, i)
        M = lp.bounded(c["lo"], c["hi"])
        first = lp.initial_codes(c["lo"], c["hi"], M, a["v"], a["y"])
        points = [(a["z"], np.where(first >= 2, a["mu"], 0.0), first), (np.asarray(o["z"], dtype=np.float64),
                                                                       np.asarray(o["mu"], dtype=np.float64), o["codes"])]
        res = []
        for z, mu, codes in points:
            per = {}
            for dtype in (np.float64, LD):
                rhs, norm, nc, _, r_c = lp.System(c["p"], c["C"], c["D"], c["lo"], c["hi"], dtype).residual(codes, o["sig"], z, mu)
                per[dtype] = dict(rc=r_c, norms=np.array([norm, nc]), **fields(rhs, n, m, N))
            res.append(dict(z=z, mu=mu, codes=codes, sig=o["sig"], f64=per[np.float64], ld=per[LD]))
        out.append(res)
    return out


def plant_nan(arrays, D_):
    """NaN in A, B, H, R, r, d of the caller's last knot and in its D: none of them is part of the problem"""
    A, B, Q, H, R, q, r, d, x0 = arrays
    for a in (A, B, H, R, r, d, D_):
        a[:, -1] = np.nan


@pytest.mark.parametrize("n,m,N", CASES)
def test_residual_kernel_per_entry(ndlqr, n, m, N):
    cases = ls.case(n, m, N)
    inputs = residual_inputs(n, m, N)
    worst = 0.0
    for point in (0, 1):
        ins = [inputs[i][point] for i in range(len(cases))]
        args = [np.stack([a[k] for a in ins]) for k in ("z", "mu", "codes")] + [np.array([a["sig"] for a in ins])]
        outs = {}
        for flags in modes(ndlqr):
            for planted in (False, True):
                bs = constrained_solver(ndlqr, cases, flags, plant_nan if planted else None)
                outs[(flags, planted)] = bs.constraint_polish_residual(*args, poison_pad=planted)
                bs.close()
        r, rc, norms = outs[(0, False)]
        # strict and default mode: the same bits; NaN in what is not part of the problem reaches no output
        for key, (r2, rc2, norms2) in outs.items():
            assert np.array_equal(r, r2) and np.array_equal(rc, rc2) and np.array_equal(norms, norms2), key
        for i in range(len(cases)):
            got = dict(rc=rc[i], norms=norms[:, i], **fields(r[i], n, m, N))
            ratio = worst_ratio(got, ins[i]["ld"], ins[i]["f64"], (n, m, N, i, point))
            worst = max(worst, ratio)
    print("residual kernel", (n, m, N), "largest error / restatement's own: %.2f" % worst)
    assert worst <= RESIDUAL_MULT, worst


# ---------------------------------------------------------------------------- 2: the first steps
def hip_polish(bs, sigma, max_steps, max_rounds):
    """ndlqr_hip_polish_constrained with the settings as they are (max_rounds = 0: no correction round)"""
    steps = np.zeros(bs.batch, dtype=np.int32)
    status = np.zeros(bs.batch, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    err = bs.L.ndlqr_hip_polish_constrained(bs.ctx, sigma, max_steps, max_rounds, ip(steps), ip(status))
    assert err == 0, bs.L.ndlqr_hip_last_error().decode()
    return steps, status


def first_step_ratio(ndlqr, n, m, N, flags):
    """(largest ratio over the candidate's fields lam, x, u, mu; over the norm slots)"""
    cases = ls.case(n, m, N)
    worst = [0.0, 0.0]
    for max_steps in (1, 2):
        bs = constrained_solver(ndlqr, cases, flags)
        st = admm_state(bs, lp.ADMM_EPS)
        hip_polish(bs, lp.DEFAULT_SIGMA, max_steps, 0)
        dev = bs.constraint_polish_state(max_steps)
        codes = bs.constraint_polish_codes()
        bs.close()
        for i, c in enumerate(cases):
            if st["status"][i] in (3, 4):
                continue
            tr = {np.float64: [], LD: []}
            ref = {dt: restate(c, st, i, dt, max_steps=max_steps, max_rounds=-1, trace=tr[dt]) for dt in tr}
            assert np.array_equal(codes[i], ref[np.float64]["codes"]) and dev["sig"][i] == ref[np.float64]["sig"]
            if len(tr[LD]) < max_steps or len(tr[np.float64]) < max_steps:
                continue  # (a restatement stopped before this step: nothing to compare the candidate with)
            pick = lambda dt: dict(mu=tr[dt][max_steps - 1]["mu"], norms=np.array(ref[dt]["norms"][0][: max_steps + 1]),
                                   **fields(tr[dt][max_steps - 1]["z"], n, m, N))
            got = dict(mu=dev["muc"][i], norms=dev["norms"][0, :, i], **fields(dev["zc"][i], n, m, N))
            ref, own = pick(LD), pick(np.float64)
            cut = lambda a, keys: {k: a[k] for k in keys}
            for j, keys in enumerate((("lam", "x", "u", "mu"), ("norms",))):
                worst[j] = max(worst[j], worst_ratio(cut(got, keys), cut(ref, keys), cut(own, keys), (n, m, N, i, max_steps)))
    return tuple(worst)


@pytest.mark.parametrize("n,m,N", CASES)
def test_first_steps_per_entry(ndlqr, n, m, N):
    ratios = {flags: first_step_ratio(ndlqr, n, m, N, flags) for flags in modes(ndlqr)}
    for flags, (cand, slots) in ratios.items():
        print("first steps", (n, m, N), "flags", flags, "largest error / restatement's own: candidate %.2f, norm slots %.2f" % (cand, slots))
    for flags, (cand, slots) in ratios.items():
        assert cand <= STEP_MULT, (flags, cand)
        assert slots <= STEP_NORM_MULT, (flags, slots)


# ---------------------------------------------------------------------------- 3: converged
def accepted_slot(row):
    """the slot of the last accepted iterate of a round from its norms (the rule of refine_accepted)"""
    s = 0
    while s + 1 < len(row) and row[s + 1] < row[s]:
        s += 1
    return s


def check_dynamics(c, z):
    p = c["p"]
    n, m, N = cs.dims(p)
    _, x, u = cs.split(z.astype(LD), n, m, N)
    dyn = [np.abs(x[0] - p["x0"]).max()]
    for k in range(N - 1):
        dyn.append(np.abs(x[k + 1] - (p["A"][k] @ x[k] + p["B"][k] @ u[k] + p["d"][k])).max())
    assert float(max(dyn)) <= REL_TOL * float(np.abs(x).max()), (float(max(dyn)), float(np.abs(x).max()))


_CONVERGED = {}


def converged(ndlqr, n, m, N, flags):
    """(unpolished problems, worst stationarity ratio, (device steps, restatement steps) per problem) of the case from the
    device's ADMM at 1e-3, everything of test 3 but the step counts asserted on the way; run once per (case, mode)"""
    key = (n, m, N, flags)
    if key in _CONVERGED:
        return _CONVERGED[key]
    cases = ls.case(n, m, N)
    bs = constrained_solver(ndlqr, cases, flags)
    st = admm_state(bs, lp.ADMM_EPS)
    count0 = bs.factor_count()
    steps, status = bs.polish_constrained()
    Z, mu, codes = bs.solutions(), bs.constraint_multipliers(), bs.constraint_polish_codes()
    dev = bs.constraint_polish_state()
    red = bs.constraint_reduction()
    assert bs.factor_count() - count0 == dev["rounds"]
    bs.close()
    refs = [restate(c, st, i) for i, c in enumerate(cases)]
    print("converged", (n, m, N), "flags", flags, "ADMM", list(st["iters"]), list(st["status"]), "| device steps", list(steps),
          "status", list(status), "rounds", dev["rounds"], "| restatement steps", [o["steps"] for o in refs], "status",
          [o["status"] for o in refs], "rounds", [o["rounds"] for o in refs])
    assert list(status) == [o["status"] for o in refs]
    pairs = [(int(steps[i]), o["steps"]) for i, o in enumerate(refs)]
    unpolished, worst = 0, 0.0
    for i, (c, o) in enumerate(zip(cases, refs)):
        if status[i] != 1:
            # left alone: solution, v, y and mu bit for bit what the constrained solve delivered
            unpolished += 1
            for a, b in ((Z[i], st["Z"][i]), (red["v"][i], st["v"][i]), (red["y"][i], st["y"][i]), (mu[i], st["mu"][i])):
                assert np.array_equal(a, b)
            continue
        p, C_, D_, lo, hi = c["p"], c["C"], c["D"], c["lo"], c["hi"]
        assert np.array_equal(codes[i], o["codes"])
        # the final |r_c| of the device where its last round's slots hold it, else the restatement's
        rc = float(o["rc"])
        if o["rounds"] == dev["rounds"]:
            rc = max(rc, float(dev["norms"][1, accepted_slot(dev["norms"][0, :, i]), i]))
        nrows = 2 * n + m + C_.shape[1] + 2
        big = max(1.0, max(float(np.abs(p[a]).max()) for a in ("A", "B", "Q", "H", "R")), float(np.abs(C_).max()),
                  float(np.abs(D_).max()))
        rounding = nrows * nrows * EPS * big * max(float(np.abs(Z[i]).max()), float(np.abs(mu[i]).max()), 1.0)
        got = ls.kkt_violation(p, C_, D_, lo, hi, Z[i], mu[i], rc + rounding)
        assert got["feasibility"] <= rc + rounding, (got, rc, rounding)
        assert got["complementarity"] == 0.0, got
        assert (mu[i][codes[i] == 3] >= 0).all() and (mu[i][codes[i] == 2] <= 0).all() and not mu[i][codes[i] < 2].any()
        check_dynamics(c, Z[i])
        # the warm start of the next solve is the polished point
        M = lp.bounded(lo, hi)
        w = ls.rows_of(p, C_, D_, Z[i])
        assert np.abs(red["v"][i][M] - np.clip(w, lo, hi)[M]).max() <= 4 * EPS * max(1.0, float(np.abs(w).max()))
        assert np.array_equal(red["y"][i][M], (mu[i] / ls.RHO)[M])
        direct = lp.active_direct(p, C_, D_, lo, hi, codes[i])
        if direct is None:
            continue  # (dependent active rows: no yardstick)
        ratio = got["stationarity"] / max(lp.stationarity_ld(p, C_, D_, *direct), np.finfo(float).tiny)
        worst = max(worst, ratio)
    print("   unpolished", unpolished, "| worst stationarity / that of the direct solve: %.2f" % worst)
    assert worst <= DIRECT_MULT, worst
    _CONVERGED[key] = (unpolished, worst, pairs)
    return _CONVERGED[key]


@pytest.mark.parametrize("n,m,N", CASES)
def test_converged_from_loose_admm(ndlqr, n, m, N):
    pairs = []
    for flags in modes(ndlqr):
        pairs += converged(ndlqr, n, m, N, flags)[2]
    # (last: everything else of the case has been checked by now)
    assert all(abs(dev - ref) <= STEP_TOLERANCE for dev, ref in pairs), pairs


def test_the_cap_on_unpolished_problems(ndlqr):
    total = sum(converged(ndlqr, n, m, N, 0)[0] for (n, m, N) in CASES)
    print("unpolished problems:", total, "of", 3 * len(CASES))
    assert total <= 3 * len(CASES) - lp.STATUS1_CAP


# ---------------------------------------------------------------------------- 4: rounds
@pytest.mark.parametrize("n,m,N", [(12, 4, 8), (7, 9, 16)])
def test_rounds_correct_a_wrong_first_set(ndlqr, n, m, N):
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        st = admm_state(bs, 1e-1)
        count0 = bs.factor_count()
        steps, status = bs.polish_constrained()
        codes, dev = bs.constraint_polish_codes(), bs.constraint_polish_state()
        moved = bs.factor_count() - count0
        bs.close()
        refs = [restate(c, st, i) for i, c in enumerate(cases)]
        want = max(o["rounds"] for o in refs)
        print("rounds", (n, m, N), "flags", flags, "device", dev["rounds"], list(status), "restatement", [o["rounds"] for o in refs],
              [o["status"] for o in refs])
        assert want >= 2  # (the case: a first set that is wrong)
        assert dev["rounds"] == want and moved == want
        assert list(status) == [o["status"] for o in refs]
        for i, o in enumerate(refs):
            assert np.array_equal(codes[i], o["codes"]), i


# ---------------------------------------------------------------------------- 5: state rules and refusals
def refused(bs, call, *needles):
    with pytest.raises(RuntimeError) as e:
        call()
    for needle in needles:
        assert needle in str(e.value), (needle, str(e.value))


def test_state_rules_and_refusals(ndlqr):
    n, m, N = 6, 3, 5
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        assert bs.solve() == 0
        plain = bs.solutions().copy()
        # refused without a constrained solve
        refused(bs, bs.polish_constrained, "ndlqr_hip_polish_constrained", "latest constrained solve")
        refused(bs, bs.constraint_polish_codes, "ndlqr_hip_download_constraint_polish_codes")
        st = admm_state(bs, lp.ADMM_EPS)
        # the box polish still refuses here, and points at this one
        refused(bs, bs.polish_box, "ndlqr_hip_polish_box", "ndlqr_PolishBatchLinConstrained")
        # refused after a new right-hand side
        q, r, d, x0 = cs.flat([c["p"] for c in cases], ("q", "r", "d", "x0"))
        bs.set_rhs_flat(q, r, d, x0)
        refused(bs, bs.polish_constrained, "ndlqr_hip_polish_constrained", "latest constrained solve")
        st = admm_state(bs, lp.ADMM_EPS)
        count0 = bs.factor_count()
        steps, status = bs.polish_constrained()
        rounds = bs.constraint_polish_state()["rounds"]
        assert (status == 1).all() and bs.factor_count() - count0 == rounds
        polished, mu = bs.solutions().copy(), bs.constraint_multipliers()
        # a polish is a new solution: a second one, the adjoint and the constraint gradients refuse, and say why
        refused(bs, bs.polish_constrained, "ndlqr_hip_polish_constrained", "latest constrained solve")
        refused(bs, lambda: bs.solve_constrained_adjoint(np.ones((3, bs.nvars))), "ndlqr_hip_solve_constrained_adjoint", "polished")
        refused(bs, bs.constraint_gradients, "ndlqr_hip_constraint_gradients", "polished")
        # a warm-started constrained solve reduces and factors once and converges at the polished point
        count1 = bs.factor_count()
        iters, status = bs.solve_constrained(eps_abs=lp.ADMM_EPS, eps_rel=lp.ADMM_EPS, max_iter=50, warm_start=True, **SET)
        assert bs.factor_count() - count1 == 1
        assert (status == 1).all() and (iters <= 2).all(), (iters, status)
        assert np.abs(bs.solutions() - polished).max() <= 1e-6 * np.abs(polished).max()
        # the adjoint works again
        bs.solve_constrained_adjoint(np.ones((3, bs.nvars)), eps_abs=1e-6, eps_rel=1e-6, max_iter=500)
        # a plain solve afterwards: the bits it gave before
        bs.polish_constrained()
        assert bs.solve() == 0
        assert np.array_equal(bs.solutions(), plain)
        refused(bs, bs.polish_constrained, "ndlqr_hip_polish_constrained", "latest constrained solve")
        bs.close()


def test_a_non_finite_and_a_certified_problem_are_left_alone(ndlqr):
    import lin_infeas_support as li
    # status 3: NaN in q of problem 1
    cases = ls.case(6, 3, 5)

    def poison(arrays, D_):
        arrays[5][1, 2, 0] = np.nan

    bs = constrained_solver(ndlqr, cases, 0, poison)
    st = admm_state(bs, lp.ADMM_EPS, max_iter=200)
    assert list(st["status"]) == [1, 3, 1]
    steps, status = bs.polish_constrained()
    assert list(status) == [1, 3, 1] and steps[1] == 0
    red = bs.constraint_reduction()
    for a, b in ((bs.solutions()[1], st["Z"][1]), (red["v"][1], st["v"][1]), (red["y"][1], st["y"][1])):
        assert np.array_equal(a, b, equal_nan=True)
    bs.close()
    # status 4: the infeasible member of lin_infeas_support.instance
    inst = li.instance(6, 3, 5, "A")
    bs = constrained_solver(ndlqr, inst, 0)
    bs.set_constraint_infeasibility(li.EVERY, li.EPS)
    iters, status = bs.solve_constrained(rho=li.RHO, alpha=li.ALPHA, eps_abs=li.EPS_ABS, eps_rel=li.EPS_REL, max_iter=li.MAX_ITER)
    assert list(status) == [1, 4, 1]
    red0, Z0, mu0 = bs.constraint_reduction(), bs.solutions().copy(), bs.constraint_multipliers()
    steps, status = bs.polish_constrained()
    assert status[1] == 2 and steps[1] == 0
    red = bs.constraint_reduction()
    assert np.array_equal(bs.solutions()[1], Z0[1]) and np.array_equal(red["v"][1], red0["v"][1])
    assert np.array_equal(red["y"][1], red0["y"][1]) and np.array_equal(bs.constraint_multipliers()[1], mu0[1])
    bs.close()
