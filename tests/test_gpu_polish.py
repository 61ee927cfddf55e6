"""Active-set polish of the box-constrained batch solve (ndlqr_PolishBatchBoxConstrained) on the
device: strict mode against the numpy restatement of polish_support.py bit for bit, fast mode on every schedule against
the direct solution of the active-set system, the problems a polish must leave alone, and the state rules."""
import numpy as np
import pytest

import polish_support as ps
from box_grad_support import active_forward
from box_support import split

pytestmark = pytest.mark.gpu


def stack(probs, keys=ps.ARGS):
    return [np.stack([getattr(p, k) for p in probs]) for k in keys]


def setup(ndlqr, oracle, n, m, N, seeds, flags):
    """(solver with per-problem bounds set, problems, bounds per problem, rho)"""
    probs = [ps.synth(ndlqr, n, m, N, s) for s in seeds]
    bounds = [ps.boxes(oracle, p) for p in probs]
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat(*stack(probs))
    bs.set_bounds(*[np.stack([b[i] for b in bounds]) for i in range(4)])
    return bs, probs, bounds, float(np.mean([p.Q.mean() for p in probs]))


def strict_flags(ndlqr):
    return ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT


def mu_of(bs):
    mux, muu = bs.bound_multipliers()
    return np.concatenate([mux, muu], axis=2)


# ------------------------------------------------------------------------------------------------ 1. strict mode

STRICT_CASES = {"loose-admm": dict(shape=(4, 2, 16), seeds=ps.SWEEP_SEEDS, eps=1e-3, iters=4000, kw={}),
                "padded": dict(shape=(7, 9, 16), seeds=ps.SWEEP_SEEDS, eps=1e-3, iters=4000, kw={}),
                "rounds": dict(shape=ps.ROUNDS_CASE["shape"], seeds=ps.ROUNDS_CASE["seeds"], eps=1e-300,
                               iters=ps.ROUNDS_CASE["admm_iters"], kw=dict(max_rounds=ps.ROUNDS_CASE["max_rounds"])),
                "infeasible": dict(shape=ps.INFEASIBLE_CASE["shape"], seeds=ps.INFEASIBLE_CASE["seeds"], eps=1e-300,
                                   iters=ps.INFEASIBLE_CASE["admm_iters"],
                                   kw=dict(max_steps=1, max_rounds=ps.INFEASIBLE_CASE["max_rounds"]))}


@pytest.mark.parametrize("name", list(STRICT_CASES))
def test_strict_mode_is_the_numpy_restatement_bit_for_bit(ndlqr, oracle, name):
    case = STRICT_CASES[name]
    n, m, N = case["shape"]
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, case["seeds"], strict_flags(ndlqr))
    assert bs.solve() == 0
    plain = bs.solutions().copy()
    it, st = bs.solve_box(rho=rho, alpha=1.6, eps_abs=case["eps"], eps_rel=case["eps"], max_iter=case["iters"], check_every=1)
    f0 = bs.factor_count()
    steps, status = bs.polish_box(**case["kw"])
    sol, mu, codes = bs.solutions(), mu_of(bs), bs.polish_codes()
    solve = ps.oracle_solve(oracle)
    rounds = []
    for p, prob in enumerate(probs):
        z, v, y, rit, rst = ps.admm_state(prob, solve, bounds[p], rho, 1.6, case["eps"], case["iters"])
        assert rit == it[p] and rst == st[p]
        o = ps.polish_reference(prob, solve, bounds[p], z, v, y, rho, **case["kw"])
        rounds.append(o["rounds"])
        print(name, p, "status", o["status"], "steps", o["steps"], "rounds", o["rounds"])
        assert status[p] == o["status"] and steps[p] == o["steps"], (p, status, steps, o["status"], o["steps"])
        assert np.array_equal(codes[p], o["codes"]), p
        assert np.array_equal(sol[p], o["z"]), p
        assert np.array_equal(mu[p], o["mu"]), p
    assert bs.factor_count() - f0 == max(rounds)
    # v, y as the restatement leaves them (polished for status 1, ADMM's bit for bit otherwise): one warm-started
    # iteration from the device's v, y equals the numpy iteration from the restatement's
    bs.solve_box(rho=rho, alpha=1.6, eps_abs=1e-300, eps_rel=1e-300, max_iter=1, warm_start=True)
    warm, warm_mu = bs.solutions(), mu_of(bs)
    for p, prob in enumerate(probs):
        z, v, y, _, _ = ps.admm_state(prob, solve, bounds[p], rho, 1.6, case["eps"], case["iters"])
        o = ps.polish_reference(prob, solve, bounds[p], z, v, y, rho, **case["kw"])
        zw, muw = ps.admm_step_from(prob, solve, bounds[p], rho, 1.6, o["v"], o["y"])
        assert np.array_equal(warm[p], zw) and np.array_equal(warm_mu[p], muw), p
    # the resident inputs are as they were: the plain solve is the one from before
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), plain)
    bs.close()


# ------------------------------------------------------------------------------------------------ 2. fast mode, every schedule

# (n, m, N, batch, flags, NDLQR_TREE, schedule of the constrained solve or None): compact records, tree, runtime-sized
# records, knot-lean, generic-keep beyond 128 states, strict, a padded shape, a short horizon
SCHEDULE_CASES = [(12, 4, 64, 3, "records", "0", "reduced-compact-records"),
                  (6, 3, 64, 3, "records", None, "reduced-tree"),
                  (16, 4, 32, 2, "none", None, None),
                  (2, 1, 64, 3, "records", None, "knot-lean"),
                  (144, 16, 8, 1, "records", None, "generic-keep"),
                  (12, 4, 16, 2, "strict", None, "knot-strict"),
                  (7, 9, 16, 2, "records", "0", "reduced-compact-records"),
                  (6, 3, 4, 2, "records", None, "generic-reduced-records")]


def polished(ndlqr, oracle, n, m, N, seeds, flags):
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, seeds, flags)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
    admm = (bs.solutions().copy(), mu_of(bs))
    steps, status = bs.polish_box()
    return bs, probs, bounds, rho, admm, steps, status


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6] or c[4], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
def test_every_schedule_reaches_the_active_set_solution(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "none": 0, "strict": strict_flags(ndlqr)}[flags]
    seeds = [1700 + p for p in range(batch)]
    bs, probs, bounds, rho, admm, steps, status = polished(ndlqr, oracle, n, m, N, seeds, fl)
    assert want is None or bs.schedule() == want, bs.schedule()
    sol, mu, codes = bs.solutions(), mu_of(bs), bs.polish_codes()
    print("steps", steps.tolist(), "status", status.tolist())
    assert (status == 1).all(), status  # (every recorded run polishes every problem of these cases)
    for p, prob in enumerate(probs):
        if status[p] != 1:
            assert np.array_equal(sol[p], admm[0][p]) and np.array_equal(mu[p], admm[1][p]), p
            continue
        zt, mt = active_forward(prob, codes[p].astype(np.int8), *bounds[p])
        got, ref, was = (ps.stationarity(prob, *a, bounds[p]) for a in ((sol[p], mu[p]), (zt, mt), (admm[0][p], admm[1][p])))
        print("problem %d: stationarity %.3e, of the direct solve %.3e (ratio %.2f), of ADMM %.3e"
              % (p, got["stationarity"], ref["stationarity"], got["stationarity"] / ref["stationarity"], was["stationarity"]))
        assert got["bounds"] == 0 and got["complementarity"] == 0, got
        assert got["stationarity"] <= 4 * ref["stationarity"]
        assert got["stationarity"] <= 1e-3 * was["stationarity"]
        x, u = split(sol[p], n, m, N)[1:]
        xu = np.concatenate([x, np.concatenate([u, np.zeros((1, m))])], axis=1)
        lo = np.concatenate([bounds[p][0], bounds[p][2]], axis=1)
        hi = np.concatenate([bounds[p][1], bounds[p][3]], axis=1)
        assert np.array_equal(xu[codes[p] == 3], hi[codes[p] == 3]) and np.array_equal(xu[codes[p] == 2], lo[codes[p] == 2])
    bs.close()
    if flags != "strict":  # the statuses are those of the strict run on the same inputs
        sb, _, _, _, _, _, strict_status = polished(ndlqr, oracle, n, m, N, seeds, strict_flags(ndlqr))
        sb.close()
        assert np.array_equal(status, strict_status), (status, strict_status)


# ------------------------------------------------------------------------------------------------ 3. left alone

def test_unpolished_and_non_finite_problems_keep_their_bits(ndlqr, oracle):
    case = ps.INFEASIBLE_CASE
    n, m, N = case["shape"]
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, case["seeds"], ndlqr.FLAG_KEEP_RECORDS)
    bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=case["admm_iters"])
    sol, mu = bs.solutions().copy(), mu_of(bs)
    steps, status = bs.polish_box(max_steps=1, max_rounds=case["max_rounds"])
    assert (status == 2).all(), status
    assert np.array_equal(bs.solutions(), sol) and np.array_equal(mu_of(bs), mu)
    bs.close()
    # a NaN in the data of one problem: its constrained solve ends as 3, and so does its polish
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, (1, 2, 3), ndlqr.FLAG_KEEP_RECORDS)
    x0 = np.stack([p.x0 for p in probs])
    x0[2, 1] = np.nan
    bs.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000, check_every=1)
    assert st[2] == 3 and (st[:2] == 1).all(), st
    sol, mu = bs.solutions().copy(), mu_of(bs)
    steps, status = bs.polish_box()
    assert status[2] == 3 and steps[2] == 0 and (status[:2] == 1).all(), (steps, status)
    assert np.array_equal(bs.solutions()[2], sol[2], equal_nan=True) and np.array_equal(mu_of(bs)[2], mu[2], equal_nan=True)
    bs.close()


# ------------------------------------------------------------------------------------------------ 4. state rules

def test_state_rules(ndlqr, oracle):
    n, m, N, seeds = 12, 4, 16, (1, 2, 3)
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, seeds, ndlqr.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    plain = bs.solutions().copy()
    with pytest.raises(RuntimeError, match="latest constrained solve"):  # nothing to polish after a plain solve
        bs.polish_box()
    settings = dict(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
    bs.solve_box(**settings)
    f0 = bs.factor_count()
    status_dev = ndlqr.DeviceArray((len(seeds),))  # (device memory for status; steps on the host)
    steps, _ = bs.polish_box(status=status_dev)
    status = status_dev.get().view(np.int32)[: len(seeds)]
    assert (status == 1).all() and (steps >= 1).all(), (steps, status)
    rounds = bs.factor_count() - f0
    assert 1 <= rounds <= 4
    assert bs.solve_ms() > 0.0
    sol, mu = bs.solutions().copy(), mu_of(bs)
    # the ADMM factorisation is gone: its adjoint refuses and names the polished one; so do the plain re-solves and a
    # second polish
    with pytest.raises(RuntimeError, match="polished adjoint"):
        bs.solve_box_adjoint(np.ones((len(seeds), bs.nvars)))
    assert bs.solve_rhs_only() != 0
    assert bs.solve_adjoint(np.ones((len(seeds), bs.nvars))) != 0
    with pytest.raises(RuntimeError, match="latest constrained solve"):
        bs.polish_box()
    assert np.array_equal(bs.solutions(), sol)
    # a warm-started ADMM with the same settings starts at the polished point: one factorisation, at most 2 iterations
    it, st = bs.solve_box(warm_start=True, **settings)
    assert bs.factor_count() == f0 + rounds + 1
    assert (it <= 2).all() and (st == 1).all(), (it, st)
    # new bounds after a constrained solve: its polish refuses
    bs.set_bounds(*[np.stack([b[i] for b in bounds]) for i in range(4)])
    with pytest.raises(RuntimeError, match="latest constrained solve"):
        bs.polish_box()
    # a plain solve afterwards is the one from before
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), plain)
    assert bs.solve_rhs_only() == 0
    # shared bounds equal the same bounds per problem, bit for bit
    shared = bounds[0]
    out = []
    for per_problem in (False, True):
        bs.set_bounds(*[np.broadcast_to(a, (len(seeds),) + a.shape).copy() if per_problem else a for a in shared])
        bs.solve_box(**settings)
        steps, status = bs.polish_box()
        out.append((steps, status, bs.solutions().copy(), mu_of(bs), bs.polish_codes()))
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert (out[0][1] == 1).any()
    bs.close()


def test_a_non_positive_pivot_restores_the_inputs_and_names_the_polish(ndlqr, oracle):
    """R < 0 on an input entry whose bounds are far away: bounded, so ADMM's shift by rho covers it; never active, so the
    polish's shift does not"""
    n, m, N, k, i = 4, 2, 16, 3, 0
    probs = [ps.synth(ndlqr, n, m, N, s) for s in (1, 2)]
    bounds = [[a.copy() for a in ps.boxes(oracle, p)] for p in probs]
    rho = float(np.mean([p.Q.mean() for p in probs]))
    bounds[1][2][k, i], bounds[1][3][k, i] = -1e6, 1e6
    probs[1].R[k, i] = -0.25 * rho
    bs = ndlqr.BatchSolver(n, m, N, 2, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    bs.set_bounds(*[np.stack([b[j] for b in bounds]) for j in range(4)])
    settings = dict(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=200)
    it, st = bs.solve_box(**settings)  # (R + rho > 0: ADMM factors; whether it converges does not matter here)
    sol = bs.solutions().copy()
    f0 = bs.factor_count()
    assert bs.L.ndlqr_PolishBatchBoxConstrained(bs.h, None, None, None) == ndlqr.api.ERR_NOT_SPD
    msg = bs.L.ndlqr_hip_last_error().decode()
    assert "ndlqr_hip_polish_box" in msg and "sigma" in msg, msg
    assert bs.factor_count() == f0 + 1
    with pytest.raises(RuntimeError):  # no resident solution, nothing remembered
        bs.solutions()
    with pytest.raises(RuntimeError):
        bs.solve_polished_adjoint(np.ones((2, bs.nvars)))
    # Q, R restored on the error exit: the constrained solve is the one from before, bit for bit
    it2, st2 = bs.solve_box(**settings)
    assert np.array_equal(it, it2) and np.array_equal(st, st2)
    assert np.array_equal(bs.solutions(), sol, equal_nan=True)
    bs.close()


# ------------------------------------------------------------------------------------------------ 5. polished adjoint

BOUNDS = ("xlo", "xhi", "ulo", "uhi")


def nu_of(bg, p):
    return np.concatenate([bg["xlo"][p] + bg["xhi"][p], bg["ulo"][p] + bg["uhi"][p]], axis=1)


@pytest.mark.parametrize("name", ["loose-admm", "padded", "rounds"])
def test_strict_polished_adjoint_is_the_numpy_restatement_bit_for_bit(ndlqr, oracle, name):
    from box_grad_support import bound_grads
    from test_gpu_gradients import ARGS, grad_formula
    case = STRICT_CASES[name]
    n, m, N = case["shape"]
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, case["seeds"], strict_flags(ndlqr))
    bs.solve_box(rho=rho, alpha=1.6, eps_abs=case["eps"], eps_rel=case["eps"], max_iter=case["iters"], check_every=1)
    _, status = bs.polish_box(**case["kw"])
    sol, mu, codes = bs.solutions().copy(), mu_of(bs), bs.polish_codes()
    g = np.random.default_rng(11).standard_normal((len(probs), bs.nvars))
    f0 = bs.factor_count()
    asteps, astatus = bs.solve_polished_adjoint(g)
    assert bs.factor_count() == f0
    w, grads, bg = bs.adjoint(), bs.gradients(), bs.bound_gradients()
    solve = ps.oracle_solve(oracle)
    for p, prob in enumerate(probs):
        sig = ps.sigma_of(prob, ps.DEFAULT_SIGMA)
        wr, nur, rsteps, rstatus = ps.polished_adjoint_reference(prob, solve, codes[p].astype(np.int8), sig, g[p],
                                                                 polish_status=int(status[p]))
        print(name, p, "polish status", status[p], "adjoint steps", rsteps, "status", rstatus)
        assert asteps[p] == rsteps and astatus[p] == rstatus, (p, asteps, astatus, rsteps, rstatus)
        assert np.array_equal(w[p], wr), p
        ref = grad_formula(prob, sol[p], wr)
        for k in ARGS:
            assert np.array_equal(grads[k][p], ref[k]), (p, k)
        bref = bound_grads(codes[p].astype(np.int8), nur, n)
        for k in BOUNDS:
            assert np.array_equal(bg[k][p], bref[k]), (p, k)
    # nothing of the polish changed
    assert np.array_equal(bs.solutions(), sol) and np.array_equal(mu_of(bs), mu)
    bs.close()


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6] or c[4], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
def test_every_schedule_against_the_active_set_adjoint(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want):
    from box_grad_support import active_adjoint, bound_grads, kkt_sparse
    from support import kkt_residual_ld
    from test_gpu_gradients import ARGS, grad_formula
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "none": 0, "strict": strict_flags(ndlqr)}[flags]
    bs, probs, bounds, rho, admm, steps, status = polished(ndlqr, oracle, n, m, N, [1700 + p for p in range(batch)], fl)
    assert (status == 1).all(), status
    sol, codes = bs.solutions().copy(), bs.polish_codes()
    g_host = np.random.default_rng(n + N).standard_normal((batch, bs.nvars))
    g = ndlqr.DeviceArray((batch, bs.nvars)).set(g_host)  # (device memory for g)
    asteps, astatus = bs.solve_polished_adjoint(g)
    print("adjoint steps", asteps.tolist())
    assert (astatus == 1).all(), astatus
    w, grads, bg = bs.adjoint(), bs.gradients(), bs.bound_gradients()
    summed = [bs.bound_gradients(summed=True) for _ in range(2)]
    for k in BOUNDS:  # two summed calls bit-identical, and the sum of the per-problem ones to rounding
        assert np.array_equal(summed[0][k], summed[1][k]), k
        assert np.abs(summed[0][k] - bg[k].sum(axis=0)).max() <= 1e-12 * max(1.0, np.abs(bg[k]).max()), k
    for p, prob in enumerate(probs):
        cd = codes[p].astype(np.int8)
        wr, nur = active_adjoint(prob, cd, g_host[p])
        nu = nu_of(bg, p)
        # the bar of the forward applied to the adjoint's stationarity g - K w - E' nu, in extended precision: at most 4 x
        # that of the direct solve of the same system (both fp64-rounded solutions of it)
        def stat(wv, nv):
            from box_grad_support import adjoint_problem
            from support import Problem
            ap = adjoint_problem(prob, g_host[p])
            ap = Problem(n, m, N, ap.A, ap.B, ap.Q, ap.R, ap.q + nv[:, :n], ap.r + nv[:, n:], ap.d, ap.x0)
            r = kkt_residual_ld(ap, wv)
            return float(max(np.abs(r[0]).max(), np.abs(r[1]).max(), np.abs(r[2][: N - 1]).max()))
        got, ref = stat(w[p], nu), stat(wr, nur)
        print("problem %d: adjoint stationarity %.3e, of the direct solve %.3e (ratio %.2f)" % (p, got, ref, got / ref))
        assert got <= 4 * ref
        assert (ps.entries_of(prob, w[p])[cd >= 2] == 0).all()
        bref = bound_grads(cd, nur, n)
        for k in BOUNDS:
            assert np.array_equal(bg[k][p] != 0, bref[k] != 0), (p, k)
        ref12 = grad_formula(prob, sol[p], wr)
        for k in ARGS:  # (the tolerance test_gpu_box_gradients holds the box adjoint's gradients to)
            err = np.linalg.norm(grads[k][p] - ref12[k]) / max(np.linalg.norm(ref12[k]), 1e-300)
            assert err <= 1e-6, (p, k, err)
    bs.close()


def test_adjoint_state_rules(ndlqr, oracle):
    n, m, N, seeds = 4, 2, 16, ps.INFEASIBLE_CASE["seeds"] + (1,)
    bs, probs, bounds, rho = setup(ndlqr, oracle, n, m, N, seeds, ndlqr.FLAG_KEEP_RECORDS)
    g = np.ones((len(seeds), bs.nvars))
    bs.solve_box(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
    with pytest.raises(RuntimeError, match="latest polish"):  # no polish yet
        bs.solve_polished_adjoint(g)
    _, status = bs.polish_box()
    assert (status == 1).all()
    bs.solve_polished_adjoint(g)
    w = bs.adjoint().copy()
    bs.solve_polished_adjoint(g)  # (repeatable: the record columns were restored)
    assert np.array_equal(bs.adjoint(), w)
    # new bounds: the polished adjoint refuses
    bs.set_bounds(*[np.stack([b[i] for b in bounds]) for i in range(4)])
    with pytest.raises(RuntimeError, match="latest polish"):
        bs.solve_polished_adjoint(g)
    # problems that were not polished report the polish status and get zeros
    bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=1)
    _, status = bs.polish_box(max_steps=1, max_rounds=1)
    assert (status[:2] == 2).all(), status
    asteps, astatus = bs.solve_polished_adjoint(g)
    assert np.array_equal(astatus[:2], status[:2]) and (asteps[:2] == 0).all()
    assert not bs.adjoint()[:2].any()
    bg = bs.bound_gradients()
    assert not any(bg[k][:2].any() for k in BOUNDS)
    bs.close()


# ------------------------------------------------------------------------------------------------ 6. torch
# Each case runs in a fresh process that initialises torch's device first (as test_gpu_box_gradients._run_case).

def _run_case(name):
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_polish as T\n"
            "T.%s(rslqr_amd)\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_torch_polish_agrees_with_the_admm_path():
    _run_case("_case_torch_polish")


def test_torch_polish_raises_when_a_problem_is_not_polished():
    _run_case("_case_torch_raises")


def _case_torch_polish(ndlqr):
    """forward values and all twelve gradients of polish=True (ADMM at 1e-3) against polish=False run to 1e-10, within
    the tolerances test_gpu_box_gradients holds that path to against its dense reference (1e-8 forward, 1e-6 gradients)"""
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    from test_gpu_box_gradients import _grads12, _torch_bounds, _torch_problem, rel
    from test_gpu_gradients import ARGS
    n, m, N, batch = 6, 3, 16, 3
    t = _torch_problem(ndlqr, n, m, N, batch, 2000)
    bnd = _torch_bounds(t, n, m, N, batch, "mixed")
    leaves = dict(t, **bnd)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    args = [t[k] for k in ARGS] + [bnd[k] for k in BOUNDS]
    zr, ref = _grads12(lambda: lqr_solve_box(*args, rho=1.0, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000), leaves, gz)
    z, got = _grads12(lambda: lqr_solve_box(*args, rho=1.0, eps_abs=1e-3, eps_rel=1e-3, max_iter=20000, polish=True), leaves, gz)
    assert rel(z.cpu().numpy(), zr.cpu().numpy()) <= 1e-8
    for k in tuple(ARGS) + BOUNDS:
        assert got[k].shape == ref[k].shape, k
        assert rel(got[k].cpu().numpy(), ref[k].cpu().numpy()) <= 1e-6, (k, rel(got[k].cpu().numpy(), ref[k].cpu().numpy()))


def _case_torch_raises(ndlqr):
    """the raise on a polish status that is not 1 (the status comes from a stand-in: ADMM that converges onto a set the
    polish cannot correct is not constructible at will)"""
    import torch
    from unittest import mock
    from rslqr_amd.autograd import lqr_solve_box
    from test_gpu_box_gradients import _torch_bounds, _torch_problem
    from test_gpu_gradients import ARGS
    n, m, N, batch = 3, 2, 8, 2
    t = {k: v.detach() for k, v in _torch_problem(ndlqr, n, m, N, batch, 2400).items()}
    bnd = {k: v.detach() for k, v in _torch_bounds(t, n, m, N, batch, "per_problem").items()}
    args = [t[k] for k in ARGS]
    z = lqr_solve_box(*args, ulo=bnd["ulo"], uhi=bnd["uhi"], rho=1.0, eps_abs=1e-3, eps_rel=1e-3, polish=True)
    assert torch.isfinite(z).all()
    not_polished = lambda self, *a, **k: (np.zeros(batch, dtype=np.int32), np.array([1, 2], dtype=np.int32))
    with mock.patch.object(ndlqr.BatchSolver, "polish_box", not_polished):
        with pytest.raises(RuntimeError, match="not polished"):
            lqr_solve_box(*args, ulo=bnd["ulo"], uhi=bnd["uhi"], rho=1.0, eps_abs=1e-3, eps_rel=1e-3, polish=True)
