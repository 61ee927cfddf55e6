"""The per-problem adaptive penalty of the solve with linear inequality constraints on the device
(ndlqr_BatchSetConstraintPenaltyAdaptation, ndlqr_CopyBatchConstraintPenalties) against
lin_adaptive_support.py: lin_support.admm with the rule of box_adaptive_support.penalty_step. Batch 3, the cases of
lin_support.case, rho = 1, alpha = 1.6, period 25 unless stated otherwise; default and strict mode.

What is exact and what is not. The DECISION is exact: rho+ is penalty_step of the device's own residual row (test 1). The
re-solve after a move adds no arithmetic to a re-solve, so it is held to the bar test_gpu_lin.py applies to one (test 2).
Whole trajectories are compared where the restatement's decisions were not within 1e-3 of going the other way
(lin_adaptive_support.margin: a condition on the inputs): there the final penalties and the number of factorisations are
the restatement's exactly and the iteration counts within the +-2 of section 3.17 (test 3)."""
import numpy as np
import pytest

import cost_support as cs
import lin_adaptive_support as las
import lin_grad_support as lg
import lin_support as ls
from box_adaptive_support import penalty_step
from test_gpu_lin import REL_TOL, SET, constrained_solver, fields, first_mult, modes, ratio_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
DECISION_CASES = [(6, 3, 5), (12, 4, 8), (7, 9, 16), (20, 5, 2), (12, 4, 5)]
CASES = [(n, m, N) for (n, m) in las.SHAPES for N in las.HORIZONS]


def adaptive_solver(ndlqr, cases, flags, every=las.EVERY, **kw):
    bs = constrained_solver(ndlqr, cases, flags, **kw)
    bs.set_constraint_adaptation(every)
    return bs


def runs_25_26(ndlqr, n, m, N, flags):
    """(the solver after max_iter = 25, a fresh one after max_iter = 26): with the period 25 the first does not move
    (it < max_iter fails), the second moves after iteration 25 and re-solves once"""
    cases = ls.case(n, m, N)
    a = adaptive_solver(ndlqr, cases, flags)
    it_a, st_a = a.solve_constrained(max_iter=25, **SET)
    assert np.array_equal(a.constraint_penalties(), np.ones(cs.BATCH))
    b = adaptive_solver(ndlqr, cases, flags)
    it_b, st_b = b.solve_constrained(max_iter=26, **SET)
    assert (st_a == 2).all() and (it_a == 25).all() and (it_b == 26).all(), (it_a, st_a, it_b, st_b)
    return a, b


# ---------------------------------------------------------------------------- 1: the decision, exactly
def test_the_decision_is_penalty_step_of_the_own_residuals(ndlqr):
    for flags in modes(ndlqr):
        moved = stayed = 0
        for n, m, N in DECISION_CASES:
            a, b = runs_25_26(ndlqr, n, m, N, flags)
            rows, got = a.constraint_residuals(), b.constraint_penalties()
            a.close(); b.close()
            want = np.array([penalty_step(1.0, *(float(x) for x in row)) for row in rows])
            print("decision", (n, m, N), "flags", flags, "device", list(got), "penalty_step of its rows", list(want))
            assert np.array_equal(got, want), (n, m, N, flags, got, want)
            moved += int((got != 1.0).sum())
            stayed += int((got == 1.0).sum())
        assert moved >= 3 and stayed >= 2, (moved, stayed)


# ---------------------------------------------------------------------------- 2: the iteration after a move
@pytest.mark.parametrize("n,m,N", DECISION_CASES[:4])
def test_the_resolve_after_a_move_per_entry(ndlqr, n, m, N):
    """z delivered after max_iter = 26 is the re-solve of iteration 26: the KKT system shifted by the device's rho+ with
    the right-hand side b - rho+ G'M(mu / rho+ - v), v and mu those of iteration 25. Per field and entry against the
    longdouble solve; bar: test_gpu_lin.first_mult x the float64 restatement's own error on that solve, at least 16 eps
    of the field's largest entry."""
    cases = ls.case(n, m, N)
    moved = 0
    for flags in modes(ndlqr):
        a, b = runs_25_26(ndlqr, n, m, N, flags)
        v, mu = a.constraint_reduction()["v"], a.constraint_multipliers()
        rho, Z = b.constraint_penalties(), b.solutions()
        a.close(); b.close()
        moved += int((rho != 1.0).sum())
        worst = 0.0
        for i, c in enumerate(cases):
            M = np.isfinite(c["lo"]) | np.isfinite(c["hi"])
            sol = {}
            for dtype in (LD, np.float64):
                K, rhs = ls.kkt_ld(ls.shifted_problem(c["p"], c["C"], c["D"], c["lo"], c["hi"], rho[i], dtype))
                r_ = dtype(rho[i])
                t = np.where(M, r_ * (mu[i].astype(dtype) / r_ - v[i].astype(dtype)), 0).astype(dtype)
                sol[dtype] = ls.Solver(K)(rhs - ls.perturbation(c["p"], c["C"], c["D"], t))
            ratio = ratio_of(fields(Z[i], n, m, N), fields(sol[LD], n, m, N), fields(sol[np.float64], n, m, N))
            print("re-solve after a move", (n, m, N), "flags", flags, "problem", i, "rho+ %g" % rho[i],
                  "largest error / restatement's own: %.2f" % ratio)
            worst = max(worst, ratio)
        assert worst <= first_mult(ndlqr, flags), (flags, worst)
    assert moved >= 2, moved


# ---------------------------------------------------------------------------- 3: trajectories
def check_converged(c, z, mu, res, rho):
    """test_gpu_lin.check_converged with the problem's own final penalty in the bar"""
    p = c["p"]
    n, m, N = cs.dims(p)
    bar = ls.kkt_bar(p, c["C"], c["D"], z, res, rho=rho)
    got = ls.kkt_violation(p, c["C"], c["D"], c["lo"], c["hi"], z, mu, bar["tol"])
    assert got["stationarity"] <= bar["stationarity"], (got, bar)
    assert got["feasibility"] <= bar["feasibility"], (got, bar)
    assert got["complementarity"] == 0.0, got
    _, x, u = cs.split(z.astype(LD), n, m, N)
    dyn = [np.abs(x[0] - p["x0"]).max()]
    for k in range(N - 1):
        dyn.append(np.abs(x[k + 1] - (p["A"][k] @ x[k] + p["B"][k] @ u[k] + p["d"][k])).max())
    assert float(max(dyn)) <= REL_TOL * float(np.abs(x).max()), max(dyn)


@pytest.mark.parametrize("n,m,N", CASES)
def test_trajectories(ndlqr, n, m, N):
    cases, ref = ls.case(n, m, N), las.case(n, m, N, 600)
    runs = [a["run"] for a in ref]
    decided = [a["decided"] for a in ref]
    for flags in modes(ndlqr):
        bs = adaptive_solver(ndlqr, cases, flags)
        fc = bs.factor_count()
        iters, status = bs.solve_constrained(max_iter=600, **SET)
        factored = bs.factor_count() - fc
        Z, mu, res, rho = bs.solutions(), bs.constraint_multipliers(), bs.constraint_residuals(), bs.constraint_penalties()
        bs.close()
        print("trajectory", (n, m, N), "flags", flags, "device", list(iters), list(status), list(rho), "factorisations", factored,
              "| restatement", [r["iters"] for r in runs], [r["status"] for r in runs], [r["rho"] for r in runs],
              1 + len(las.adapt_rounds(runs)), "margins", ["%.1e" % a["margin"] for a in ref])
        if all(decided):
            assert factored == 1 + len(las.adapt_rounds(runs)), (factored, las.adapt_rounds(runs))
        for i, (c, r) in enumerate(zip(cases, runs)):
            if not decided[i]:
                continue
            assert status[i] == r["status"], (i, status, r["status"])
            assert rho[i] == r["rho"], (i, rho, r["rho"])
            assert abs(int(iters[i]) - r["iters"]) <= 2, (i, iters, r["iters"])
            if r["status"] == 1:
                check_converged(c, Z[i], mu[i], res[i], rho[i])
            else:
                assert r["status"] == 2 and rho[i] == las.RHO_MAX  # (a seed that does not converge: at the clamp)
    # the cap on what the comparison above may leave out, over all 48 cases (shared, cached runs)
    undecided = [(n_, m_, N_, i) for n_, m_, N_ in CASES for i, a in enumerate(las.case(n_, m_, N_, 600)) if not a["decided"]]
    assert len(undecided) <= las.UNDECIDED_CAP, undecided


# ---------------------------------------------------------------------------- 4: frozen problems
@pytest.mark.parametrize("n,m,N", [(12, 4, 8), (20, 5, 8)])
def test_a_frozen_problem_never_moves(ndlqr, n, m, N):
    """Period 10, eps 0.03: in the restatement one problem converges within 8 iterations, another moves its penalty
    after iteration 10 and goes on. The batch is factored again then, and what the frozen problem delivers -- z, v, mu,
    iteration count, status -- is, bit for bit, what it delivers with adaptation off."""
    cases = ls.case(n, m, N)
    kw = dict(rho=ls.RHO, alpha=ls.ALPHA, eps_abs=0.03, eps_rel=0.03, max_iter=40)
    runs = [las.admm_adaptive(c["p"], c["C"], c["D"], c["lo"], c["hi"], every=10, eps_abs=0.03, eps_rel=0.03, max_iter=40)
            for c in cases]
    frozen = [i for i, r in enumerate(runs) if r["status"] == 1 and r["iters"] <= 8 and not r["moves"]]
    assert frozen and any(r["moves"] and r["moves"][0]["it"] == 10 for r in runs), [(r["iters"], r["rho"]) for r in runs]
    for flags in modes(ndlqr):
        out = []
        for every in (10, 0):
            bs = adaptive_solver(ndlqr, cases, flags, every=every)
            fc = bs.factor_count()
            iters, status = bs.solve_constrained(**kw)
            out.append(dict(iters=iters, status=status, Z=bs.solutions(), v=bs.constraint_reduction()["v"],
                            mu=bs.constraint_multipliers(), rho=bs.constraint_penalties(), factored=bs.factor_count() - fc))
            bs.close()
        on, off = out
        print("frozen", (n, m, N), "flags", flags, "adaptive", list(on["iters"]), list(on["rho"]), on["factored"], "fixed",
              list(off["iters"]), off["factored"])
        assert on["factored"] >= 2 and off["factored"] == 1 and (on["rho"] != 1.0).any()
        for i in frozen:
            assert on["status"][i] == off["status"][i] == 1 and on["iters"][i] == off["iters"][i] < 10 and on["rho"][i] == 1.0
            for k in ("Z", "v", "mu"):
                assert np.array_equal(on[k][i], off[k][i]), (i, k)


# ---------------------------------------------------------------------------- 5: state
def test_state(ndlqr):
    n, m, N = 6, 3, 5
    cases = ls.case(n, m, N)
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        assert bs.solve() == 0
        Z0 = bs.solutions()
        it_f, st_f = bs.solve_constrained(max_iter=600, **SET)
        Zf, muf = bs.solutions(), bs.constraint_multipliers()
        assert np.array_equal(bs.constraint_penalties(), np.ones(cs.BATCH))
        # an adaptive solve: a vector that is not uniform; a plain solve afterwards gives the plain bits
        bs.set_constraint_adaptation(las.EVERY)
        it_a, st_a = bs.solve_constrained(max_iter=600, **SET)
        rho_a = bs.constraint_penalties()
        assert (st_a == 1).all() and len(set(rho_a)) > 1, (st_a, rho_a)
        assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z0)
        # a new right-hand side and a warm start: the remembered vector and factorisation, whatever the settings' rho
        bs.solve_constrained(max_iter=600, **SET)
        fc = bs.factor_count()
        rng = np.random.default_rng(5)
        new = [dict(c["p"], q=c["p"]["q"] + 0.1 * rng.standard_normal((N, n)), x0=c["p"]["x0"] * 1.1) for c in cases]
        _, _, _, _, _, q, r, d, x0 = cs.flat(new)
        bs.set_rhs_flat(q, r, d, x0)
        bs.solve_constrained(max_iter=las.EVERY - 1, warm_start=True, **dict(SET, rho=7.0))
        assert bs.factor_count() == fc and np.array_equal(bs.constraint_penalties(), rho_a)
        # adaptation off after a vector that is not uniform: factored again, at the settings' rho
        bs.set_constraint_adaptation(0)
        _, _, _, _, _, q, r, d, x0 = cs.flat([c["p"] for c in cases])
        bs.set_rhs_flat(q, r, d, x0)
        it_g, st_g = bs.solve_constrained(max_iter=600, **SET)
        assert bs.factor_count() == fc + 1 and np.array_equal(bs.constraint_penalties(), np.ones(cs.BATCH))
        # ... and it is the fixed-penalty solve of this context, bit for bit
        assert np.array_equal(it_g, it_f) and np.array_equal(st_g, st_f)
        assert np.array_equal(bs.solutions(), Zf) and np.array_equal(bs.constraint_multipliers(), muf)
        # the setting is the solver's: another initialiser keeps it
        bs.set_constraint_adaptation(las.EVERY)
        bs.initialize_flat_dense(*cs.flat([c["p"] for c in cases]))
        C, D, lo, hi = ls.flat_rows(cases)
        bs.initialize_flat_constrained(*cs.flat([c["p"] for c in cases]), C, D, lo, hi)
        it_b, st_b = bs.solve_constrained(max_iter=600, **SET)
        assert np.array_equal(it_b, it_a) and np.array_equal(bs.constraint_penalties(), rho_a)
        bs.close()


# ---------------------------------------------------------------------------- 6: gradients
@pytest.mark.parametrize("n,m,N,every", [(6, 3, 5, 25), (12, 4, 8, 40)])
def test_gradients_after_an_adaptive_forward(ndlqr, n, m, N, every):
    """The adjoint and the constraint gradients after a forward that ended with different penalties in one batch, on the
    forward's own active set: w and nu against the direct solve of the active-set system (lin_grad_support.direct) to
    lin_grad_support.adjoint_bar with the problem's own rho; the constraint gradients recomputed from the device's z*,
    w, mu, nu and codes (lin_grad_support.constraint_grads), 2 eps (|mu w| + |nu z|) per entry in default mode, bit for
    bit in strict mode -- the bars of test_gpu_lin_gradients.py."""
    cases = ls.case(n, m, N)
    p = m + 2
    G = np.stack([lg.seeded_g(n, m, N, i) for i in range(cs.BATCH)])
    for flags in modes(ndlqr):
        strict = bool(flags & ndlqr.FLAG_STRICT_FP)
        bs = adaptive_solver(ndlqr, cases, flags, every=every)
        _, fstatus = bs.solve_constrained(max_iter=2000, **SET)
        rho = bs.constraint_penalties()
        assert (fstatus == 1).all() and len(set(rho)) > 1, (fstatus, rho)
        iters, status = bs.solve_constrained_adjoint(G, max_iter=2000, alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8)
        assert (status == 1).all(), (iters, status)
        Z, W, mu, nu = bs.solutions(), bs.adjoint(), bs.constraint_multipliers(), bs.constraint_adjoint_multipliers()
        codes, res, got = bs.constraint_codes(), bs.constraint_adjoint_residuals(), bs.constraint_gradients()
        assert np.array_equal(bs.constraint_penalties(), rho)  # (nothing of the adjoint moves it)
        bs.close()
        for i, c in enumerate(cases):
            w_direct, nu_direct = lg.direct(c["p"], c["C"], c["D"], codes[i], G[i])
            KK, _, _ = lg.bordered(c["p"], c["C"], c["D"], codes[i])
            e = dict(c, inv_norm=float(np.abs(np.linalg.inv(KK)).sum(axis=1).max()))
            bar = lg.adjoint_bar(e, W[i], res[i], rho=rho[i])
            err_w, err_nu = float(np.abs(W[i] - w_direct).max()), float(np.abs(nu[i] - nu_direct).max())
            print("adaptive gradients", (n, m, N), "flags", flags, "problem", i, "rho %g" % rho[i], "iterations", iters[i],
                  "|w - w_direct| %.3e |nu - nu_direct| %.3e (bar %.3e)" % (err_w, err_nu, bar["w"]))
            assert err_w <= bar["w"] and err_nu <= bar["w"], (err_w, err_nu, bar)
            act = codes[i] >= 2
            assert act.any()
            _, x, u = cs.split(Z[i], n, m, N)
            _, wx, wu = cs.split(W[i], n, m, N)
            ref = lg.constraint_grads(c["p"], codes[i], Z[i], W[i], mu[i], nu[i])
            mu_, nu_ = np.where(act, mu[i], 0.0), np.where(act, nu[i], 0.0)
            for name, width, wj, zj in (("C", n, wx, x), ("D", m, wu, u)):
                dev = got[name][i].reshape(N, width, p).swapaxes(-1, -2)
                size = np.abs(mu_[:, :, None] * wj[:, None, :]) + np.abs(nu_[:, :, None] * zj[:, None, :])
                if strict:
                    assert np.array_equal(dev, ref[name]), (name, float(np.abs(dev - ref[name]).max()))
                else:
                    assert (np.abs(dev - ref[name]) <= 2 * EPS * size).all(), (name, float(np.abs(dev - ref[name]).max()))
            assert np.array_equal(got["lo"][i], ref["lo"]) and np.array_equal(got["hi"][i], ref["hi"])


def test_torch_adaptive_against_dense_active_set_reference():
    _run_child("_case_adaptive")


def _run_child(name, *args):
    """test_gpu_lin_gradients._run_case for a case of this module: torch's HIP runtime has to be the first in its process"""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_lin_adaptive as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _case_adaptive(ndlqr):
    import torch
    import test_gpu_lin_gradients as T
    from rslqr_amd.autograd import _lin_cache, lqr_solve_constrained
    n, m, N, batch = 6, 3, 5, 3
    t = T._torch_case(n, m, N, "per_problem")
    gz = torch.tensor(np.stack([lg.seeded_g(n, m, N, i) for i in range(batch)]), dtype=torch.float64, device="cuda")
    args = [t[k] for k in T.NAMES13]
    z, got = T._grads13(lambda: lqr_solve_constrained(*args, adapt_every=las.EVERY, **T.KW), t, gz)
    (bs, _), = _lin_cache.values()
    rho = bs.constraint_penalties()
    print("final penalties", list(rho))
    assert len(set(rho)) > 1, rho
    zr, ref = T._grads13(lambda: T._dense_active_solve(t, z, n, m, N, batch), t, gz)
    assert T.rel(z.cpu().numpy(), zr.cpu().numpy()) <= 1e-8
    for k in T.NAMES13:
        assert got[k] is not None and got[k].shape == t[k].shape, k
        gr = ref[k] if ref[k] is not None else torch.zeros_like(got[k])
        err = T.rel(got[k].cpu().numpy(), gr.cpu().numpy())
        print(k, "relative error %.3e" % err)
        assert err <= 1e-6, (k, err)
    # adapt_every = 0 on the same cached solver switches it off again
    lqr_solve_constrained(*args, **T.KW)
    assert np.array_equal(bs.constraint_penalties(), np.ones(batch))


# ---------------------------------------------------------------------------- 7: refusals and arguments
def test_refusals_and_arguments(ndlqr):
    n, m, N = 6, 3, 5
    cases = ls.case(n, m, N)
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    bs.set_constraint_adaptation(5)  # (allowed in any mode)
    for kw in (dict(every=-1), dict(every=5, rho_min=-1.0), dict(every=5, rho_max=-1.0), dict(every=5, rho_min=2.0, rho_max=1.0),
               dict(every=5, rho_min=np.nan), dict(every=5, rho_max=np.inf)):
        with pytest.raises(RuntimeError, match="ndlqr_BatchSetConstraintPenaltyAdaptation failed"):
            bs.set_constraint_adaptation(**kw)
    with pytest.raises(RuntimeError, match="ndlqr_hip_download_constraint_penalties: the solver is not in constrained mode"):
        bs.constraint_penalties()
    bs.close()
    bs = adaptive_solver(ndlqr, cases, 0)
    with pytest.raises(RuntimeError, match="ndlqr_hip_download_constraint_penalties: no constrained solve yet"):
        bs.constraint_penalties()
    with pytest.raises(RuntimeError, match="ndlqr_hip_solve_constrained: the adaptive penalty .*ndlqr_BatchSetConstraintPenaltyAdaptation"):
        bs.solve_constrained(adapt_every=5, **SET)
    # the clamp is the caller's: a solve that may not leave [1, 1] is the fixed-penalty solve
    bs.set_constraint_adaptation(las.EVERY, rho_min=1.0, rho_max=1.0)
    iters, status = bs.solve_constrained(max_iter=600, **SET)
    assert np.array_equal(bs.constraint_penalties(), np.ones(cs.BATCH))
    assert (np.abs(iters - [c["ref"]["iters"] for c in cases]) <= 2).all() and (status == 1).all()
    bs.close()
