"""Per-problem adaptive penalty of the box-constrained batch solve (NdLqrBoxSettings.adapt_every,
ndlqr_CopyBatchBoxPenalties) on the device: strict mode against the numpy restatement of the rule
driving the oracle (bit for bit), fast mode from rho = mean diag R against the references of box_support.py on several
shapes and on every schedule, iteration totals and factorisation counts against the fixed penalty, the state rules, and
the gradients behind an adaptive forward."""
import numpy as np
import pytest

from box_adaptive_support import admm_adaptive_reference
from box_grad_support import active_adjoint, adjoint_admm_reference, bound_grads
from box_support import bvls_inputs, split
from support import Problem
from test_gpu_box import (SCHEDULE_CASES, assert_state_bounds_active, check_certificate, input_box, rel, solver, stack,
                          state_box, synth)
from test_gpu_box_gradients import adjoint_residual, codes_of
from test_gpu_gradients import ARGS, grad_formula

pytestmark = pytest.mark.gpu

BOUNDS = ("xlo", "xhi", "ulo", "uhi")
ADAPT = 25  # the library has no default period: 0 is the fixed penalty; 25 is what DESIGN.md section 3.11 measures


def mean_r(probs):
    return float(np.mean([p.R.mean() for p in probs]))


def adaptive_input_bounded_states(bs, ulo, uhi, rho):
    """x [batch, N, n] of the solution with the input bounds alone (eps 1e-10), by the adaptive solve"""
    bs.set_bounds(None, None, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, check_every=25, adapt_every=ADAPT)
    assert (st == 1).all(), (it, st)
    return np.stack([split(z, bs.n, bs.m, bs.N)[1] for z in bs.solutions()])


# ------------------------------------------------------------------------------------------------ a. strict, bit for bit

STRICT = dict(n=12, m=4, N=16, batch=4, seed=110, rho=0.37, alpha=1.6, eps=1e-2, adapt_every=3, max_iter=13)


def strict_case(ndlqr, oracle):
    """The strict case and its reference (chosen on the CPU): some problem changes its penalty after another one was
    frozen, so the refactorisation has to reproduce the frozen problem's z. Returns (probs, bounds, reference results)."""
    c = STRICT
    n, m, N, batch = c["n"], c["m"], c["N"], c["batch"]
    probs = [synth(ndlqr, n, m, N, c["seed"] + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 1.0)
    frac = np.array([0.5, 3.0, 0.5, 1.5])[:, None, None]
    ulo, uhi = ulo * frac, uhi * frac
    xlo, xhi = state_box(oracle, probs, 0.7)
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    run = lambda p, max_iter: admm_adaptive_reference(probs[p], solve, xlo[p], xhi[p], ulo[p], uhi[p], c["rho"], c["alpha"],
                                                      c["eps"], c["eps"], max_iter, c["adapt_every"])
    ref = [run(p, c["max_iter"]) for p in range(batch)]
    changed = [p for p in range(batch) if ref[p][8] > 0]
    frozen = [p for p in range(batch) if ref[p][6] == 1 and ref[p][8] == 0 and ref[p][5] < c["max_iter"]]
    assert changed and frozen, [(r[5], r[6], r[8]) for r in ref]
    first = min(ref[p][5] for p in frozen)
    # (a run cut at first + 1 iterations adapts at the iterations <= first only)
    assert any(ref[p][8] > run(p, first + 1)[8] for p in changed), "no penalty changes after a problem was frozen"
    return probs, (xlo, xhi, ulo, uhi), ref


def test_strict_mode_is_the_numpy_restatement_bit_for_bit(ndlqr, oracle):
    c = STRICT
    n, m, N, batch = c["n"], c["m"], c["N"], c["batch"]
    probs, (xlo, xhi, ulo, uhi), ref = strict_case(ndlqr, oracle)
    bs = solver(ndlqr, probs, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    bs.set_bounds(xlo, xhi, ulo, uhi)
    f0 = bs.factor_count()
    it, st = bs.solve_box(rho=c["rho"], alpha=c["alpha"], eps_abs=c["eps"], eps_rel=c["eps"], max_iter=c["max_iter"],
                          adapt_every=c["adapt_every"])
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    pen = bs.box_penalties()
    print("iterations", it.tolist(), "status", st.tolist(), "penalties", pen.tolist(), "factorisations", bs.factor_count() - f0)
    for p in range(batch):
        x, u, rx, ru, lam, rit, rst, rrho, _ = ref[p]
        assert it[p] == rit and st[p] == rst, (p, it[p], rit, st[p], rst)
        assert pen[p] == rrho, (p, pen[p], rrho)
        lg, xg, ug = split(sol[p], n, m, N)
        assert np.array_equal(xg, x) and np.array_equal(ug, u[: N - 1]) and np.array_equal(lg, lam), p
        assert np.array_equal(mux[p], rx) and np.array_equal(muu[p], ru), p
    assert 1 < bs.factor_count() - f0 <= 1 + int(it.max()) // c["adapt_every"]
    # f. the gradients behind it, bit for bit: the adjoint iteration with every problem's own final penalty
    g = np.random.default_rng(7).standard_normal((batch, bs.nvars))
    sol = sol.copy()
    ait, ast = bs.solve_box_adjoint(g, alpha=c["alpha"], eps_abs=1e-300, eps_rel=1e-300, max_iter=5)
    w, grads, bg = bs.adjoint(), bs.gradients(), bs.bound_gradients()
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    for p, prob in enumerate(probs):
        codes = codes_of(bs, sol, p, xlo, xhi, ulo, uhi)
        wr, nur, rit, rst = adjoint_admm_reference(prob, solve, codes, g[p], float(pen[p]), c["alpha"], 1e-300, 1e-300, 5)
        assert ait[p] == rit and ast[p] == rst, (p, ait[p], rit, ast[p], rst)
        assert np.array_equal(w[p], wr), p
        gref = grad_formula(prob, sol[p], wr)
        for k in ARGS:
            assert np.array_equal(grads[k][p], gref[k]), (p, k)
        bref = bound_grads(codes, nur, n)
        for k in BOUNDS:
            assert np.array_equal(bg[k][p], bref[k]), (p, k)
    bs.close()


# ------------------------------------------------------------------------------------------------ b, c. fast mode across shapes

@pytest.mark.parametrize("states", [False, True], ids=["inputs", "states+inputs"])
@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 8), (6, 3, 32, 4), (7, 9, 16, 2), (16, 4, 32, 2)])
def test_fast_mode_from_mean_diag_r(ndlqr, oracle, n, m, N, batch, states):
    """From rho = mean diag R -- the scale the fixed-penalty tests avoid for state bounds -- every problem converges within
    the max_iter of those tests and meets their references, in fewer iterations in total than the fixed penalty, with
    at most one factorisation per adapt iteration."""
    probs = [synth(ndlqr, n, m, N, 40 + p) for p in range(batch)]
    rho = mean_r(probs)
    bs = solver(ndlqr, probs)
    inf = np.full((batch, N, n), np.inf)
    if states:
        ulo, uhi = input_box(oracle, probs, 0.6)
        xlo, xhi = state_box(oracle, probs, 0.7, adaptive_input_bounded_states(bs, ulo, uhi, rho))
        bs.set_bounds(xlo, xhi, ulo, uhi)
    else:
        ulo, uhi = input_box(oracle, probs, 0.5)
        xlo, xhi = -inf, inf
        bs.set_bounds(None, None, ulo, uhi)
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    f0 = bs.factor_count()
    it, st = bs.solve_box(adapt_every=ADAPT, **kw)
    nfact = bs.factor_count() - f0
    pen = bs.box_penalties()
    print("adaptive iterations", it.tolist(), "factorisations", nfact, "penalties / rho", (pen / rho).tolist())
    assert (st == 1).all(), (it, st)
    assert 1 <= nfact <= 1 + int(it.max()) // ADAPT, (nfact, it)
    sol = bs.solutions().copy()
    mux, muu = bs.bound_multipliers()
    if states:
        assert_state_bounds_active(bs, sol, mux, xlo, xhi)
    for p, prob in enumerate(probs):
        check_certificate(prob, sol[p], mux[p], muu[p], xlo[p], xhi[p], ulo[p], uhi[p])
        if not states:
            u = split(sol[p], n, m, N)[2]
            ub, _ = bvls_inputs(prob, ulo[p], uhi[p])
            assert rel(u, ub) <= 1e-6, (p, rel(u, ub))
    # the fixed penalty on the same batch (a non-uniform vector behind it: it refactors)
    f0 = bs.factor_count()
    fit, fst = bs.solve_box(**kw)
    assert bs.factor_count() == f0 + 1
    assert (bs.box_penalties() == rho).all()
    print("fixed iterations", fit.tolist(), "status", fst.tolist(), "ratio of totals %.3f" % (it.sum() / fit.sum()))
    assert it.sum() < fit.sum(), (it, fit)
    bs.close()


# ------------------------------------------------------------------------------------------------ d. every schedule

@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6] or c[4], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
def test_every_schedule_meets_the_certificate(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 1500 + p) for p in range(batch)]
    fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "fact": ndlqr.FLAG_KEEP_FACT, "none": 0,
          "strict": ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT}[flags]
    bs = solver(ndlqr, probs, fl)
    ulo, uhi = input_box(oracle, probs, 0.5)
    rho = mean_r(probs)  # (no diag Q scale for the state bounds here)
    if N >= 4:
        xlo, xhi = state_box(oracle, probs, 0.9, adaptive_input_bounded_states(bs, ulo, uhi, rho))
    else:
        xlo, xhi = None, None
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25, adapt_every=ADAPT)
    print("iterations: max %d, median %d" % (int(it.max()), int(np.median(it))))
    assert want is None or bs.schedule() == want, bs.schedule()
    assert (st == 1).all(), (it, st)
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    if xlo is not None:
        assert_state_bounds_active(bs, sol, mux, xlo, xhi)
    inf = np.full((N, n), np.inf)
    for p in sorted({0, batch - 1}):
        check_certificate(probs[p], sol[p], mux[p], muu[p], -inf if xlo is None else xlo[p], inf if xhi is None else xhi[p],
                          ulo[p], uhi[p])
    bs.close()


# ------------------------------------------------------------------------------------------------ e. state rules

def test_state_rules(ndlqr, oracle):
    n, m, N, batch = 12, 4, 64, 4
    probs = [synth(ndlqr, n, m, N, 200 + p) for p in range(batch)]
    rho = mean_r(probs)
    ulo, uhi = input_box(oracle, probs, 0.5)
    kw = dict(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    bs.set_bounds(None, None, ulo, uhi)
    # invalid settings are refused, by the binding's wrapper and by the C entry point
    for bad in (dict(adapt_every=-1), dict(adapt_every=5, rho_min=2.0, rho_max=1.0), dict(adapt_every=5, rho_min=1e7),
                dict(adapt_every=5, rho_max=-1.0)):
        with pytest.raises(RuntimeError):
            bs.solve_box(**dict(kw, **bad))
    with pytest.raises(RuntimeError):
        bs.box_penalties()  # no constrained solve yet
    it, st = bs.solve_box(adapt_every=ADAPT, **kw)
    assert (st == 1).all(), (it, st)
    pen = bs.box_penalties()
    assert pen.shape == (batch,) and (pen != rho).any()  # (the vector is not uniform)
    dev = ndlqr.DeviceArray((batch,))
    bs.box_penalties(dev)
    assert np.array_equal(dev.get(), pen)
    # adapt_every = 0 after new inputs equals a fresh context's fixed-penalty solve, bit for bit
    bs.initialize_flat(*stack(probs))
    f0 = bs.factor_count()
    it0, st0 = bs.solve_box(**kw)
    assert bs.factor_count() == f0 + 1
    fresh = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    fresh.set_bounds(None, None, ulo, uhi)
    it1, st1 = fresh.solve_box(**kw)
    assert np.array_equal(it0, it1) and np.array_equal(st0, st1)
    assert np.array_equal(bs.solutions(), fresh.solutions())
    m0, m1 = bs.bound_multipliers(), fresh.bound_multipliers()
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1])
    assert (bs.box_penalties() == rho).all()
    fresh.close()
    # a fixed-penalty solve behind an adaptive one with a non-uniform vector refactors; behind a fixed one it does not
    bs.solve_box(adapt_every=ADAPT, **kw)
    assert (bs.box_penalties() != rho).any()
    f0 = bs.factor_count()
    bs.solve_box(**kw)
    assert bs.factor_count() == f0 + 1
    bs.solve_box(**kw)
    assert bs.factor_count() == f0 + 1
    # rho_min = rho_max = rho: nothing can move, the fixed-penalty result bit for bit
    a = bs.solutions().copy()
    f0 = bs.factor_count()
    itc, stc = bs.solve_box(adapt_every=ADAPT, rho_min=rho, rho_max=rho, **kw)
    assert bs.factor_count() == f0 and np.array_equal(bs.solutions(), a) and (bs.box_penalties() == rho).all()
    bs.close()


def test_warm_started_mpc_loop_keeps_its_penalties(ndlqr, oracle):
    n, m, N, batch = 12, 4, 64, 8
    probs = [synth(ndlqr, n, m, N, 400 + p) for p in range(batch)]
    rho = mean_r(probs)
    ulo, uhi = input_box(oracle, probs, 0.5)
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, adapt_every=ADAPT)
    bs = solver(ndlqr, probs)
    bs.set_bounds(None, None, ulo[0], uhi[0])
    q, r, d = stack(probs, ("q", "r", "d"))
    x = np.stack([p.x0 for p in probs])
    quiet = 0
    for step in range(6):
        bs.set_rhs_flat(q, r, d, x)
        before = bs.box_penalties().copy() if step > 0 else None
        f0 = bs.factor_count()
        # (rho is ignored by the warm-started steps: they start from the penalties of the step before)
        it, st = bs.solve_box(warm_start=step > 0, **dict(kw, rho=rho if step == 0 else 1e3 * rho))
        assert (st == 1).all(), (step, it)
        nfact = bs.factor_count() - f0
        pen = bs.box_penalties()
        sol = bs.solutions()
        u0 = np.stack([split(sol[p], n, m, N)[2][0] for p in range(batch)])
        cold = solver(ndlqr, [Problem(n, m, N, *(p.arrays()[:7] + (x[i],))) for i, p in enumerate(probs)])
        cold.set_bounds(None, None, ulo[0], uhi[0])
        cit, cst = cold.solve_box(**kw)
        assert (cst == 1).all()
        u0c = np.stack([split(cold.solutions()[p], n, m, N)[2][0] for p in range(batch)])
        cold.close()
        print("step %d: warm iterations %s, cold %s, factorisations %d" % (step, it.tolist(), cit.tolist(), nfact))
        assert rel(u0, u0c) <= 1e-6, (step, rel(u0, u0c))
        if step > 0:
            assert it.sum() <= cit.sum(), (step, it, cit)
            assert nfact <= int(it.max()) // ADAPT, (step, nfact, it)
            if nfact == 0:  # (a start from 1e3 rho would have factored)
                assert np.array_equal(pen, before), step
                quiet += 1
            else:
                assert not np.array_equal(pen, before) or nfact >= 2, step
        x = np.stack([probs[p].A[0].reshape(n, n).T @ x[p] + probs[p].B[0].reshape(m, n).T @ u0[p] + probs[p].d[0]
                      for p in range(batch)])
    # the same right-hand side again, from the converged point: at most 2 iterations, no penalty moves, nothing factored
    pen, f0 = bs.box_penalties().copy(), bs.factor_count()
    it, st = bs.solve_box(warm_start=True, **kw)
    assert (it <= 2).all() and (st == 1).all(), it
    assert bs.factor_count() == f0 and np.array_equal(bs.box_penalties(), pen)
    print("warm-started steps without a factorisation: %d of 5" % quiet)
    bs.close()


def test_multipliers_unbounded_batches_and_non_finite_problems(ndlqr, oracle):
    # bound_multipliers = rho_p y against the strict reference is part of the strict test above; here: fast mode
    n, m, N, batch = 12, 4, 32, 3
    probs = [synth(ndlqr, n, m, N, 500 + p) for p in range(batch)]
    rho = mean_r(probs)
    bs = solver(ndlqr, probs)
    # no finite bound: converged in iteration 1, penalties untouched, nothing refactored
    inf = np.full((N, n), np.inf)
    bs.set_bounds(-inf, inf, None, None)
    f0 = bs.factor_count()
    it, st = bs.solve_box(rho=rho, max_iter=50, adapt_every=1)
    assert (it == 1).all() and (st == 1).all(), (it, st)
    assert (bs.box_penalties() == rho).all() and bs.factor_count() == f0 + 1
    # a NaN in the data of one problem: status 3 at once, its penalty untouched, the others converge
    ulo, uhi = input_box(oracle, probs, 0.5)
    bs.set_bounds(None, None, ulo, uhi)
    x0 = np.stack([p.x0 for p in probs])
    x0[2, 3] = np.nan
    bs.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, check_every=1, adapt_every=ADAPT)
    assert st[2] == 3 and it[2] == 1 and (st[:2] == 1).all(), (it, st)
    assert bs.box_penalties()[2] == rho
    bs.close()


# ------------------------------------------------------------------------------------------------ f. gradients, fast mode

def test_gradients_behind_an_adaptive_forward(ndlqr, oracle):
    n, m, N, batch = 12, 4, 64, 4
    probs = [synth(ndlqr, n, m, N, 1500 + p) for p in range(batch)]
    rho = mean_r(probs)
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.9, adaptive_input_bounded_states(bs, ulo, uhi, rho))
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25, adapt_every=ADAPT)
    assert (st == 1).all(), (it, st)
    pen = bs.box_penalties()
    assert (pen != rho).any()
    sol = bs.solutions().copy()
    g = np.random.default_rng(n + N).standard_normal((batch, bs.nvars))
    f0 = bs.factor_count()
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25)
    print("forward iterations %s, backward %s, penalties / rho %s" % (it.tolist(), ait.tolist(), (pen / rho).tolist()))
    assert (ast == 1).all(), (ait, ast)
    assert bs.factor_count() == f0 and np.array_equal(bs.box_penalties(), pen)
    w, grads, bg = bs.adjoint(), bs.gradients(), bs.bound_gradients()
    for p, prob in enumerate(probs):
        codes = codes_of(bs, sol, p, xlo, xhi, ulo, uhi)
        wr, nur = active_adjoint(prob, codes, g[p])
        assert rel(w[p], wr) <= 1e-6, (p, rel(w[p], wr))
        bref = bound_grads(codes, nur, n)
        nu = np.concatenate([bg["xlo"][p] + bg["xhi"][p], bg["ulo"][p] + bg["uhi"][p]], axis=1)
        assert rel(nu, nur) <= 1e-6, p
        for k in BOUNDS:
            assert np.array_equal(bg[k][p] != 0, bref[k] != 0) or rel(bg[k][p], bref[k]) <= 1e-6, (p, k)
        assert adjoint_residual(prob, g[p], w[p], nu) <= 1e-6
        ref = grad_formula(prob, sol[p], wr)
        for k in ARGS:
            assert rel(grads[k][p], ref[k]) <= 1e-6, (p, k, rel(grads[k][p], ref[k]))
    # the batch sums use every problem's own penalty too
    s = bs.bound_gradients(summed=True)
    for k in BOUNDS:
        ref = bg[k].sum(axis=0)
        assert np.abs(s[k] - ref).max() <= 1e-12 * max(1.0, np.abs(bg[k]).sum(axis=0).max()), k
    bs.close()


def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_box_adaptive as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_torch_gradcheck_with_adapt_every():
    _run_case("_case_gradcheck")


def _case_gradcheck(ndlqr):
    """test_gpu_box_gradients._case_gradcheck with the adaptive penalty, from a rho 100 times too small"""
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    from test_gpu_box_gradients import BOUNDS as B, _torch_bounds, _torch_problem
    n, m, N, batch = 3, 2, 8, 2
    t = _torch_problem(ndlqr, n, m, N, batch, 2300)
    bnd = _torch_bounds(t, n, m, N, batch, "per_problem", frac_u=0.5, frac_x=50.0)  # inputs cut, states far away
    fn = lambda *a: lqr_solve_box(*a, rho=0.01, eps_abs=1e-12, eps_rel=1e-12, max_iter=50000, adapt_every=ADAPT)
    args = tuple(t[k] for k in ARGS) + tuple(bnd[k] for k in B)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)
    with pytest.raises(RuntimeError, match="adapt_every"):
        lqr_solve_box(*[a.detach() for a in args], max_iter=1)
