"""Objective values and stage costs on the device (ndlqr_BatchObjective, BatchSolver.objective, lqr_value; DESIGN.md section
3.24) against objective_support.exact -- fractions.Fraction on the float64 bits of the inputs and of the delivered solution.

Bars. Diagonal costs, and dense costs evaluated in the caller's variables (a constrained solve or polish): 4 eps S for J,
4 eps S_k for l_k -- at most two rounded factor products per term at eps / 2 each, the final rounding, and a double-double
accumulation that contributes nothing at this scale. Dense-cost mode with the solution in the reduced variables:
max(8 x the float64 restatement's own error against exact, 16 eps S), the bar of test_gpu_gains and test_gpu_cost; the ratio
to it is printed per shape (the table of DESIGN.md section 3.24).
"""
import numpy as np
import pytest

import cost_support as cs
import objective_support as osup
from test_gpu_cost import flag_modes

pytestmark = pytest.mark.gpu

EPS = osup.EPS
DIAG_CASES = [(n, m, N) for (n, m) in osup.SHAPES for N in osup.HORIZONS] + [(64, 16, 4)]
DENSE_CASES = [(n, m, N) for (n, m) in osup.SHAPES for N in osup.HORIZONS]


def with_rhs(probs, q, r, d, x0):
    """the problems with another right-hand side ([batch, N, ..] arrays)"""
    return [dict(p, q=q[i], r=r[i], d=d[i], x0=x0[i]) for i, p in enumerate(probs)]


def check_exact(tag, out, probs, Z, mult=4.0):
    """J and stage of `out` against exact on Z with the bar mult eps S / mult eps S_k; returns the largest ratios"""
    ex = osup.exact_batch(probs, Z)
    eJ, el = np.abs(out["J"] - ex["J"]), np.abs(out["stage"] - ex["ell"])
    rJ, rl = float((eJ / (EPS * ex["S"])).max()), float((el / (EPS * ex["S_k"])).max())
    print("objective", tag, "J: %.3f eps S   stage: %.3f eps S_k" % (rJ, rl))
    assert np.all(eJ <= mult * EPS * ex["S"]), (tag, out["J"], ex["J"], ex["S"])
    assert np.all(el <= mult * EPS * ex["S_k"]), (tag, out["stage"], ex["ell"], ex["S_k"])
    return ex


def check_dense(tag, out, probs, Z):
    """... with the bar of dense-cost mode; prints the ratio to it"""
    ex = osup.exact_batch(probs, Z)
    barJ, barl, ownJ, ownl = osup.dense_bar(probs, Z, ex)
    eJ, el = np.abs(out["J"] - ex["J"]), np.abs(out["stage"] - ex["ell"])
    print("objective", tag, "J: %.3f of its bar (%.2f eps S, restatement %.2f eps S)   stage: %.3f of its bar"
          % (float((eJ / barJ).max()), float((eJ / (EPS * ex["S"])).max()), float((ownJ / (EPS * ex["S"])).max()),
             float((el / barl).max())))
    assert np.all(eJ <= barJ), (tag, out["J"], ex["J"], barJ)
    assert np.all(el <= barl), (tag, out["stage"], ex["ell"], barl)
    return ex


# ------------------------------------------------------------------ 1. per problem and per knot, diagonal costs

@pytest.mark.parametrize("n,m,N", DIAG_CASES)
def test_diagonal_costs_per_problem_and_knot(ndlqr, n, m, N):
    probs = osup.families(n, m, N, "diagonal")
    bs = osup.diagonal_solver(ndlqr, probs)
    assert bs.solve() == 0
    out = bs.objective(stage=True)
    assert out["J"].shape == (osup.BATCH,) and out["stage"].shape == (osup.BATCH, N)
    check_exact((n, m, N), out, probs, bs.solutions())
    bs.close()


def test_diagonal_costs_in_every_flag_mode(ndlqr):
    n, m, N = 12, 4, 8
    probs = osup.families(n, m, N, "diagonal")
    for flags in flag_modes(ndlqr):
        bs = osup.diagonal_solver(ndlqr, probs, flags)
        assert bs.solve() == 0
        check_exact((n, m, N, "flags %d" % flags), bs.objective(stage=True), probs, bs.solutions())
        bs.close()


# ------------------------------------------------------------------ 2. more than one chunk

@pytest.mark.parametrize("batch", [1, 3])
def test_more_than_one_chunk(ndlqr, batch):
    knots, threads = ndlqr.objective_constants()
    assert knots > 0 and threads % 64 == 0
    n, m, N = 6, 3, 2 * knots + 5
    probs = osup.families(n, m, N, "diagonal", batch)
    bs = osup.diagonal_solver(ndlqr, probs)
    assert bs.solve() == 0
    out = bs.objective(stage=True)
    check_exact((n, m, N, batch), out, probs, bs.solutions())
    assert np.array_equal(bs.objective()["J"], out["J"])
    bs.close()


# ------------------------------------------------------------------ 3. dense costs, with and without H

@pytest.mark.parametrize("kind", ["dense", "dense-noH"])
@pytest.mark.parametrize("n,m,N", DENSE_CASES)
def test_dense_costs_per_problem_and_knot(ndlqr, n, m, N, kind):
    probs = osup.families(n, m, N, kind)
    bs = ndlqr.BatchSolver(n, m, N, len(probs))
    A, B, Q, H, R, q, r, d, x0 = cs.flat(probs)
    bs.initialize_flat_dense(A, B, Q, H if kind == "dense" else None, R, q, r, d, x0)
    assert bs.solve() == 0
    check_dense((n, m, N, kind), bs.objective(stage=True), probs, bs.solutions())
    bs.close()


# ------------------------------------------------------------------ 4. constrained states

def two_rows(p, z_unc, seed):
    """p = 2 dense rows with bounds at 0.6 x the largest |w| of the unconstrained solution: some rows end active"""
    import lin_support as ls
    n, m, N = cs.dims(p)
    rng = np.random.default_rng([seed, n, m, N, 23])
    Cr = rng.standard_normal((N, 2, n)) / np.sqrt(n)
    Dr = rng.standard_normal((N, 2, m)) / np.sqrt(m)
    w = ls.rows_of(p, Cr, Dr, np.asarray(z_unc, dtype=np.float64))
    hi = np.broadcast_to(0.6 * np.abs(w).max(axis=0), (N, 2)).copy()
    return dict(p=p, C=Cr, D=Dr, lo=-hi, hi=hi)


@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 5)])
def test_after_constrained_solve_and_polish(ndlqr, n, m, N):
    import lin_support as ls
    fam = cs.family(n, m, N, "moderate")
    probs = fam["probs"]
    cases = [two_rows(p, fam["z"][i], 40 + i) for i, p in enumerate(probs)]
    bs = ndlqr.BatchSolver(n, m, N, len(probs))
    bs.initialize_flat_constrained(*cs.flat(probs), *ls.flat_rows(cases))
    # a plain solve in constrained mode: the unconstrained optimum, in the reduced variables of the unshifted problem
    assert bs.solve() == 0
    unc = check_dense((n, m, N, "plain solve, constrained mode"), bs.objective(stage=True), probs, bs.solutions())
    iters, status = bs.solve_constrained(rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000)
    mu = bs.constraint_multipliers()
    assert (status == 1).all(), (iters, status)
    assert all(np.abs(mu[i]).max() > 0 for i in range(len(probs))), mu
    con = check_exact((n, m, N, "constrained"), bs.objective(stage=True), probs, bs.solutions())
    assert np.all(con["J"] > unc["J"])  # (active rows: the constrained value lies above the unconstrained one)
    steps, pstatus = bs.polish_constrained()
    print("polish status", pstatus)
    check_exact((n, m, N, "polished"), bs.objective(stage=True), probs, bs.solutions())
    # and the plain solve gives what it gave
    assert bs.solve() == 0
    check_dense((n, m, N, "plain solve again"), bs.objective(stage=True), probs, bs.solutions())
    bs.close()


def box_setup(ndlqr, n, m, N, flags):
    """a diagonal problem with input bounds at half the mean |u| of the unconstrained solution: (solver, problems, rho)"""
    probs = osup.families(n, m, N, "diagonal")
    bs = osup.diagonal_solver(ndlqr, probs, flags)
    assert bs.solve() == 0
    u = np.stack([cs.split(z, n, m, N)[2] for z in bs.solutions()])
    uh = np.tile(0.5 * np.abs(u[:, :N - 1]).mean(axis=1, keepdims=True), (1, N, 1))
    bs.set_bounds(ulo=-uh, uhi=uh)
    Qd, _ = osup.diagonals(probs)
    return bs, probs, float(Qd.mean())


@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 8)])
def test_after_box_solve_and_polish(ndlqr, n, m, N):
    bs, probs, rho = box_setup(ndlqr, n, m, N, ndlqr.FLAG_KEEP_RECORDS)
    unc = bs.objective()["J"]
    iters, status = bs.solve_box(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
    assert (status == 1).all(), (iters, status)
    mu_x, mu_u = bs.bound_multipliers()
    assert all(np.abs(mu_u[i]).max() > 0 for i in range(len(probs)))
    box = check_exact((n, m, N, "box"), bs.objective(stage=True), probs, bs.solutions())
    assert np.all(box["J"] > unc)
    steps, pstatus = bs.polish_box()
    print("polish status", pstatus)
    check_exact((n, m, N, "box polished"), bs.objective(stage=True), probs, bs.solutions())
    bs.close()


# ------------------------------------------------------------------ 5. follows the solution and its right-hand side

def new_rhs(rng, n, m, N, batch):
    return (rng.standard_normal((batch, N, n)), rng.standard_normal((batch, N, m)), 0.1 * rng.standard_normal((batch, N, n)),
            rng.standard_normal((batch, n)))


@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (12, 4, 5)])
def test_follows_the_solution_and_its_right_hand_side(ndlqr, n, m, N):
    batch = osup.BATCH
    rng = np.random.default_rng([n, m, N, 5])
    probs = osup.families(n, m, N, "diagonal")
    bs = osup.diagonal_solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    values = []

    def check(tag, cur):
        ex = check_exact((n, m, N, tag), bs.objective(stage=True), cur, bs.solutions())
        values.append(ex["J"])

    assert bs.solve() == 0
    check("solve", probs)
    q, r, d, x0 = new_rhs(rng, n, m, N, batch)
    bs.set_rhs_flat(q, r, d, x0)
    assert bs.solve_rhs_only() == 0
    check("set_rhs_flat + solve_rhs_only", with_rhs(probs, q, r, d, x0))
    bs.set_flags(0)  # (the steps that follow alternate between the two buffer sets)
    hold = {}
    for name, a in zip("qrdx", new_rhs(rng, n, m, N, batch)):
        hold[name] = ndlqr.pinned_empty(a.shape)
        hold[name][...] = a
    soln = ndlqr.pinned_empty((batch, bs.nvars))
    assert bs.step_async(hold["q"], hold["r"], hold["d"], hold["x"], soln) == 0
    assert bs.synchronize() == 0
    check("full step", with_rhs(probs, hold["q"], hold["r"], hold["d"], hold["x"]))
    assert np.array_equal(soln, bs.solutions())
    for rep in range(2):  # two x0-only steps: one on each buffer set
        x_new = ndlqr.pinned_empty((batch, n))
        x_new[...] = rng.standard_normal((batch, n))
        assert bs.step_async(None, None, None, x_new, soln) == 0
        assert bs.synchronize() == 0
        check("x0-only step %d" % rep, with_rhs(probs, hold["q"], hold["r"], hold["d"], x_new))
        assert np.array_equal(soln, bs.solutions())
    # a plain solve behind the steps sees the latest right-hand side on whichever set it lands
    assert bs.solve() == 0
    check("solve behind the steps", with_rhs(probs, hold["q"], hold["r"], hold["d"], x_new))
    for a, b in zip(values[:-2], values[1:-1]):
        assert np.all(a != b)
    bs.close()
    # dense-cost mode: the step in the caller's variables
    dprobs = osup.families(n, m, N, "dense")
    bs = osup.dense_solver(ndlqr, dprobs)
    assert bs.solve() == 0
    dvalues = [check_dense((n, m, N, "dense solve"), bs.objective(stage=True), dprobs, bs.solutions())["J"]]
    q, r, d, x0 = new_rhs(rng, n, m, N, batch)
    out = np.zeros((batch, bs.nvars))
    assert bs.step_dense_async(q, r, d, x0, out) == 0
    assert bs.synchronize() == 0
    cur = with_rhs(dprobs, q, r, d, x0)
    dvalues.append(check_dense((n, m, N, "dense step"), bs.objective(stage=True), cur, bs.solutions())["J"])
    x1 = rng.standard_normal((batch, n))
    assert bs.step_dense_async(None, None, None, x1, out) == 0
    assert bs.synchronize() == 0
    cur = with_rhs(dprobs, q, r, d, x1)
    dvalues.append(check_dense((n, m, N, "dense x0-only step"), bs.objective(stage=True), cur, bs.solutions())["J"])
    for a, b in zip(dvalues, dvalues[1:]):
        assert np.all(a != b)
    bs.close()


# ------------------------------------------------------------------ 6. touches nothing

def test_touches_nothing(ndlqr):
    n, m, N = 12, 4, 8
    probs = osup.families(n, m, N, "diagonal")
    rng = np.random.default_rng(6)
    rhs = new_rhs(rng, n, m, N, osup.BATCH)
    seen = {}
    for call in (False, True):
        bs = osup.diagonal_solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
        assert bs.solve() == 0
        objective = (lambda: bs.objective(stage=True)) if call else (lambda: None)
        objective()
        got = [bs.solutions().copy()]
        objective()
        bs.set_rhs_flat(*rhs)
        objective()  # (the new right-hand side at the old solution: a read-out all the same)
        assert bs.solve_rhs_only() == 0
        objective()
        got.append(bs.solutions().copy())
        got.append(np.asarray(bs.cholesky_failure_counts()).copy())
        bs.close()
        bs, _, rho = box_setup(ndlqr, n, m, N, ndlqr.FLAG_KEEP_RECORDS)
        it1, st1 = bs.solve_box(rho=rho, eps_abs=1e-3, eps_rel=1e-3, max_iter=4000)
        objective = (lambda: bs.objective(stage=True)) if call else (lambda: None)
        objective()
        got += [a.copy() for a in bs.bound_multipliers()]
        objective()
        it2, st2 = bs.solve_box(rho=rho, eps_abs=1e-4, eps_rel=1e-4, max_iter=4000, warm_start=True)
        got += [it1.copy(), st1.copy(), it2.copy(), st2.copy(), bs.solutions().copy()]
        bs.close()
        seen[call] = got
    assert len(seen[False]) == len(seen[True])
    for a, b in zip(seen[False], seen[True]):
        assert np.array_equal(a, b)


def test_same_bits_twice_and_in_every_memory(ndlqr):
    n, m, N = 7, 9, 5
    probs = osup.families(n, m, N, "diagonal")
    bs = osup.diagonal_solver(ndlqr, probs)
    assert bs.solve() == 0
    first = bs.objective(stage=True)
    again = bs.objective(stage=True)
    pinned = bs.objective(out=dict(J=ndlqr.pinned_empty((osup.BATCH,)), stage=ndlqr.pinned_empty((osup.BATCH, N))))
    dev = bs.objective(out=dict(J=ndlqr.DeviceArray((osup.BATCH,)), stage=ndlqr.DeviceArray((osup.BATCH, N))))
    mixed = bs.objective(out=dict(J=ndlqr.DeviceArray((osup.BATCH,)), stage=np.zeros((osup.BATCH, N))))
    only_J = bs.objective(out=dict(J=ndlqr.DeviceArray((osup.BATCH,))))
    for k in ("J", "stage"):
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], pinned[k])
        assert np.array_equal(first[k], dev[k].get())
    assert np.array_equal(first["J"], mixed["J"].get()) and np.array_equal(first["stage"], mixed["stage"])
    assert np.array_equal(first["J"], only_J["J"].get())
    with pytest.raises(ValueError):
        bs.objective(out=dict(J=np.zeros(osup.BATCH), cost=np.zeros(osup.BATCH)))
    with pytest.raises(ValueError):
        bs.objective(out=dict(J=np.zeros(osup.BATCH + 1)))
    bs.close()


# ------------------------------------------------------------------ 7. never-read data and bad members

@pytest.mark.parametrize("N", [8, 5])
@pytest.mark.parametrize("kind", ["diagonal", "dense"])
def test_never_read_data_and_bad_members(ndlqr, kind, N):
    n, m = 12, 4
    probs = osup.families(n, m, N, kind)
    make = osup.diagonal_solver if kind == "diagonal" else osup.dense_solver
    bs = make(ndlqr, probs)
    assert bs.solve() == 0
    clean = bs.objective(stage=True)
    bs.close()
    poisoned = [{k: v.copy() for k, v in p.items()} for p in probs]
    for p in poisoned:
        for k in ("A", "B", "R", "r", "d") + (("H",) if kind == "dense" else ()):
            p[k][N - 1] = np.nan
    if kind == "diagonal":  # (diagonal_solver takes the diagonals of R: every entry of the last knot's is NaN)
        assert np.isnan(osup.diagonals(poisoned)[1][:, N - 1]).all()
    bs = make(ndlqr, poisoned)
    assert bs.solve() == 0
    got = bs.objective(stage=True)
    assert np.array_equal(got["J"], clean["J"]) and np.array_equal(got["stage"], clean["stage"])
    bs.close()
    bad = [{k: v.copy() for k, v in p.items()} for p in probs]
    bad[1]["q"][1, 0] = np.nan
    bs = make(ndlqr, bad)
    bs.solve()
    got = bs.objective(stage=True)
    assert np.isnan(got["J"][1]) and np.isnan(got["stage"][1, 1])
    for i in (0, 2):
        assert got["J"][i] == clean["J"][i] and np.array_equal(got["stage"][i], clean["stage"][i])
    bs.close()


# ------------------------------------------------------------------ 8. refusals

def refused(bs, call):
    with pytest.raises(RuntimeError) as e:
        call()
    msg = bs.L.ndlqr_hip_last_error().decode()
    assert "-1" in str(e.value) and msg.startswith("ndlqr_hip_objective:"), (str(e.value), msg)
    return msg


def test_refusals(ndlqr):
    n, m, N = 12, 4, 16
    probs = osup.families(n, m, N, "diagonal")
    bs = osup.diagonal_solver(ndlqr, probs)
    refused(bs, bs.objective)  # before any solve
    assert bs.solve() == 0
    good = bs.objective(stage=True)
    # J null
    assert bs.L.ndlqr_BatchObjective(bs.h, None, None) == -1
    assert bs.L.ndlqr_hip_last_error().decode().startswith("ndlqr_hip_objective:")
    # a step that computed a slice alone
    bs.set_step_selection(0, 1, ndlqr.SOLN_INPUT | ndlqr.SOLN_ONLY)
    x0 = ndlqr.pinned_empty((osup.BATCH, n))
    x0[...] = np.stack([p["x0"] for p in probs])
    u0 = ndlqr.pinned_empty((osup.BATCH, 1, m))
    assert bs.step_async(None, None, None, x0, u0) == 0
    assert bs.synchronize() == 0
    assert "NDLQR_SOLN_ONLY" in refused(bs, bs.objective)
    bs.set_step_selection()
    assert bs.solve() == 0
    again = bs.objective(stage=True)
    assert np.array_equal(again["J"], good["J"]) and np.array_equal(again["stage"], good["stage"])
    bs.close()
    # a time-axis shard (the two chunks as two solvers of one process, as test_time_axis.py runs them)
    n, m, N, batch, G = 12, 4, 512, 3, 2
    solvers = [ndlqr.BatchSolver(n, m, N, batch) for _ in range(G)]
    for bs in solvers:
        bs.initialize_synthetic(3)
    count = solvers[0].time_shard_top_doubles(G)
    assert count > 0
    bufs = []
    for g, bs in enumerate(solvers):
        assert bs.time_shard_factor(g, G) == 0
        bufs.append(np.zeros(count))
        assert bs.time_shard_export(G, bufs[-1].ctypes.data) == 0
    total = np.sum(bufs, axis=0)
    for g, bs in enumerate(solvers):
        assert bs.time_shard_import(G, total.ctypes.data) == 0 and bs.time_shard_finish(g, G) == 0
        assert bs.synchronize() == 0 and bs.schedule() == "reduced-time-shard"
        assert "time-axis shard" in refused(bs, bs.objective)
    bs = solvers[0]
    assert bs.solve() == 0
    check_exact_synthetic = bs.objective(stage=True)
    assert np.isfinite(check_exact_synthetic["J"]).all() and np.isfinite(check_exact_synthetic["stage"]).all()
    for bs in solvers:
        bs.close()


# ------------------------------------------------------------------ 9. lqr_value, lqr_value_dense
# torch runs in a child process (test_gpu_gradients.py has the reason: torch's own HIP runtime must start first)

def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_objective as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout)


def _case_lqr_value(ndlqr, n, m, N, dense):
    import torch
    from rslqr_amd.autograd import lqr_solve, lqr_solve_dense, lqr_value, lqr_value_dense
    names = cs.NAMES if dense else ("A", "B", "Q", "R", "q", "r", "d", "x0")
    probs = [dict(p) for p in osup.families(n, m, N, "dense" if dense else "diagonal")]
    shared = "A" if dense else "q"
    for p in probs:
        p[shared] = probs[0][shared]
    arrays = {k: np.stack([p[k] for p in probs]) for k in names}
    if not dense:
        arrays["Q"], arrays["R"] = osup.diagonals(probs)

    def tensors():
        t = {k: torch.tensor(arrays[k], dtype=torch.float64, device="cuda") for k in names}
        t[shared] = t[shared][0].clone()
        return {k: v.requires_grad_(True) for k, v in t.items()}

    w = torch.tensor(np.random.default_rng([n, m, N]).standard_normal(len(probs)), device="cuda")
    t = tensors()
    J = (lqr_value_dense if dense else lqr_value)(*[t[k] for k in names])
    # forward: objective() of a solver of its own, bit for bit
    bs = (osup.dense_solver if dense else osup.diagonal_solver)(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    assert np.array_equal(J.detach().cpu().numpy(), bs.objective()["J"])
    bs.close()
    got = torch.autograd.grad((w * J).sum(), [t[k] for k in names])
    # backward: autograd of the same objective written in torch on the output of lqr_solve(_dense), its adjoint path
    s = tensors()
    z = (lqr_solve_dense if dense else lqr_solve)(*[s[k] for k in names])
    full = {k: (v.unsqueeze(0).expand(len(probs), *v.shape) if k == shared else v) for k, v in s.items()}
    ref = torch.autograd.grad((w * osup.value_torch(full, z, n, m, N, dense)).sum(), [s[k] for k in names])
    for k, a, b in zip(names, got, ref):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a.shape == b.shape == tuple(t[k].shape), k
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print("lqr_value gradient", (n, m, N, dense), k, err)
        assert err <= 1e-9, (k, err)
        if k in ("A", "B", "H", "R", "r", "d"):
            assert not (a[N - 1] if k == shared else a[:, N - 1]).any(), k


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 5)])
def test_lqr_value(n, m, N, dense):
    _run_case("_case_lqr_value", n, m, N, dense)
