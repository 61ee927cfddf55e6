"""Batch solver at horizons that are no power of two ("Padded horizon"): the device runs the next
power of two, P, and only the boundary knows. Two references:
  - the oracle on horizon_support.pad_problem(prob) (validated in test_horizon_host.py), cut to the caller's nvars;
  - a BatchSolver of horizon P on the host-padded problems: what the device must reproduce on the [:N] prefixes -- bit
    for bit in strict mode, within 1e-9 (the project's parity bar) otherwise.
Horizons: 3 -> 4 (device horizon below 8), 5 -> 8, 7 -> 8 (one tail knot: the last-knot rule alone), 9 -> 16 (tail longer
than the problem), 33 -> 64, and 100 -> 128 once per kernel family. Block sizes, one per launch family: (6,3), (12,4),
(7,9) (zero-padded block size as well), (16,4) (runtime-sized separator-only), (12,4) under FLAG_GENERIC (knot-based)."""
import ctypes as C

import numpy as np
import pytest

from box_support import bvls_inputs, certificate, split
from horizon_support import (ARGS, kkt_bar, kkt_inf, next_pow2, pad_problem, pad_vector, poisoned, reference, rel, stack,
                             synth)

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
BATCH = 3
GENERIC = "generic"
FAMILIES = [(6, 3, None), (12, 4, None), (7, 9, None), (16, 4, None), (12, 4, GENERIC)]
HORIZONS = [3, 5, 7, 9, 33]
CASES = [(n, m, f, N) for (n, m, f) in FAMILIES for N in HORIZONS] + [(n, m, f, 100) for (n, m, f) in FAMILIES]
CASES += [(24, 8, None, 3), (24, 8, None, 7)]  # beyond 16 states the device-side packer is pack_flat_tiled
SEED0 = 900

_cache = {}


def problems(ndlqr, oracle, n, m, N):
    """three problems of the shape (synthetic seeds SEED0 + p: what initialize_synthetic(SEED0) generates) and the reference
    solution of each, computed once"""
    key = (n, m, N)
    if key not in _cache:
        probs = [synth(ndlqr, n, m, N, SEED0 + p) for p in range(BATCH)]
        refs = []
        for prob in probs:
            z, tail, fails = reference(oracle, prob)
            assert fails == 0 and not tail.any()
            z.setflags(write=False)
            refs.append(z)
        _cache[key] = (probs, np.stack(refs))
    return _cache[key]


def family_flags(ndlqr, fam):
    return ndlqr.FLAG_GENERIC if fam == GENERIC else 0


def new_solver(ndlqr, probs, flags=0, init=True):
    p = probs[0]
    bs = ndlqr.BatchSolver(p.n, p.m, p.N, len(probs), flags=flags)
    if init:
        bs.initialize_flat(*stack(probs))
    return bs


def padded_solver(ndlqr, probs, flags=0):
    return new_solver(ndlqr, [pad_problem(p) for p in probs], flags)


def init_device(ndlqr, bs, probs):
    arrs = [ndlqr.DeviceArray(a.shape).set(a) for a in stack(probs)]
    bs.initialize_flat_device(*[a.ptr for a in arrs])
    bs.synchronize()
    return arrs


def check(sol, refs, probs, strict, what):
    assert np.isfinite(sol).all(), what
    for p, prob in enumerate(probs):
        if strict:
            assert np.array_equal(sol[p], refs[p]), (what, p, rel(sol[p], refs[p]))
        else:
            assert rel(sol[p], refs[p]) <= REL_TOL, (what, p, rel(sol[p], refs[p]))
            assert kkt_inf(prob, sol[p]) <= kkt_bar(prob, sol[p]), (what, p)


# ------------------------------------------------------------------------------------------------ 1. solve parity

@pytest.mark.parametrize("n,m,fam,N", CASES)
def test_solve_parity_in_every_mode(ndlqr, oracle, n, m, fam, N):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    bad = [poisoned(p) for p in probs]
    base = family_flags(ndlqr, fam)
    bs = new_solver(ndlqr, probs, init=False)
    modes = [("strict", ndlqr.FLAG_STRICT_FP), ("keep_fact", ndlqr.FLAG_KEEP_FACT), ("keep_records", ndlqr.FLAG_KEEP_RECORDS),
             ("default", 0)]
    for name, fl in modes:
        bs.set_flags(base | fl)
        strict = name == "strict"
        bs.initialize_flat(*stack(probs))
        assert bs.solve() == 0, name
        check(bs.solutions(), refs, probs, strict, name)
        # NaN in A, B, R, r, d of the caller's last knot never reaches the device: through the host packer ...
        bs.initialize_flat(*stack(bad))
        assert bs.solve() == 0, name
        check(bs.solutions(), refs, probs, strict, name + " poisoned, host packer")
        # ... and through the device-side one
        keep = init_device(ndlqr, bs, bad)
        assert bs.solve() == 0, name
        check(bs.solutions(), refs, probs, strict, name + " poisoned, device packer")
        del keep
    bs.close()


# ------------------------------------------------------------------------------------------------ 2. every upload path

def lqr_problem_list(ndlqr, n, m, N, seeds):
    L = ndlqr.lib()
    ptrs = [L.ndlqr_NewSyntheticLQRProblem(n, m, N, s) for s in seeds]
    assert all(ptrs)
    arr = (type(ptrs[0]) * len(ptrs))(*ptrs)
    return ptrs, arr


UPLOAD_CASES = [(6, 3, None, 3), (6, 3, None, 7), (12, 4, None, 5), (12, 4, None, 33), (12, 4, None, 100), (7, 9, None, 9),
                (16, 4, None, 7), (12, 4, GENERIC, 9)]


@pytest.mark.parametrize("n,m,fam,N", UPLOAD_CASES)
def test_every_upload_path_gives_the_same_solution(ndlqr, oracle, n, m, fam, N):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    L = ndlqr.lib()
    bs = new_solver(ndlqr, probs, family_flags(ndlqr, fam), init=False)
    # LQRProblem list
    ptrs, arr = lqr_problem_list(ndlqr, n, m, N, [SEED0 + p for p in range(BATCH)])
    assert L.ndlqr_InitializeBatch(bs.h, arr, BATCH) == 0
    for q in ptrs:
        L.ndlqr_FreeLQRProblem(q)
    assert bs.solve() == 0
    first = bs.solutions()
    check(first, refs, probs, False, "LQRProblem list")
    # flat host, flat device, synthetic
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), first), "flat host"
    keep = init_device(ndlqr, bs, probs)
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), first), "flat device"
    bs.initialize_synthetic(SEED0)
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), first), "synthetic"
    assert np.array_equal(bs.solution(1), first[1])
    # the device-side copy: [batch][nvars] at the caller's pitch, nothing behind it
    big = ndlqr.DeviceArray((BATCH * bs.nvars + 5,)).set(np.full(BATCH * bs.nvars + 5, 7.0))
    bs.solutions_to_device(big.ptr)
    bs.synchronize()
    got = big.get()
    assert np.array_equal(got[: BATCH * bs.nvars].reshape(BATCH, bs.nvars), first) and (got[BATCH * bs.nvars:] == 7.0).all()
    del keep
    bs.close()


@pytest.mark.parametrize("n,m,fam,N", UPLOAD_CASES)
def test_rhs_only_steps_and_slices(ndlqr, oracle, n, m, fam, N):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    # a second right-hand side on the same matrices: q, r, d, x0 of other seeds
    alt = []
    for p, prob in enumerate(probs):
        g = synth(ndlqr, n, m, N, SEED0 + 50 + p)
        alt.append(type(prob)(n, m, N, prob.A, prob.B, prob.Q, prob.R, g.q, g.r, g.d, g.x0))
    arefs = np.stack([reference(oracle, a)[0] for a in alt])
    # x0 alone replaced on top of `alt`
    alt0 = [type(a)(n, m, N, a.A, a.B, a.Q, a.R, a.q, a.r, a.d, 0.5 * a.x0 + 0.1) for a in alt]
    a0refs = np.stack([reference(oracle, a)[0] for a in alt0])
    base = family_flags(ndlqr, fam)

    # set_rhs + solve_rhs_only on a kept factorisation (NaN in r, d of the last knot as well)
    bs = new_solver(ndlqr, probs, base | ndlqr.FLAG_KEEP_FACT)
    assert bs.solve() == 0
    bad = [poisoned(a) for a in alt]
    bs.set_rhs_flat(*stack(bad, ("q", "r", "d", "x0")))
    assert bs.solve_rhs_only() == 0
    check(bs.solutions(), arefs, alt, False, "rhs only")
    bs.close()

    # steps: full and x0-only, alternating, so that both buffer sets take both kinds
    bs = new_solver(ndlqr, probs, base)
    assert bs.solve() == 0
    full = [ndlqr.pinned_empty(a.shape) for a in stack(bad, ("q", "r", "d", "x0"))]
    for dst, a in zip(full, stack(bad, ("q", "r", "d", "x0"))):
        dst[...] = a
    x0b = ndlqr.pinned_empty((BATCH, n))
    x0b[...] = np.stack([a.x0 for a in alt0])
    outs = [ndlqr.pinned_empty((BATCH, bs.nvars + 1)) for _ in range(5)]
    expect = []
    for i, out in enumerate(outs):
        out[...] = 7.0
        flat = out.reshape(-1)[: BATCH * bs.nvars]
        if i % 2 == 0 or i == 3:  # full, x0, full, full, full ... with x0-only steps on both parities
            assert bs.step_async(full[0], full[1], full[2], full[3], flat) == 0
            expect.append((arefs, alt))
        else:
            assert bs.step_async(None, None, None, x0b, flat) == 0
            expect.append((a0refs, alt0))
    bs.synchronize()
    for i, out in enumerate(outs):
        flat = out.reshape(-1)
        check(flat[: BATCH * bs.nvars].reshape(BATCH, bs.nvars), expect[i][0], expect[i][1], False, "step %d" % i)
        assert (flat[BATCH * bs.nvars:] == 7.0).all(), i
    # a second x0-only step directly behind an x0-only one (the other buffer set's q, r, d are brought up to date)
    for i in range(2):
        assert bs.step_async(None, None, None, x0b, outs[i].reshape(-1)[: BATCH * bs.nvars]) == 0
    bs.synchronize()
    for i in range(2):
        check(outs[i].reshape(-1)[: BATCH * bs.nvars].reshape(BATCH, bs.nvars), a0refs, alt0, False, "x0 step %d" % i)

    # a step with a selection: u of knot 0 alone
    bs.set_step_selection(0, 1, ndlqr.SOLN_INPUT)
    u0 = ndlqr.pinned_empty((BATCH, 1, m))
    assert bs.step_async(full[0], full[1], full[2], full[3], u0) == 0
    bs.synchronize()
    zb = 2 * n + m
    for p in range(BATCH):
        assert rel(u0[p, 0], arefs[p][2 * n: zb]) <= REL_TOL
    bs.set_step_selection()

    # slices of a solve: the last two knots (lambda, x; u of knot N - 1 is not part of the solution), u of knot 0
    bs.initialize_flat(*stack(probs))
    tail2 = ndlqr.pinned_empty((BATCH, 2, 2 * n))
    assert bs.solve_slices_async(N - 2, 2, ndlqr.SOLN_LAMBDA | ndlqr.SOLN_STATE, tail2) == 0
    bs.synchronize()
    for p in range(BATCH):
        want = np.concatenate([refs[p][(N - 2) * zb: (N - 2) * zb + 2 * n], refs[p][(N - 1) * zb: (N - 1) * zb + 2 * n]])
        assert rel(tail2[p].reshape(-1), want) <= REL_TOL
    assert bs.solve() == 0
    got = bs.solution_slices(N - 2, 2, ndlqr.SOLN_LAMBDA | ndlqr.SOLN_STATE)
    assert rel(got, np.asarray(tail2)) <= REL_TOL
    got = bs.solution_slices(0, 1, ndlqr.SOLN_INPUT)
    for p in range(BATCH):
        assert rel(got[p, 0], refs[p][2 * n: zb]) <= REL_TOL
    # knots are bounded by the caller's horizon: a slice reaching beyond it is refused
    L = ndlqr.lib()
    past = ndlqr.pinned_empty((BATCH, 2, 2 * n))
    assert bs.solve_slices_async(N - 1, 2, ndlqr.SOLN_LAMBDA | ndlqr.SOLN_STATE, past) == -1
    assert L.ndlqr_CopyBatchSolutionSlices(bs.h, N - 1, 2, 3, past.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert L.ndlqr_CopyBatchSolutionSlices(bs.h, N, 1, 3, past.ctypes.data_as(C.POINTER(C.c_double))) == -1
    with pytest.raises(ValueError):
        bs.set_step_selection(N - 1, 2, ndlqr.SOLN_STATE)
    assert bs.solve() == 0
    check(bs.solutions(), refs, probs, False, "after the refusals")
    bs.close()


# ------------------------------------------------------------------------------------------------ 3. residuals

@pytest.mark.parametrize("n,m,fam,N", UPLOAD_CASES)
def test_kkt_residuals_equal_the_host_padded_solver(ndlqr, oracle, n, m, fam, N):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    fl = family_flags(ndlqr, fam)
    bs, bp = new_solver(ndlqr, probs, fl), padded_solver(ndlqr, probs, fl)
    assert bs.solve() == 0 and bp.solve() == 0
    res, bn = bs.kkt_residuals()
    resp, bnp = bp.kkt_residuals()
    assert np.array_equal(res, resp) and np.array_equal(bn, bnp)  # (the tail adds exact zeros)
    assert (res <= 1e-9 * bn).all()
    # the residual vector: the caller's nvars, a prefix of the padded solver's, whose tail is exactly zero
    guard = np.full(BATCH * bs.nvars + 4, 7.0)
    r = bs.kkt_residual_vector(guard[: BATCH * bs.nvars].reshape(BATCH, bs.nvars))
    rp = bp.kkt_residual_vector()
    assert np.array_equal(r, rp[:, : bs.nvars]) and not rp[:, bs.nvars:].any()
    assert (guard[BATCH * bs.nvars:] == 7.0).all()
    bs.close(); bp.close()


# ------------------------------------------------------------------------------------------------ 4. adjoint, gradients

def guarded(shape, rows=1):
    """an array of `shape` with a guard row of sentinels behind it: (view, whole buffer)"""
    size = int(np.prod(shape))
    row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    buf = np.full(size + rows * row, 7.0)
    return buf[:size].reshape(shape), buf[size:]


GRAD_CASES = [(6, 3, None, 3), (6, 3, None, 7), (12, 4, None, 5), (12, 4, None, 33), (12, 4, None, 100), (7, 9, None, 9),
              (16, 4, None, 7), (16, 4, None, 33), (12, 4, GENERIC, 9)]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n,m,fam,N", GRAD_CASES)
def test_adjoint_and_gradients_equal_the_host_padded_solver(ndlqr, oracle, n, m, fam, N, strict):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    P = next_pow2(N)
    fl = family_flags(ndlqr, fam) | ((ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT) if strict else ndlqr.FLAG_KEEP_RECORDS)
    bs, bp = new_solver(ndlqr, probs, fl), padded_solver(ndlqr, probs, fl)
    assert bs.solve() == 0 and bp.solve() == 0
    g = np.random.default_rng(N).standard_normal((BATCH, bs.nvars))
    assert bs.solve_adjoint(g) == 0 and bp.solve_adjoint(pad_vector(g, probs[0])) == 0

    def same(a, b, what):
        if strict:
            assert np.array_equal(a, b), what
        else:
            assert rel(a, b) <= REL_TOL, (what, rel(a, b))

    w, wguard = guarded((BATCH, bs.nvars))
    bs.adjoint(w)
    wp = bp.adjoint()
    same(w, wp[:, : bs.nvars], "w")
    assert not wp[:, bs.nvars:].any() and (wguard == 7.0).all()
    for mask in (0, 0xFF):
        out, guards = {}, {}
        for i, name in enumerate(ndlqr.GRAD_NAMES):
            out[name], guards[name] = guarded(bs.gradient_shape(name, bool(mask & (1 << i))))
        bs.gradients(mask, out)
        gp = bp.gradients(mask)
        for name in ndlqr.GRAD_NAMES:
            assert (guards[name] == 7.0).all(), (name, mask)
            assert np.isfinite(out[name]).all()
            if name == "x0":
                same(out[name], gp[name], (name, mask))
                continue
            pref = gp[name][..., :N, :]
            same(out[name], pref, (name, mask))
            assert not gp[name][..., N:, :].any(), name  # (the tail of the padded solver's: exactly zero)
            if name in ("A", "B", "R", "r", "d"):
                assert not out[name][..., N - 1, :].any(), (name, mask)
    bs.close(); bp.close()


# ------------------------------------------------------------------------------------------------ 5. box constraints

def unconstrained_u(refs, n, m, N):
    return np.stack([split(z, n, m, N)[2] for z in refs])


def input_bounds_off_zero(refs, n, m, N):
    """[batch, N, m]: channel 0 boxed into [a, b] with 0 < a -- zero lies outside --, the other channels symmetric at
    half their mean |u|; every problem's own numbers"""
    u = unconstrained_u(refs, n, m, N)
    ulo, uhi = [], []
    for p in range(len(refs)):
        h = np.tile(0.5 * np.abs(u[p]).mean(axis=0), (N, 1))
        lo = -h.copy()
        lo[:, 0] = 0.25 * h[:, 0]
        ulo.append(lo); uhi.append(h)
    return np.stack(ulo), np.stack(uhi)


BOX_CASES = [(6, 3, None, 7), (12, 4, None, 5), (12, 4, None, 33), (7, 9, None, 9), (16, 4, None, 7), (12, 4, GENERIC, 9),
             (6, 3, None, 3), (12, 4, None, 100)]


def box_equal_padded(ndlqr, bs, bp, N, strict, it, st, itp, stp):
    assert np.array_equal(st, stp) and np.array_equal(it, itp), (it, itp, st, stp)
    mux, gx = guarded((BATCH, N, bs.n))
    muu, gu = guarded((BATCH, N, bs.m))
    bs.bound_multipliers(mux, muu)
    mpx, mpu = bp.bound_multipliers()
    assert (gx == 7.0).all() and (gu == 7.0).all()
    assert not mpx[:, N:].any() and not mpu[:, N - 1:].any()  # (the tail and u of knot N - 1 are never bounded)
    pairs = [(bs.box_residuals(), bp.box_residuals(), "residuals"), (mux, mpx[:, :N], "mu_x"), (muu, mpu[:, :N], "mu_u"),
             (bs.solutions(), bp.solutions()[:, : bs.nvars], "z"), (bs.box_penalties(), bp.box_penalties(), "rho")]
    for a, b, what in pairs:
        if strict:
            assert np.array_equal(a, b), what
        else:
            assert np.allclose(a, b, rtol=REL_TOL, atol=1e-300), what
    return mux, muu


def pad_bounds(a, P, fill):
    """bounds [batch, N, k] or [N, k] extended to horizon P with +-inf"""
    N = a.shape[-2]
    out = np.full(a.shape[:-2] + (P, a.shape[-1]), fill)
    out[..., :N, :] = a
    return out


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("n,m,fam,N", BOX_CASES)
def test_input_bounds_with_zero_outside_the_box(ndlqr, oracle, n, m, fam, N, strict, shared):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    P = next_pow2(N)
    ulo, uhi = input_bounds_off_zero(refs, n, m, N)
    if shared:  # one set for every problem: problem 0's
        ulo, uhi = ulo[0], uhi[0]
    fl = family_flags(ndlqr, fam) | ((ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT) if strict else 0)
    bs, bp = new_solver(ndlqr, probs, fl), padded_solver(ndlqr, probs, fl)
    bs.set_bounds(None, None, ulo, uhi)
    # (the host-padded solver: the same bounds on knots < N - 1, none behind them)
    plo, phi = pad_bounds(ulo, P, -np.inf), pad_bounds(uhi, P, np.inf)
    plo[..., N - 1:, :] = -np.inf; phi[..., N - 1:, :] = np.inf
    bp.set_bounds(None, None, plo, phi)
    rho = float(np.mean([p.R[: N - 1].mean() for p in probs]))
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    it, st = bs.solve_box(**kw)
    itp, stp = bp.solve_box(**kw)
    print("iterations", it.tolist())
    assert (st == 1).all(), (it, st)
    box_equal_padded(ndlqr, bs, bp, N, strict, it, st, itp, stp)
    sol = bs.solutions()
    assert np.isfinite(sol).all()
    for p, prob in enumerate(probs):
        lo, hi = (ulo, uhi) if shared else (ulo[p], uhi[p])
        u = split(sol[p], n, m, N)[2]
        assert (u <= hi[: N - 1]).all() and (u >= lo[: N - 1]).all()
        assert (u[:, 0] > 0).all()
        ub, _ = bvls_inputs(prob, lo, hi)
        assert rel(u, ub) <= 1e-6, (p, rel(u, ub))  # (the tolerance of test_gpu_box.py for the same comparison)
    bs.close(); bp.close()


def state_bounds_off_zero(probs, refs):
    """state bounds, feasible by construction (the trajectory of u = 0 lies strictly inside, as in test_gpu_box.py's
    state_box): symmetric at 0.7 of the largest unconstrained |x| of each state, widened to 1.5 |rollout| where that needs
    more; and, wherever the rollout of state 0 is positive, its lower bound raised to half the rollout: 0 < xlo there."""
    lo, hi = [], []
    for prob, z in zip(probs, refs):
        n, m, N = prob.n, prob.m, prob.N
        x = split(z, n, m, N)[1]
        roll = np.zeros_like(x)
        roll[0] = prob.x0
        for k in range(N - 1):
            roll[k + 1] = prob.A[k].reshape(n, n).T @ roll[k] + prob.d[k]
        h = np.maximum(np.tile(0.7 * np.abs(x[1:]).max(axis=0), (N, 1)), 1.5 * np.abs(roll))
        l = -h.copy()
        pos = roll[:, 0] > 0
        l[pos, 0] = 0.5 * roll[pos, 0]
        lo.append(l); hi.append(h)
    return np.stack(lo), np.stack(hi)


STATE_CASES = [(6, 3, None, 7), (12, 4, None, 5), (12, 4, None, 33), (7, 9, None, 9), (16, 4, None, 7), (12, 4, GENERIC, 9)]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("n,m,fam,N", STATE_CASES)
def test_state_bounds_with_zero_outside_the_box(ndlqr, oracle, n, m, fam, N, strict):
    probs, refs = problems(ndlqr, oracle, n, m, N)
    P = next_pow2(N)
    xlo, xhi = state_bounds_off_zero(probs, refs)
    assert (xlo[:, 1:] > 0).any()
    fl = family_flags(ndlqr, fam) | ((ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT) if strict else 0)
    bs, bp = new_solver(ndlqr, probs, fl), padded_solver(ndlqr, probs, fl)
    bs.set_bounds(xlo, xhi, None, None)
    bp.set_bounds(pad_bounds(xlo, P, -np.inf), pad_bounds(xhi, P, np.inf), None, None)
    rho = float(np.mean([p.Q.mean() for p in probs]))
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=8000)
    it, st = bs.solve_box(**kw)
    itp, stp = bp.solve_box(**kw)
    print("iterations", it.tolist())
    assert (st == 1).all(), (it, st)
    mux, muu = box_equal_padded(ndlqr, bs, bp, N, strict, it, st, itp, stp)
    sol = bs.solutions()
    inf = np.full((N, m), np.inf)
    for p, prob in enumerate(probs):
        cert = certificate(prob, sol[p], mux[p], muu[p], xlo[p], xhi[p], -inf, inf, 1e-6)
        assert cert["stationarity"] <= 1e-6 and cert["bounds"] <= 0 and cert["complementarity"] <= 1e-6, cert
    bs.close(); bp.close()


def test_adaptive_penalty_at_a_padded_horizon(ndlqr, oracle):
    n, m, N = 12, 4, 33
    probs, refs = problems(ndlqr, oracle, n, m, N)
    ulo, uhi = input_bounds_off_zero(refs, n, m, N)
    bs = new_solver(ndlqr, probs)
    bs.set_bounds(None, None, ulo, uhi)
    it, st = bs.solve_box(rho=10.0, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, adapt_every=25)
    print("iterations", it.tolist(), "penalties", bs.box_penalties().tolist())
    assert (st == 1).all(), (it, st)
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    inf = np.full((N, n), np.inf)
    for p, prob in enumerate(probs):
        cert = certificate(prob, sol[p], mux[p], muu[p], -inf, inf, ulo[p], uhi[p], 1e-6)
        assert cert["stationarity"] <= 1e-6 and cert["bounds"] <= 0 and cert["complementarity"] <= 1e-6, cert
    bs.close()


# ------------------------------------------------------------------------------------------------ 6. refusals

def last_error(ndlqr):
    return ndlqr.lib().ndlqr_hip_last_error().decode()


def refusal_calls(ndlqr, bs):
    """(name, the entry point the library names in its refusal, call) of every entry point that refuses at a padded
    horizon; each call returns the C return code or raises RuntimeError"""
    L = ndlqr.lib()
    n, m, N, B = bs.n, bs.m, bs.N, bs.batch
    g = np.ones((B, bs.nvars))
    five = (C.c_void_p * 5)()
    io = [C.POINTER(C.c_double)() for _ in range(4)]
    multi = (np.zeros((2, B, N, n)), np.zeros((2, B, N, m)), np.zeros((2, B, N, n)), np.zeros((2, B, n)))
    top = np.zeros(1 << 16)
    blocks = np.zeros(N * (2 * n + m))
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    return [
        ("refine", "ndlqr_hip_refine", lambda: bs.refine(1)),
        ("refine_adjoint", "ndlqr_hip_refine", lambda: bs.refine_adjoint(1)),
        ("box adjoint", "ndlqr_hip_solve_box_adjoint", lambda: bs.solve_box_adjoint(g, max_iter=50)),
        ("bound gradients", "ndlqr_hip_bound_gradients", lambda: bs.bound_gradients()),
        ("box adjoint residuals", "ndlqr_hip_download_box_adjoint_residuals", lambda: bs.box_adjoint_residuals()),
        ("polish", "ndlqr_hip_polish_box", lambda: bs.polish_box()),
        ("polished adjoint", "ndlqr_hip_solve_polished_adjoint", lambda: bs.solve_polished_adjoint(g)),
        ("polish codes", "ndlqr_hip_download_polish_codes", lambda: bs.polish_codes()),
        ("infeasibility on", "ndlqr_hip_set_box_infeasibility", lambda: bs.set_box_infeasibility(10)),
        ("infeasibility certificate", "ndlqr_hip_download_infeasibility_certificate", lambda: bs.infeasibility_certificate()),
        ("infeasibility measures", "ndlqr_hip_download_infeasibility_measures", lambda: bs.infeasibility_measures()),
        ("acceleration on", "ndlqr_hip_set_box_acceleration", lambda: bs.set_box_acceleration(4)),
        ("acceleration read-out", "ndlqr_hip_download_box_acceleration", lambda: bs.box_acceleration()),
        ("multi rhs", "ndlqr_hip_solve_multi_rhs", lambda: bs.solve_multi_rhs(*multi)),
        ("multi rhs slices", "ndlqr_hip_solve_multi_rhs_slices",
         lambda: bs.solve_multi_rhs(*multi, selection=(0, 1, ndlqr.SOLN_INPUT))),
        ("time shard top doubles", "ndlqr_hip_time_shard_top_doubles", lambda: min(bs.time_shard_top_doubles(2), 0)),
        ("time shard factor", "ndlqr_hip_time_shard_factor", lambda: bs.time_shard_factor(0, 2)),
        ("time shard export", "ndlqr_hip_time_shard_export", lambda: bs.time_shard_export(2, top.ctypes.data)),
        ("time shard import", "ndlqr_hip_time_shard_import", lambda: bs.time_shard_import(2, top.ctypes.data)),
        ("time shard finish", "ndlqr_hip_time_shard_finish", lambda: bs.time_shard_finish(0, 2)),
        ("factors", "ndlqr_hip_download_factors", lambda: L.ndlqr_CopyBatchFactors(
            bs.h, 0, dptr(np.zeros(4 * N * 8 * (2 * n + m) * n)))),
        ("device pointers", "ndlqr_hip_device_pointers", lambda: L.ndlqr_hip_device_pointers(bs.ctx, five)),
        ("staged io", "ndlqr_hip_staged_io", lambda: L.ndlqr_hip_staged_io(bs.ctx, *[C.byref(p) for p in io])),
        ("rhs blocks", "ndlqr_hip_download_rhs_blocks", lambda: L.ndlqr_hip_download_rhs_blocks(bs.ctx, 0, dptr(blocks))),
    ]


def outcome(call):
    try:
        ret = call()
    except RuntimeError as e:
        return "raised", str(e)
    if isinstance(ret, int) and ret != 0:
        return "code", ret
    return "ok", ret


def test_entry_points_that_refuse_a_padded_horizon(ndlqr, oracle):
    n, m = 12, 4
    probs, refs = problems(ndlqr, oracle, n, m, 5)
    bs = new_solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    u = unconstrained_u(refs, n, m, 5)
    hi = np.tile(0.5 * np.abs(u).mean(axis=(0, 1)), (5, 1))
    bs.set_bounds(None, None, -hi, hi)
    it, st = bs.solve_box(eps_abs=1e-8, eps_rel=1e-8)
    assert (st == 1).all()
    assert bs.solve() == 0
    previous = None
    for name, who, call in refusal_calls(ndlqr, bs):
        kind, what = outcome(call)
        assert kind in ("raised", "code"), (name, kind, what)
        if kind == "code":
            assert what == -1, (name, what)  # NDLQR_ERR_INVALID
        # the message is this call's: it opens with the entry point's name (no two consecutive calls share one, except
        # the two refinements, whose message is then the same) and names both horizons
        msg = last_error(ndlqr)
        assert msg.startswith(who + ": not available for a padded horizon (horizon 5 runs as 8 knots)"), (name, msg)
        assert who != previous or name == "refine_adjoint", name
        previous = who
    with pytest.raises(RuntimeError, match="horizon"):
        bs.factors(0)
    # switching the refused settings off stays possible, and the solver still solves
    bs.set_box_infeasibility(0)
    bs.set_box_acceleration(0)
    assert bs.solve() == 0
    check(bs.solutions(), refs, probs, False, "after the refusals")
    it, st = bs.solve_box(eps_abs=1e-8, eps_rel=1e-8)
    assert (st == 1).all()
    bs.close()


def test_the_same_entry_points_at_a_power_of_two(ndlqr, oracle):
    """N = 8: every one of them that eight knots allow succeeds -- refinement, the box adjoint and its read-outs, polish,
    its adjoint and its codes, the infeasibility and acceleration read-outs, the factor download, raw device pointers, the
    staged path, the solution blocks. Multiple right-hand sides and time sharding need 16 and 32 knots of their own accord
    (test_multi_rhs_and_time_sharding_at_the_next_power_of_two): at 8 they refuse, but not for the horizon."""
    n, m, N = 12, 4, 8
    probs = [synth(ndlqr, n, m, N, SEED0 + p) for p in range(BATCH)]
    refs = np.stack([oracle.solve(p, 1)[0][: p.nvars] for p in probs])
    u = unconstrained_u(refs, n, m, N)
    hi = np.tile(0.5 * np.abs(u).mean(axis=(0, 1)), (N, 1))
    g = np.random.default_rng(8).standard_normal((BATCH, probs[0].nvars))
    bs = new_solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    calls = {name: call for name, _, call in refusal_calls(ndlqr, bs)}
    ok = lambda name: outcome(calls[name])  # noqa: E731

    assert bs.solve() == 0 and bs.solve_adjoint(g) == 0
    assert ok("refine")[0] == "ok"
    assert bs.solve_adjoint(g) == 0
    assert ok("refine_adjoint")[0] == "ok"
    assert ok("rhs blocks")[0] == "ok"
    assert ok("infeasibility on")[0] == "ok" and ok("acceleration on")[0] == "ok"
    bs.set_bounds(None, None, -hi, hi)
    it, st = bs.solve_box(eps_abs=1e-8, eps_rel=1e-8)
    assert (st == 1).all(), (it, st)
    assert ok("infeasibility certificate")[0] == "ok" and ok("infeasibility measures")[0] == "ok"
    assert ok("acceleration read-out")[0] == "ok"
    assert ok("box adjoint")[0] == "ok"
    assert ok("bound gradients")[0] == "ok" and ok("box adjoint residuals")[0] == "ok"
    bs.set_box_infeasibility(0); bs.set_box_acceleration(0)
    it, st = bs.solve_box(eps_abs=1e-8, eps_rel=1e-8)
    assert ok("polish")[0] == "ok" and ok("polish codes")[0] == "ok"
    assert ok("polished adjoint")[0] == "ok"
    bs.close()

    bs = new_solver(ndlqr, probs, ndlqr.FLAG_KEEP_FACT)
    calls = {name: call for name, _, call in refusal_calls(ndlqr, bs)}
    assert bs.solve() == 0
    assert ok("factors")[0] == "ok" and bs.factors(0).size == N * 3 * (2 * n + m) * n
    assert ok("device pointers")[0] == "ok"
    for name in ("multi rhs", "multi rhs slices", "time shard top doubles", "time shard factor", "time shard export",
                 "time shard import", "time shard finish"):
        kind, what = ok(name)
        assert kind != "ok" and "padded horizon" not in last_error(ndlqr), (name, last_error(ndlqr))
    assert bs.solve() == 0
    check(bs.solutions(), refs, probs, False, "N = 8")
    bs.close()

    bs = new_solver(ndlqr, probs)
    calls = {name: call for name, _, call in refusal_calls(ndlqr, bs)}
    assert ok("staged io")[0] == "ok"
    bs.close()


def test_multi_rhs_and_time_sharding_at_the_next_power_of_two(ndlqr, oracle, monkeypatch):
    """The two refused families whose own preconditions eight knots do not meet, at the smallest shapes that do: multiple
    right-hand sides (compact records: 16 knots and the level-per-launch schedule) refuse at N = 9, which runs as 16, and
    succeed at 16; time sharding (chunks of 16 knots, here the suite's smallest sharded shape, 128 over two chunks)
    refuses at N = 100, which runs as 128, and succeeds at 128. The guard is not the only thing these calls meet."""
    monkeypatch.setenv("NDLQR_TREE", "0")
    n, m = 12, 4
    for N, refused in ((9, True), (16, False)):
        probs = [synth(ndlqr, n, m, N, SEED0 + p) for p in range(BATCH)]
        bs = new_solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
        assert bs.solve() == 0
        calls = {name: (who, call) for name, who, call in refusal_calls(ndlqr, bs)}
        for name in ("multi rhs", "multi rhs slices"):
            kind, what = outcome(calls[name][1])
            if refused:
                assert kind == "raised" and last_error(ndlqr).startswith(calls[name][0] + ": not available for a padded horizon")
            else:
                assert kind == "ok", (name, what)
                assert bs.schedule() == "reduced-compact-records"
                assert np.isfinite(what).all()
        bs.close()
    monkeypatch.delenv("NDLQR_TREE")
    n, m, G = 13, 4, 2
    for N, refused in ((100, True), (128, False)):
        solvers = [ndlqr.BatchSolver(n, m, N, 1) for _ in range(G)]
        for bs in solvers:
            bs.initialize_synthetic(SEED0)
        count = solvers[0].time_shard_top_doubles(G)
        if refused:
            assert count < 0 and last_error(ndlqr).startswith("ndlqr_hip_time_shard_top_doubles: not available for a padded")
            assert solvers[0].time_shard_factor(0, G) == -1
            assert last_error(ndlqr).startswith("ndlqr_hip_time_shard_factor: not available for a padded horizon")
        else:  # (the sequence of test_time_axis.py: factor, sum of the top slots, finish)
            assert count > 0
            bufs = []
            for g, bs in enumerate(solvers):
                assert bs.time_shard_factor(g, G) == 0
                bufs.append(np.zeros(count))
                assert bs.time_shard_export(G, bufs[-1].ctypes.data) == 0
            total = np.sum(bufs, axis=0)
            for g, bs in enumerate(solvers):
                assert bs.time_shard_import(G, total.ctypes.data) == 0
                assert bs.time_shard_finish(g, G) == 0
                assert bs.synchronize() == 0 and bs.cholesky_failures() == 0
        for bs in solvers:
            assert bs.solve() == 0
            bs.close()


# ------------------------------------------------------------------------------------------------ 7. torch
# Each case runs in a fresh process that initialises torch's device before the library's (as in test_gpu_gradients.py:
# torch ships its own HIP runtime, and the second of the two to start in a process may find no device).

def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_horizon as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def to_torch(torch, probs):
    n, m, N = probs[0].n, probs[0].m, probs[0].N
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)  # noqa: E731
    A = np.stack([p.A.reshape(N, n, n).transpose(0, 2, 1) for p in probs])
    B = np.stack([p.B.reshape(N, m, n).transpose(0, 2, 1) for p in probs])
    rest = [np.stack([getattr(p, k) for p in probs]) for k in ("Q", "R", "q", "r", "d", "x0")]
    return [t(A), t(B)] + [t(a) for a in rest]


def _case_lqr_solve(ndlqr, n, m, N):
    """lqr_solve at horizon N against the same call on the host-padded problems: the solution, and the gradients of a
    random linear loss of it on their [:N] prefixes; A, B, R, r, d of knot N - 1 get exactly zero"""
    import torch
    from rslqr_amd.autograd import lqr_solve
    from support import Oracle
    probs, refs = problems(ndlqr, Oracle(), n, m, N)
    P = next_pow2(N)
    nvars = probs[0].nvars
    wgt = torch.tensor(np.random.default_rng(N).standard_normal((BATCH, nvars)), dtype=torch.float64, device="cuda")
    grads = []
    for ps in (probs, [pad_problem(p) for p in probs]):
        args = to_torch(torch, ps)
        z = lqr_solve(*args)
        if ps is probs:
            assert z.shape == (BATCH, nvars)
            for p in range(BATCH):
                assert rel(z[p].detach().cpu().numpy(), refs[p]) <= REL_TOL
        (z[:, :nvars] * wgt).sum().backward()
        grads.append([a.grad.detach().cpu().numpy() for a in args])
    for name, a, b in zip(ARGS, grads[0], grads[1]):
        if name == "x0":
            assert rel(a, b) <= REL_TOL, name
            continue
        assert a.shape[1] == N and b.shape[1] == P
        assert rel(a, b[:, :N]) <= REL_TOL, (name, rel(a, b[:, :N]))
        assert not b[:, N:].any(), name
        if name in ("A", "B", "R", "r", "d"):
            assert not a[:, N - 1].any(), name


def _case_box_backward(ndlqr):
    """lqr_solve_box at a padded horizon: the forward works, the backward (the box adjoint, not carried through) raises
    the library's message"""
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    from support import Oracle
    n, m, N = 6, 3, 5
    probs, refs = problems(ndlqr, Oracle(), n, m, N)
    u = unconstrained_u(refs, n, m, N)
    hi_np = np.tile(0.5 * np.abs(u).mean(axis=(0, 1)), (N, 1))
    hi = torch.tensor(hi_np, dtype=torch.float64, device="cuda")
    z = lqr_solve_box(*to_torch(torch, probs), ulo=-hi, uhi=hi)
    assert z.shape == (BATCH, probs[0].nvars) and bool(torch.isfinite(z).all())
    for p, prob in enumerate(probs):
        un = split(z[p].detach().cpu().numpy(), n, m, N)[2]
        assert (np.abs(un) <= hi_np[: N - 1]).all()
        ub, _ = bvls_inputs(prob, -hi_np, hi_np)
        assert rel(un, ub) <= 1e-4, rel(un, ub)  # (the library's default eps of 1e-6)
    try:
        z.sum().backward()
    except RuntimeError as e:
        assert "horizon" in str(e), str(e)
    else:
        raise AssertionError("the backward of lqr_solve_box did not raise at a padded horizon")


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 12)])
def test_lqr_solve_at_any_horizon(n, m, N):
    _run_case("_case_lqr_solve", n, m, N)


def test_lqr_solve_box_backward_raises_the_library_message():
    _run_case("_case_box_backward")
