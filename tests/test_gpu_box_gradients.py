"""Gradients through the box-constrained solve (ndlqr_SolveBatchBoxAdjoint, ndlqr_BatchBoundGradients,
rslqr_amd.autograd.lqr_solve_box) on the device: strict mode against the numpy restatement of the adjoint iteration
driving the oracle (bit for bit), fast mode on every kept-factorisation schedule against the direct solve of the
active-set adjoint system (box_grad_support.py), batch sums, the state rules and torch."""
import numpy as np
import pytest

from box_grad_support import active_adjoint, active_codes, adjoint_admm_reference, adjoint_problem, bound_grads
from support import Problem, kkt_residual_ld
from test_gpu_box import SCHEDULE_CASES, input_bounded_states, input_box, solver, stack, state_box, synth
from test_gpu_gradients import ARGS, grad_formula

pytestmark = pytest.mark.gpu

BOUNDS = ("xlo", "xhi", "ulo", "uhi")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def codes_of(bs, sol, p, xlo, xhi, ulo, uhi):
    from types import SimpleNamespace
    prob = SimpleNamespace(n=bs.n, m=bs.m, N=bs.N)
    pick = lambda a: None if a is None else a[p]
    return active_codes(prob, sol[p], pick(xlo), pick(xhi), pick(ulo), pick(uhi))


def adjoint_residual(prob, g, w, nu):
    """||K w + E_A' nu - g||_inf relative to max(|g|, |w|, |nu|), in extended precision"""
    n = prob.n
    ap = adjoint_problem(prob, g)
    p2 = Problem(prob.n, prob.m, prob.N, ap.A, ap.B, ap.Q, ap.R, ap.q + nu[:, :n], ap.r + nu[:, n:], ap.d, ap.x0)
    r = kkt_residual_ld(p2, w)
    scale = max(1.0, float(np.abs(g).max()), float(np.abs(w).max()), float(np.abs(nu).max()))
    return float(max(np.abs(part).max() for part in r)) / scale


# ------------------------------------------------------------------------------------------------ 1. strict, bit for bit

@pytest.mark.parametrize("iters", [1, 3, 40])
def test_strict_mode_is_the_numpy_restatement_bit_for_bit(ndlqr, oracle, iters):
    n, m, N, batch = 12, 4, 16, 2
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    rho, alpha = 0.37, 1.6
    bs = solver(ndlqr, probs, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, alpha=alpha, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000)
    assert (st == 1).all(), (it, st)
    sol = bs.solutions().copy()
    g = np.random.default_rng(7).standard_normal((batch, bs.nvars))
    eps = 1e-300 if iters < 40 else 1e-7
    ait, ast = bs.solve_box_adjoint(g, alpha=alpha, eps_abs=eps, eps_rel=eps, max_iter=iters)
    w = bs.adjoint()
    grads = bs.gradients()
    bg = bs.bound_gradients()
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    for p, prob in enumerate(probs):
        codes = codes_of(bs, sol, p, xlo, xhi, ulo, uhi)
        assert (codes >= 2).any() and (codes == 1).any()
        wr, nur, rit, rst = adjoint_admm_reference(prob, solve, codes, g[p], rho, alpha, eps, eps, iters)
        assert ait[p] == rit and ast[p] == rst, (p, ait[p], rit, ast[p], rst)
        assert np.array_equal(w[p], wr), p
        ref = grad_formula(prob, sol[p], wr)
        for k in ARGS:
            assert np.array_equal(grads[k][p], ref[k]), (p, k)
        bref = bound_grads(codes, nur, n)
        for k in BOUNDS:
            assert np.array_equal(bg[k][p], bref[k]), (p, k)
    bs.close()


# ------------------------------------------------------------------------------------------------ 2. every schedule

@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6] or c[4], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
def test_every_schedule_against_the_active_set_adjoint(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 1500 + p) for p in range(batch)]
    fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "fact": ndlqr.FLAG_KEEP_FACT, "none": 0,
          "strict": ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT}[flags]
    bs = solver(ndlqr, probs, fl)
    ulo, uhi = input_box(oracle, probs, 0.5)
    rho_r = float(np.mean([p.R.mean() for p in probs]))
    rho = float(np.mean([p.Q.mean() for p in probs])) * (3.0 if n > 128 else 1.0)
    if N >= 4:
        xlo, xhi = state_box(oracle, probs, 0.9, input_bounded_states(bs, ulo, uhi, rho_r))
    else:
        xlo, xhi, rho = None, None, rho_r
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25)
    assert want is None or bs.schedule() == want, bs.schedule()
    assert (st == 1).all(), (it, st)
    sol = bs.solutions().copy()
    g = np.random.default_rng(n + N).standard_normal((batch, bs.nvars))
    f0 = bs.factor_count()
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25)
    print("forward iterations: max %d, median %d; backward: max %d, median %d"
          % (int(it.max()), int(np.median(it)), int(ait.max()), int(np.median(ait))))
    # (one of the 160 problems of the first case, the one whose forward needs the most iterations, does not reach 1e-10
    # within 20000: the problems checked below do, and all but at most 1 % of the batch)
    checked = sorted({0, batch - 1})
    assert (ast[checked] == 1).all() and (ast != 1).sum() <= batch // 100, (ait, ast)
    assert bs.factor_count() == f0
    w = bs.adjoint()
    grads = bs.gradients()
    bg = bs.bound_gradients()
    for p in checked:
        prob = probs[p]
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
    bs.close()


# ------------------------------------------------------------------------------------------------ 3. batch sums

@pytest.mark.parametrize("n,m,N,batch,per_problem", [(12, 4, 64, 40, True), (12, 4, 256, 100, False), (6, 3, 16, 1, False)])
def test_batch_sums(ndlqr, oracle, n, m, N, batch, per_problem):
    probs = [synth(ndlqr, n, m, N, 300 + p) for p in range(batch)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    ulo, uhi = input_box(oracle, probs, 0.5)
    rho = float(np.mean([p.R.mean() for p in probs]))
    if per_problem:
        xlo, xhi = state_box(oracle, probs, 0.9, input_bounded_states(bs, ulo, uhi, rho))
        bs.set_bounds(xlo, xhi, ulo, uhi)
        rho = float(np.mean([p.Q.mean() for p in probs]))
    else:
        bs.set_bounds(None, None, ulo[0], uhi[0])
    it, st = bs.solve_box(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000, check_every=25)
    assert (st == 1).all()
    g = np.random.default_rng(5).standard_normal((batch, bs.nvars))
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000, check_every=25)
    assert (ast == 1).all()
    per = bs.bound_gradients()
    s1 = bs.bound_gradients(summed=True)
    s2 = bs.bound_gradients(summed=True)
    assert any(np.abs(per[k]).max() > 0 for k in BOUNDS)
    for k in BOUNDS:
        assert s1[k].shape == per[k].shape[1:]
        assert np.array_equal(s1[k], s2[k]), k
        ref = per[k].sum(axis=0)
        assert np.abs(s1[k] - ref).max() <= 1e-12 * max(1.0, np.abs(per[k]).sum(axis=0).max()), k
    # partial outputs and device memory
    dev = ndlqr.DeviceArray((N, m))
    out = bs.bound_gradients(summed=True, out={"uhi": dev})
    assert set(out) == {"uhi"} and np.array_equal(dev.get(), s1["uhi"])
    bs.close()


# ------------------------------------------------------------------------------------------------ 4. state rules

def _forward(ndlqr, probs, ulo, uhi, xlo, xhi, flags):
    bs = solver(ndlqr, probs, flags)
    bs.set_bounds(xlo, xhi, ulo, uhi)
    return bs


def test_state_rules(ndlqr, oracle):
    n, m, N, batch = 12, 4, 16, 3
    probs = [synth(ndlqr, n, m, N, 400 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    rho = 0.37
    flags = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT
    kw = dict(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000)
    g = np.random.default_rng(4).standard_normal((batch, (2 * n + m) * N - m))
    a = _forward(ndlqr, probs, ulo, uhi, xlo, xhi, flags)
    b = _forward(ndlqr, probs, ulo, uhi, xlo, xhi, flags)
    # refused before any constrained solve, and after a plain one
    with pytest.raises(RuntimeError):
        a.solve_box_adjoint(g)
    assert a.solve() == 0
    with pytest.raises(RuntimeError):
        a.solve_box_adjoint(g)
    for s in (a, b):
        it, st = s.solve_box(**kw)
        assert (st == 1).all()
    sol, mu = a.solutions().copy(), a.bound_multipliers()
    f0 = a.factor_count()
    ait, ast = a.solve_box_adjoint(g, max_iter=4000)
    assert (ast == 1).all()
    # nothing of the forward changed
    assert a.factor_count() == f0
    assert np.array_equal(a.solutions(), sol)
    mu2 = a.bound_multipliers()
    assert np.array_equal(mu[0], mu2[0]) and np.array_equal(mu[1], mu2[1])
    # the plain adjoint and re-solves still refuse; the box adjoint's w is what the getters read
    assert a.solve_adjoint(g) != 0
    assert a.solve_rhs_only() != 0
    w = a.adjoint()
    a.gradients()
    a.bound_gradients()
    # a second box adjoint is the same, bit for bit
    a.solve_box_adjoint(g, max_iter=4000)
    assert np.array_equal(a.adjoint(), w)
    # a warm-started forward after the backward is the one without it, bit for bit, and factors nothing
    x0 = np.stack([0.8 * p.x0 for p in probs])
    for s in (a, b):
        s.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
        it, st = s.solve_box(warm_start=True, **kw)
        assert (st == 1).all()
    assert a.factor_count() == f0
    assert np.array_equal(a.solutions(), b.solutions())
    ma, mb = a.bound_multipliers(), b.bound_multipliers()
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    # a later solve invalidates the box adjoint's outputs
    with pytest.raises(RuntimeError):
        a.adjoint()
    with pytest.raises(RuntimeError):
        a.bound_gradients()
    a.solve_box_adjoint(g, max_iter=4000)
    # new bounds: refused until the next constrained solve
    a.set_bounds(xlo, xhi, ulo, uhi)
    with pytest.raises(RuntimeError):
        a.solve_box_adjoint(g)
    a.solve_box(**kw)
    a.solve_box_adjoint(g, max_iter=4000)
    # new inputs: refused
    a.initialize_flat(*stack(probs))
    with pytest.raises(RuntimeError):
        a.solve_box_adjoint(g)
    # a plain solve + plain adjoint: the bound gradients refuse (no box adjoint of that solution)
    assert a.solve() == 0
    assert a.solve_adjoint(g) == 0
    with pytest.raises(RuntimeError):
        a.bound_gradients()
    with pytest.raises(RuntimeError):
        a.solve_box_adjoint(g)
    a.close()
    b.close()


def test_bad_settings_and_non_finite_forward(ndlqr, oracle):
    n, m, N, batch = 6, 3, 16, 3
    probs = [synth(ndlqr, n, m, N, 500 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    probs[1].q[3, 0] = np.nan
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    bs.set_bounds(None, None, ulo, uhi)
    it, st = bs.solve_box(rho=1.0, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000)
    assert st[1] == 3 and st[0] == 1 and st[2] == 1, st
    g = np.random.default_rng(1).standard_normal((batch, bs.nvars))
    for bad in (dict(alpha=2.5), dict(eps_abs=-1.0), dict(max_iter=-1)):
        with pytest.raises(RuntimeError):
            bs.solve_box_adjoint(g, **bad)
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000)
    assert ast[1] == 3 and ait[1] == 0 and ast[0] == 1 and ast[2] == 1, (ait, ast)
    # too few iterations: status 2
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-14, eps_rel=1e-14, max_iter=2)
    assert (ast[[0, 2]] == 2).all() and (ait[[0, 2]] == 2).all(), (ait, ast)
    bs.close()


# ------------------------------------------------------------------------------------------------ 5. no active bounds

@pytest.mark.parametrize("strict", [False, True])
def test_no_active_bounds_is_the_plain_adjoint(ndlqr, oracle, strict):
    n, m, N, batch = 12, 4, 64, 3
    probs = [synth(ndlqr, n, m, N, 600 + p) for p in range(batch)]
    fl = (ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT) if strict else ndlqr.FLAG_KEEP_RECORDS
    bs = solver(ndlqr, probs, fl)
    assert bs.solve() == 0
    g = np.random.default_rng(2).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    w0, g0 = bs.adjoint().copy(), bs.gradients()
    ulo, uhi = input_box(oracle, probs, 100.0)
    xlo, xhi = state_box(oracle, probs, 100.0)
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=0.5, eps_abs=1e-11, eps_rel=1e-11, max_iter=4000)
    assert (st == 1).all()
    ait, ast = bs.solve_box_adjoint(g, eps_abs=1e-11, eps_rel=1e-11, max_iter=4000)
    assert (ast == 1).all()
    assert rel(bs.adjoint(), w0) <= 1e-7
    gr = bs.gradients()
    for k in ARGS:
        assert rel(gr[k], g0[k]) <= 1e-7, k
    bg = bs.bound_gradients()
    for k in BOUNDS:
        assert not bg[k].any(), k
    bs.close()


# ------------------------------------------------------------------------------------------------ 6. torch
# Each case runs in a fresh process that initialises torch's device first (test_gpu_gradients._run_case).

def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_box_gradients as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("bounds", ["shared", "per_problem", "mixed"])
def test_torch_against_dense_reference(bounds):
    """lqr_solve_box's gradients in all twelve tensors against the dense active-set KKT system assembled in torch and
    solved by torch.linalg.solve with autograd (the active set from the forward)."""
    _run_case("_case_dense_reference", bounds)


def test_torch_backwards_in_reverse_order():
    _run_case("_case_backwards_in_reverse_order")


def test_torch_gradcheck():
    _run_case("_case_gradcheck")


def test_torch_refusals_and_non_convergence():
    _run_case("_case_refusals")


def _torch_problem(ndlqr, n, m, N, batch, seed):
    from test_gpu_gradients import _torch_problem as tp
    return tp(ndlqr, n, m, N, batch, seed)


def _torch_bounds(t, n, m, N, batch, mode, frac_u=0.5, frac_x=0.8):
    """bounds from the unconstrained solution: inputs at frac_u of the mean |u| per channel, states at frac_x of the
    largest |x| (widened for feasibility along u = 0 as test_gpu_box.state_box); shared = the first problem's"""
    import torch
    from test_gpu_gradients import _dense_solve
    with torch.no_grad():
        z = _dense_solve({k: v.detach() for k, v in t.items()}, n, m, N, batch)
    zb = 2 * n + m
    Z = torch.nn.functional.pad(z, (0, m)).reshape(batch, N, zb)
    x, u = Z[:, :, n:2 * n], Z[:, : N - 1, 2 * n:]
    uh = (frac_u * u.abs().mean(dim=1, keepdim=True)).expand(batch, N, m).clone()
    xh = (frac_x * x[:, 1:].abs().amax(dim=1, keepdim=True)).expand(batch, N, n).clone()
    with torch.no_grad():  # widened where the trajectory of u = 0 (inside every input box) needs more: feasible
        A, d, x0 = t["A"].detach(), t["d"].detach(), t["x0"].detach()
        roll = [x0]
        for k in range(N - 1):
            roll.append(torch.einsum("bij,bj->bi", A[:, k], roll[-1]) + d[:, k])
        xh = torch.maximum(xh, 1.5 * torch.stack(roll, dim=1).abs())
    out = {"xlo": -xh, "xhi": xh, "ulo": -uh, "uhi": uh}
    if mode == "shared":  # (the widest state box of the batch: feasible for every problem)
        out = {"xlo": -xh.amax(0), "xhi": xh.amax(0), "ulo": -uh[0], "uhi": uh[0]}
    elif mode == "mixed":
        out["ulo"], out["uhi"] = out["ulo"][0], out["uhi"][0]
    return {k: v.contiguous().requires_grad_(True) for k, v in out.items()}


def _dense_box_solve(t, bnd, z_fwd, n, m, N, batch):
    """z* [batch, nvars] of the equality-constrained KKT system on the active set of z_fwd, assembled in torch and solved
    by torch.linalg.solve (differentiable in the twelve tensors: the bounds enter as the right-hand side c_A)"""
    import torch
    zb = 2 * n + m
    nv = zb * N - m
    zs = []
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    for p in range(batch):
        get = lambda k: t[k] if t[k].dim() == {"A": 3, "B": 3, "Q": 2, "R": 2, "q": 2, "r": 2, "d": 2, "x0": 1}[k] else t[k][p]
        getb = lambda k: bnd[k] if bnd[k].dim() == 2 else bnd[k][p]
        A, B, Q, R, q, r, d, x0 = [get(k) for k in ARGS]
        K = torch.zeros((nv, nv), dtype=torch.float64, device="cuda")
        b = torch.zeros(nv, dtype=torch.float64, device="cuda")
        K[0:n, n:2 * n] = -eye
        K[n:2 * n, 0:n] = -eye
        b[0:n] = -x0
        for k in range(N):
            lo, xo, uo = k * zb, k * zb + n, k * zb + 2 * n
            K[xo:xo + n, xo:xo + n] = torch.diag(Q[k])
            b[xo:xo + n] = -q[k]
            if k == N - 1:
                break
            l1, x1 = (k + 1) * zb, (k + 1) * zb + n
            K[uo:uo + m, uo:uo + m] = torch.diag(R[k])
            b[uo:uo + m] = -r[k]
            K[l1:l1 + n, xo:xo + n] = A[k]
            K[xo:xo + n, l1:l1 + n] = A[k].T
            K[l1:l1 + n, uo:uo + m] = B[k]
            K[uo:uo + m, l1:l1 + n] = B[k].T
            K[l1:l1 + n, x1:x1 + n] = -eye
            K[x1:x1 + n, l1:l1 + n] = -eye
            b[l1:l1 + n] = -d[k]
        rows, vals = [], []
        zp = z_fwd[p]
        for k in range(N):
            for j in range(n + m):
                if j < n and k == 0 or j >= n and k == N - 1:
                    continue
                idx = k * zb + n + j
                name, jj = ("x", j) if j < n else ("u", j - n)
                for side in ("hi", "lo"):
                    c = getb(name + side)[k, jj]
                    if float(zp[idx]) == float(c):
                        rows.append(idx)
                        vals.append(c)
                        break
        na = len(rows)
        KK = torch.zeros((nv + na, nv + na), dtype=torch.float64, device="cuda")
        KK[:nv, :nv] = K
        for i, idx in enumerate(rows):
            KK[nv + i, idx] = 1.0
            KK[idx, nv + i] = 1.0
        rhs = torch.cat([b, torch.stack(vals)]) if na else b
        zs.append(torch.linalg.solve(KK, rhs)[:nv])
    return torch.stack(zs)


def _grads12(fn, leaves, gz):
    for v in leaves.values():
        v.grad = None
    z = fn()
    (z * gz).sum().backward()
    return z.detach(), {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in leaves.items()}


def _case_dense_reference(ndlqr, mode):
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    n, m, N, batch = 6, 3, 16, 3
    t = _torch_problem(ndlqr, n, m, N, batch, 2000)
    bnd = _torch_bounds(t, n, m, N, batch, mode)
    leaves = dict(t, **bnd)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    kw = dict(rho=1.0, eps_abs=1e-11, eps_rel=1e-11, max_iter=20000)
    args = [t[k] for k in ARGS] + [bnd[k] for k in BOUNDS]
    z, got = _grads12(lambda: lqr_solve_box(*args, **kw), leaves, gz)
    zr, ref = _grads12(lambda: _dense_box_solve(t, bnd, z, n, m, N, batch), leaves, gz)
    assert rel(z.cpu().numpy(), zr.cpu().numpy()) <= 1e-8
    active = 0
    for k in ARGS + BOUNDS:
        assert got[k].shape == leaves[k].shape, k
        gr = ref[k] if ref[k] is not None else torch.zeros_like(got[k])
        assert rel(got[k].cpu().numpy(), gr.cpu().numpy()) <= 1e-6, (k, rel(got[k].cpu().numpy(), gr.cpu().numpy()))
        if k in BOUNDS:
            active += int((gr != 0).sum())
    assert active > 0


def _case_backwards_in_reverse_order(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve, lqr_solve_box
    n, m, N, batch = 6, 3, 16, 2
    kw = dict(rho=1.0, eps_abs=1e-11, eps_rel=1e-11, max_iter=20000)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    cases = []
    for seed in (2100, 2200):
        t = _torch_problem(ndlqr, n, m, N, batch, seed)
        bnd = _torch_bounds(t, n, m, N, batch, "per_problem")
        leaves = dict(t, **bnd)
        args = [t[k] for k in ARGS] + [bnd[k] for k in BOUNDS]
        _, ref = _grads12(lambda: lqr_solve_box(*args, **kw), leaves, gz)
        cases.append((leaves, args, ref))
    for leaves, _, _ in cases:
        for v in leaves.values():
            v.grad = None
    z1 = lqr_solve_box(*cases[0][1], **kw)
    z2 = lqr_solve_box(*cases[1][1], **kw)  # (same shape: the same cached solver)
    z3 = lqr_solve(*cases[0][1][:8])         # (a solver of its own: lqr_solve's cache)
    (z2 * gz).sum().backward()
    (z1 * gz).sum().backward()
    (z3 * 0).sum().backward()
    for leaves, _, ref in cases:
        for k in ARGS + BOUNDS:
            assert rel(leaves[k].grad.cpu().numpy(), ref[k].cpu().numpy()) <= 1e-9, k


def _case_gradcheck(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    n, m, N, batch = 3, 2, 8, 2
    t = _torch_problem(ndlqr, n, m, N, batch, 2300)
    bnd = _torch_bounds(t, n, m, N, batch, "per_problem", frac_u=0.5, frac_x=50.0)  # inputs cut, states far away
    fn = lambda *a: lqr_solve_box(*a, rho=1.0, eps_abs=1e-12, eps_rel=1e-12, max_iter=50000)
    args = tuple(t[k] for k in ARGS) + tuple(bnd[k] for k in BOUNDS)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def _case_refusals(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    n, m, N, batch = 3, 2, 8, 2
    t = {k: v.detach() for k, v in _torch_problem(ndlqr, n, m, N, batch, 2400).items()}
    bnd = {k: v.detach() for k, v in _torch_bounds(t, n, m, N, batch, "per_problem").items()}
    args = [t[k] for k in ARGS]
    with pytest.raises(ValueError):
        lqr_solve_box(*args)  # no bounds
    with pytest.raises(TypeError):
        lqr_solve_box(*args, ulo=bnd["ulo"].float())
    with pytest.raises(ValueError):
        lqr_solve_box(*args, ulo=bnd["ulo"].cpu())
    with pytest.raises(ValueError):
        lqr_solve_box(*args, ulo=bnd["ulo"][:, :4])
    with pytest.raises(ValueError):
        lqr_solve_box(*args, ulo=bnd["uhi"], uhi=bnd["ulo"] - 1.0)  # lo > hi
    with pytest.raises(RuntimeError, match="did not converge"):
        lqr_solve_box(*args, ulo=bnd["ulo"], uhi=bnd["uhi"], max_iter=1)
    # a backward after another forward on the cached solver redoes this node's forward
    tt = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    z = lqr_solve_box(*[tt[k] for k in ARGS], ulo=bnd["ulo"], uhi=bnd["uhi"], rho=1.0, eps_abs=1e-9, eps_rel=1e-9,
                      max_iter=20000)
    from rslqr_amd import autograd as AG
    lqr_solve_box(*[t[k] for k in ARGS], ulo=bnd["ulo"] * 0.5, uhi=bnd["uhi"] * 0.5, rho=1.0)
    assert all(v[1] is not None for v in AG._box_cache.values())
    z.sum().backward()
    assert tt["A"].grad is not None
