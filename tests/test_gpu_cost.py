"""Dense cost matrices and cross terms by reduction on the device (ndlqr_InitializeBatchFlatDense; DESIGN.md section
3.16), against cost_support.py: the longdouble restatement of the reduction and the refined solution of the dense KKT
system. Families: cond(Q'), cond(R) = 1e3 (moderate) and 1e6 (hard). Shapes: (6,3), (12,4), (7,9) (m > n), (20,5) (beyond
a 16-lane row, tiled pack path), (32,8); horizons 2 (one dynamics knot), 5 (padded), 8, 16; batch 3.

Bars. Reduction read-out, per array and entry: 8 x the float64 numpy restatement's own largest error against the
longdouble one on the same problem (another operation order, FMA), at least 16 eps of the array's largest entry.
Solutions, rhs-only re-solves and adjoints, per field (max-abs difference over max-abs of the field): moderate family
1e-9, the project's parity contract; hard family 10 x the error of the same solver given the host-reduced problem through
initialize_flat and mapped back in numpy (the margin tools/fuzz_parity.py uses for ill-conditioned draws)."""
import ctypes as C

import numpy as np
import pytest

import cost_support as cs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
EPS = np.finfo(float).eps
CASES = [(n, m, N) for (n, m) in cs.SHAPES for N in cs.HORIZONS]
RED_NAMES = ("L", "LR", "G", "At", "Bt", "qt", "rt", "dt", "x0t")


def flag_modes(ndlqr):
    return [0, ndlqr.FLAG_KEEP_RECORDS, ndlqr.FLAG_GENERIC, ndlqr.FLAG_STRICT_FP]


def dense_solver(ndlqr, probs, flags=0, drop_H=False):
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    A, B, Q, H, R, q, r, d, x0 = cs.flat(probs)
    bs.initialize_flat_dense(A, B, Q, None if drop_H else H, R, q, r, d, x0)
    assert bs.cost_is_dense()
    return bs


def errors(Z, ref, n, m, N):
    """largest per-field error over the batch"""
    return np.max([cs.field_errors(z, zr, n, m, N) for z, zr in zip(Z, ref)], axis=0)


def yardstick(ndlqr, probs, ref, flags, rhs=None, adjoint=None):
    """Per-field errors of the same solver on the HOST-reduced problems (initialize_flat; float64 numpy reduction), mapped
    back in numpy. rhs: (q, r, d, x0) lists for an rhs-only re-solve; adjoint: g [batch, nvars]."""
    n, m, N = cs.dims(probs[0])
    reds = [cs.reduce(p) for p in probs]
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat(*cs.reduced_flat_diag(reds))
    assert bs.solve() == 0
    if rhs is not None:
        reds2 = [cs.reduce(dict(p, q=q, r=r, d=d, x0=x0)) for p, (q, r, d, x0) in zip(probs, rhs)]
        _, _, _, _, qt, rt, dt, x0t = cs.reduced_flat_diag(reds2)
        bs.set_rhs_flat(qt, rt, dt, x0t)
        assert bs.solve_rhs_only() == 0
    if adjoint is not None:
        assert bs.solve_adjoint(np.stack([cs.apply_St(r, g) for r, g in zip(reds, adjoint)])) == 0
        Zt = bs.adjoint()
    else:
        Zt = bs.solutions()
    bs.close()
    return errors(np.stack([cs.apply_S(r, zt) for r, zt in zip(reds, Zt)]), ref, n, m, N)


def check(ndlqr, name, got, probs, ref, flags, what, **kw):
    """test 2's bars for `got` [batch, nvars] against `ref`"""
    n, m, N = cs.dims(probs[0])
    err = errors(got, ref, n, m, N)
    if name == "moderate":
        print(what, (n, m, N), "flags", flags, "moderate: device", err)
        assert (err <= REL_TOL).all(), (what, flags, err)
    else:
        yard = yardstick(ndlqr, probs, ref, flags, **kw)
        print(what, (n, m, N), "flags", flags, "hard: device", err, "host-reduced", yard)
        assert (err <= 10 * yard).all(), (what, flags, err, yard)


# ---------------------------------------------------------------------------- 1: the reduction, entry by entry
@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", CASES)
def test_reduction_per_entry(ndlqr, n, m, N, name):
    fam = cs.family(n, m, N, name)
    exact = cs.reduction_flat([cs.reduce(p, np.longdouble) for p in fam["probs"]])
    f64 = cs.reduction_flat([cs.reduce(p, np.float64) for p in fam["probs"]])
    bs = dense_solver(ndlqr, fam["probs"])
    got = bs.cost_reduction()
    bs.close()
    for k in RED_NAMES:
        own = float(np.abs(f64[k] - exact[k]).max())
        bar = max(8 * own, 16 * EPS * float(np.abs(exact[k]).max()))
        err = float(np.abs(got[k] - exact[k]).max())
        print("reduction", (n, m, N), name, k, "device %.3e numpy %.3e ratio to bar %.3f" % (err, own, err / bar))
        assert got[k].shape == exact[k].shape and np.isfinite(got[k]).all()
        assert err <= bar, (k, err, bar)


# ---------------------------------------------------------------------------- 2: solutions per field, every flag mode
@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", CASES)
def test_solutions_per_field(ndlqr, n, m, N, name):
    fam = cs.family(n, m, N, name)
    for flags in flag_modes(ndlqr):
        bs = dense_solver(ndlqr, fam["probs"], flags)
        assert bs.solve() == 0 and bs.cholesky_failures() == 0
        Z = bs.solutions()
        one = bs.solution(1)
        assert bs.solve_ms() > 0
        bs.close()
        assert Z.shape == (cs.BATCH, (2 * n + m) * N - m) and np.array_equal(one, Z[1])
        check(ndlqr, name, Z, fam["probs"], fam["z"], flags, "solution")


def test_async_and_device_delivery(ndlqr):
    n, m, N = 12, 4, 5
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solver(ndlqr, fam["probs"])
    assert bs.solve_async() == 0 and bs.synchronize() == 0
    Z = bs.solutions()
    dev = ndlqr.DeviceArray((cs.BATCH, bs.nvars))
    bs.solutions_to_device(dev.ptr)
    assert bs.synchronize() == 0
    assert np.array_equal(dev.get(), Z)
    check(ndlqr, "moderate", Z, fam["probs"], fam["z"], 0, "async")
    # the inputs from device memory: the same bits
    arrs = cs.flat(fam["probs"])
    devs = [ndlqr.DeviceArray(a.shape).set(a) for a in arrs]
    bs.initialize_flat_dense(*devs)
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), Z)
    bs.close()


# ---------------------------------------------------------------------------- 3: degenerate input
@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8), (7, 9, 2), (20, 5, 16), (32, 8, 8)])
def test_diagonal_costs_match_the_diagonal_path(ndlqr, n, m, N):
    probs, Qd, Rd = zip(*[cs.diagonal_problem(n, m, N, 40 + i) for i in range(cs.BATCH)])
    A, B, _, _, _, q, r, d, x0 = cs.flat(probs)
    plain = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    plain.initialize_flat(A, B, np.stack(Qd), np.stack(Rd), q, r, d, x0)
    assert plain.solve() == 0
    Zp = plain.solutions()
    plain.close()
    bs = dense_solver(ndlqr, probs)
    assert bs.solve() == 0
    Z0 = bs.solutions()
    bs.close()
    err = errors(Z0, Zp, n, m, N)
    print("diagonal", (n, m, N), err)
    assert (err <= 1e-12).all(), err
    bs = dense_solver(ndlqr, probs, drop_H=True)
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), Z0)  # H = NULL is H = 0, bit for bit
    bs.close()


# ---------------------------------------------------------------------------- 4, 5: rhs-only re-solve and adjoint
def keep_flags(ndlqr, N):
    # (a device horizon below 8 has no record-based re-solve: the factor array there)
    return ndlqr.FLAG_KEEP_FACT if N < 5 else ndlqr.FLAG_KEEP_RECORDS


@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", [(6, 3, 2), (6, 3, 5), (12, 4, 16), (7, 9, 5), (20, 5, 8), (32, 8, 16)])
def test_rhs_only_resolve(ndlqr, n, m, N, name):
    fam = cs.family(n, m, N, name)
    flags = keep_flags(ndlqr, N)
    rng = np.random.default_rng([n, m, N, 4])
    rhs = [(rng.standard_normal((N, n)), rng.standard_normal((N, m)), rng.standard_normal((N, n)), rng.standard_normal(n))
           for _ in range(cs.BATCH)]
    probs2 = [dict(p, q=q, r=r, d=d, x0=x0) for p, (q, r, d, x0) in zip(fam["probs"], rhs)]
    ref = np.stack([cs.refined_solve(*cs.dense_kkt(p)) for p in probs2])
    bs = dense_solver(ndlqr, fam["probs"], flags)
    assert bs.solve() == 0
    bs.set_rhs_flat(*[np.stack(a) for a in zip(*rhs)])
    assert bs.cost_is_dense()
    assert bs.solve_rhs_only() == 0
    Z = bs.solutions()
    bs.close()
    check(ndlqr, name, Z, fam["probs"], ref, flags, "rhs-only", rhs=rhs)


@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", [(6, 3, 2), (6, 3, 5), (12, 4, 16), (7, 9, 5), (20, 5, 8), (32, 8, 16)])
def test_adjoint(ndlqr, n, m, N, name):
    fam = cs.family(n, m, N, name)
    flags = keep_flags(ndlqr, N)
    bs = dense_solver(ndlqr, fam["probs"], flags)
    assert bs.solve() == 0
    Z = bs.solutions()
    assert bs.solve_adjoint(fam["g"].copy()) == 0
    W = bs.adjoint()
    assert W.shape == (cs.BATCH, (2 * n + m) * N - m)
    # ... from and into device memory: the same bits; the primal solution is untouched
    g_dev, w_dev = ndlqr.DeviceArray(W.shape).set(fam["g"]), ndlqr.DeviceArray(W.shape)
    assert bs.solve_adjoint(g_dev) == 0
    bs.adjoint(w_dev)
    assert np.array_equal(w_dev.get(), W) and np.array_equal(bs.solutions(), Z)
    bs.close()
    check(ndlqr, name, W, fam["probs"], fam["w"], flags, "adjoint", adjoint=fam["g"])


# ---------------------------------------------------------------------------- 6: the last knot is never loaded
@pytest.mark.parametrize("n,m,N", [(6, 3, 2), (12, 4, 5), (7, 9, 8), (20, 5, 5), (32, 8, 16)])
def test_last_knot_is_never_loaded(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    flags = keep_flags(ndlqr, N)

    def run(probs):
        bs = dense_solver(ndlqr, probs, flags)
        assert bs.solve() == 0 and bs.cholesky_failures() == 0
        out = [bs.solutions(), bs.cost_reduction()]
        assert bs.solve_adjoint(fam["g"].copy()) == 0
        out.append(bs.adjoint())
        bs.set_rhs_flat(*cs.flat(probs, ("q", "r", "d", "x0")))
        assert bs.solve_rhs_only() == 0
        out.append(bs.solutions())
        bs.close()
        return out

    clean = run(fam["probs"])
    bad = []
    for p in fam["probs"]:
        p = {k: v.copy() for k, v in p.items()}
        for k in ("A", "B", "H", "R", "r", "d"):
            p[k][N - 1] = np.nan
        bad.append(p)
    Z, red, W, Z2 = run(bad)
    assert np.isfinite(Z).all() and np.array_equal(Z, clean[0])
    for k in RED_NAMES:
        assert np.isfinite(red[k]).all() and np.array_equal(red[k], clean[1][k]), k
    assert np.isfinite(W).all() and np.array_equal(W, clean[2])
    assert np.isfinite(Z2).all() and np.array_equal(Z2, clean[3])


# ---------------------------------------------------------------------------- 7: not positive definite
@pytest.mark.parametrize("which", ["R", "Qp"])
@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8), (7, 9, 2), (32, 8, 8)])
def test_not_positive_definite(ndlqr, n, m, N, which):
    fam = cs.family(n, m, N, "moderate")
    probs = [{k: v.copy() for k, v in p.items()} for p in fam["probs"]]
    k = (N - 1) // 2
    if which == "R":
        probs[1]["R"][k] = -probs[1]["R"][k]  # indefinite R_k
    else:  # Q_k - H R^-1 H' = -1/2
        probs[1]["Q"][k] = probs[1]["H"][k] @ np.linalg.solve(probs[1]["R"][k], probs[1]["H"][k].T) - 0.5 * np.eye(n)
        probs[1]["Q"][k] = 0.5 * (probs[1]["Q"][k] + probs[1]["Q"][k].T)
    bs = dense_solver(ndlqr, probs)
    assert bs.solve() == ndlqr.api.ERR_NOT_SPD
    assert bs.cholesky_failures() >= 1
    Z = bs.solutions()
    red = bs.cost_reduction()
    bs.close()
    for i in (0, 2):
        err = np.array(cs.field_errors(Z[i], fam["z"][i], n, m, N))
        assert (err <= REL_TOL).all(), (i, err)
        for name in RED_NAMES:
            assert np.isfinite(red[name][i]).all()


# ---------------------------------------------------------------------------- 8: mode switching
def refused_calls(ndlqr, bs):
    """(the name that opens the refusal, a call that must return -1 or raise) for every entry point refused in dense mode"""
    n, m, N, b = bs.n, bs.m, bs.N, bs.batch
    z = lambda *s: np.zeros(s)
    out5 = (C.c_void_p * 5)()
    ptrs = [C.POINTER(C.c_double)() for _ in range(4)]
    L = bs.L
    return [
        ("ndlqr_hip_step_async", lambda: bs.step_async(z(b, N, n), z(b, N, m), z(b, N, n), z(b, n), z(b, bs.nvars))),
        ("ndlqr_hip_set_step_selection", lambda: bs.set_step_selection(0, 1, 7)),
        ("ndlqr_hip_solve_slices_async", lambda: bs.solve_slices_async(0, 1, 7, ndlqr.pinned_empty((b, 1, 2 * n + m)))),
        ("ndlqr_hip_download_selection", lambda: bs.solution_slices(0, 1, 7)),
        ("ndlqr_hip_solve_multi_rhs", lambda: bs.solve_multi_rhs(z(2, b, N, n), z(2, b, N, m), z(2, b, N, n), z(2, b, n))),
        ("ndlqr_hip_solve_multi_rhs_slices",
         lambda: bs.solve_multi_rhs(z(2, b, N, n), z(2, b, N, m), z(2, b, N, n), z(2, b, n), selection=(0, 1, 4))),
        ("ndlqr_hip_gradients", lambda: bs.gradients()),
        ("ndlqr_hip_refine", lambda: bs.refine(1)),
        ("ndlqr_hip_refine", lambda: bs.refine_adjoint(1)),
        ("ndlqr_hip_kkt_residual", lambda: bs.kkt_residuals()),
        ("ndlqr_hip_kkt_residual_vector", lambda: bs.kkt_residual_vector()),
        ("ndlqr_hip_set_bounds", lambda: bs.set_bounds(ulo=-np.ones(m), uhi=np.ones(m))),
        ("ndlqr_hip_solve_box", lambda: bs.solve_box()),
        ("ndlqr_hip_time_shard_top_doubles", lambda: bs.time_shard_top_doubles(2)),
        ("ndlqr_hip_time_shard_factor", lambda: bs.time_shard_factor(0, 2)),
        ("ndlqr_hip_download_factors", lambda: bs.factors(0)),
        ("ndlqr_hip_device_pointers", lambda: L.ndlqr_hip_device_pointers(bs.ctx, out5)),
        ("ndlqr_hip_staged_io", lambda: L.ndlqr_hip_staged_io(bs.ctx, *[C.byref(p) for p in ptrs])),
    ]


def outcome(bs, call):
    """(refused, message): refused = the call returned a negative code or raised"""
    try:
        ret = call()
    except (RuntimeError, ValueError):
        return True, bs.L.ndlqr_hip_last_error().decode()
    if isinstance(ret, int) and ret < 0:
        return True, bs.L.ndlqr_hip_last_error().decode()
    return False, ""


def test_mode_switching(ndlqr, oracle):
    from support import Problem
    n, m, N = 12, 4, 8
    fam = cs.family(n, m, N, "moderate")
    flags = ndlqr.FLAG_KEEP_RECORDS
    bs = dense_solver(ndlqr, fam["probs"], flags)
    assert bs.solve() == 0 and bs.solve_adjoint(fam["g"].copy()) == 0
    for who, call in refused_calls(ndlqr, bs):
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":") and "dense-cost" in msg, (who, refused, msg)
    assert bs.cost_is_dense()
    check(ndlqr, "moderate", bs.solutions(), fam["probs"], fam["z"], flags, "after the refusals")
    # a diagonal initialiser leaves the mode: everything works again
    gen = [ndlqr.generate_synthetic(n, m, N, 60 + i) for i in range(cs.BATCH)]
    diag = [np.stack([g[k] for g in gen]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")]
    bs.initialize_flat(*diag)
    assert not bs.cost_is_dense()
    assert bs.solve() == 0
    Z = bs.solutions()
    for p, g in enumerate(gen):
        ref = oracle.solve(Problem(n, m, N, *[g[k] for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")]), 1)[0][: bs.nvars]
        assert np.linalg.norm(Z[p] - ref) <= REL_TOL * np.linalg.norm(ref), p
    must_work = ("ndlqr_hip_set_step_selection", "ndlqr_hip_download_selection", "ndlqr_hip_gradients", "ndlqr_hip_refine",
                 "ndlqr_hip_kkt_residual", "ndlqr_hip_kkt_residual_vector", "ndlqr_hip_set_bounds", "ndlqr_hip_solve_box",
                 "ndlqr_hip_step_async", "ndlqr_hip_solve_slices_async")
    for who, call in refused_calls(ndlqr, bs):
        # (each call on a fresh solve and adjoint: some of them replace the resident solution)
        assert bs.synchronize() == 0 and bs.solve() == 0 and bs.solve_adjoint(fam["g"].copy()) == 0
        refused, msg = outcome(bs, call)
        # (the others need another configuration -- a schedule, a flag, a longer horizon: that is their own refusal)
        assert "dense-cost" not in msg, (who, msg)
        assert not (refused and who in must_work), (who, msg)
        if who == "ndlqr_hip_set_step_selection":
            bs.set_step_selection()
    bs.close()
    # ... and back: a fresh solver through diagonal -> dense
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH, flags=flags)
    bs.initialize_flat(*diag)
    assert bs.solve() == 0
    bs.initialize_flat_dense(*cs.flat(fam["probs"]))
    assert bs.cost_is_dense() and bs.solve() == 0
    check(ndlqr, "moderate", bs.solutions(), fam["probs"], fam["z"], flags, "dense again")
    bs.close()


def test_block_size_beyond_the_lds_is_refused_by_name(ndlqr):
    n, m, N = 96, 8, 2
    bs = ndlqr.BatchSolver(n, m, N, 1)
    z = lambda *s: np.zeros(s)
    with pytest.raises(RuntimeError, match="ndlqr_hip_init_dense: cost_transform"):
        bs.initialize_flat_dense(z(1, N, n * n), z(1, N, n * m), z(1, N, n * n), None, z(1, N, m * m), z(1, N, n), z(1, N, m),
                                 z(1, N, n), z(1, n))
    assert not bs.cost_is_dense()
    bs.close()


# ---------------------------------------------------------------------------- 9: lqr_solve_dense
# torch runs in a child process (test_gpu_gradients.py has the reason: torch's own HIP runtime must start first)
GRAD_TOL = 1e-8  # the bar of test_gpu_gradients.py for lqr_solve


def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_cost as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _tensors(probs, names=cs.NAMES):
    import torch
    return {k: torch.tensor(np.stack([p[k] for p in probs]), dtype=torch.float64, device="cuda", requires_grad=True)
            for k in names}


def _case_lqr_solve_dense(ndlqr, n, m, N):
    import torch
    from rslqr_amd.autograd import lqr_solve_dense
    fam = cs.family(n, m, N, "moderate")
    t = _tensors(fam["probs"])
    z = lqr_solve_dense(*[t[k] for k in cs.NAMES])
    check(ndlqr, "moderate", z.detach().cpu().numpy(), fam["probs"], fam["z"], ndlqr.FLAG_KEEP_RECORDS, "lqr_solve_dense")
    (z * torch.tensor(fam["g"], device="cuda")).sum().backward()
    for i, p in enumerate(fam["probs"]):
        ref = cs.gradient_reference(p, fam["z"][i], fam["w"][i])
        for k in cs.NAMES:
            got = t[k].grad[i].cpu().numpy()
            assert got.shape == ref[k].shape, k
            err = rel(got, ref[k])
            print("gradient", (n, m, N), i, k, err)
            assert err <= GRAD_TOL, (i, k, err)
        assert np.array_equal(t["Q"].grad[i].cpu().numpy(), t["Q"].grad[i].cpu().numpy().transpose(0, 2, 1))
        assert np.array_equal(t["R"].grad[i].cpu().numpy(), t["R"].grad[i].cpu().numpy().transpose(0, 2, 1))
    # shared arguments: their gradients are the batch sums
    sh = ("A", "q")
    shared = {k: (t[k].detach()[0].clone() if k in sh else t[k].detach().clone()).requires_grad_(True) for k in cs.NAMES}
    probs = [dict(p, A=fam["probs"][0]["A"], q=fam["probs"][0]["q"]) for p in fam["probs"]]
    z = lqr_solve_dense(*[shared[k] for k in cs.NAMES])
    (z * torch.tensor(fam["g"], device="cuda")).sum().backward()
    refs = []
    for i, p in enumerate(probs):
        K, b = cs.dense_kkt(p)
        refs.append(cs.gradient_reference(p, cs.refined_solve(K, b), cs.refined_solve(K, fam["g"][i])))
    for k in sh:
        assert shared[k].grad.shape == shared[k].shape
        assert rel(shared[k].grad.cpu().numpy(), sum(r[k] for r in refs)) <= GRAD_TOL, k
    assert rel(shared["H"].grad.cpu().numpy(), np.stack([r["H"] for r in refs])) <= GRAD_TOL


def _case_lqr_solve_dense_diagonal(ndlqr, n, m, N):
    import torch
    from rslqr_amd.autograd import lqr_solve, lqr_solve_dense
    probs, Qd, Rd = zip(*[cs.diagonal_problem(n, m, N, 70 + i) for i in range(cs.BATCH)])
    t = _tensors(probs)
    g = torch.randn((cs.BATCH, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    z = lqr_solve_dense(*[t[k] for k in cs.NAMES])
    (z * g).sum().backward()
    d = _tensors(probs, ("A", "B", "q", "r", "d", "x0"))
    d["Q"] = torch.tensor(np.stack(Qd), device="cuda", requires_grad=True)
    d["R"] = torch.tensor(np.stack(Rd), device="cuda", requires_grad=True)
    zd = lqr_solve(*[d[k] for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")])
    (zd * g).sum().backward()
    assert rel(z.detach().cpu().numpy(), zd.detach().cpu().numpy()) <= REL_TOL
    for k in ("A", "B", "q", "r", "d", "x0"):
        assert rel(t[k].grad.cpu().numpy(), d[k].grad.cpu().numpy()) <= GRAD_TOL, k
    for k in ("Q", "R"):
        diag = torch.diagonal(t[k].grad, dim1=-2, dim2=-1)
        assert rel(diag.cpu().numpy(), d[k].grad.cpu().numpy()) <= GRAD_TOL, k


def _case_lqr_solve_dense_refuses(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve_dense
    t = _tensors(cs.family(6, 3, 5, "moderate")["probs"])
    args = [t[k].detach() for k in cs.NAMES]
    with pytest.raises(ValueError):
        lqr_solve_dense(*(args[:2] + [args[2][..., 0]] + args[3:]))  # Q as diagonals
    with pytest.raises(TypeError):
        lqr_solve_dense(*(args[:3] + [args[3].float()] + args[4:]))
    with pytest.raises(ValueError):
        lqr_solve_dense(*([args[0].cpu()] + args[1:]))
    bad = [a.clone() for a in args]
    bad[4][1, 1] = -bad[4][1, 1]  # an indefinite R
    with pytest.raises(RuntimeError, match="not positive definite"):
        lqr_solve_dense(*bad)


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8)])
def test_lqr_solve_dense(n, m, N):
    """Forward as test 2; the backward for all nine tensors against -(dK/dtheta z - db/dtheta)' w from the refined z, w."""
    _run_case("_case_lqr_solve_dense", n, m, N)


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8)])
def test_lqr_solve_dense_at_diagonal_costs(n, m, N):
    """H = 0 and diagonal Q, R: the diagonals of dL/dQ, dL/dR and the other gradients equal lqr_solve's."""
    _run_case("_case_lqr_solve_dense_diagonal", n, m, N)


def test_lqr_solve_dense_refuses_bad_arguments():
    _run_case("_case_lqr_solve_dense_refuses")
