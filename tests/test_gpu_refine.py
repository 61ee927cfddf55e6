"""Iterative refinement of batch solves with a double-double residual (ndlqr_RefineBatch, ndlqr_RefineBatchAdjoint,
ndlqr_BatchKktResidualVector) against the numpy restatement of tests/refine_support.py, the CPU
oracle and support.refined_solution.

Accuracy in fast mode (test_fast_mode_reaches_the_cpu_loop, measured on an MI355X; normwise error per field lambda | x | u
against refined_solution(iters=5), in units of eps ||field||_inf, the worst problem of each batch):

    shape x batch    before               after refine(2)      CPU loop on the oracle   steps
    (12,4,64) x 4    1770 / 1107 / 632    0.08 / 0.14 / 0.14   0.08 / 0.14 / 0.14       1 1 1 1
    (6,3,32) x 4     221 / 193 / 184      0.01 / 0.07 / 0.04   0.01 / 0.07 / 0.04       1 1 1 1
    (7,9,16) x 2     85 / 67 / 32         0 / 0 / 0            0 / 0 / 0                1 1
    (16,4,32) x 2    2715 / 880 / 1124    0.21 / 0.23 / 0      0.21 / 0.23 / 0          1 1

(a_scale 1.05, q_scale 1e-2, r_scale 1e-4, KEEP_RECORDS; eta 2e-15 .. 1.7e-13 before, 1.5e-17 .. 5.4e-17 after.) Across the
schedule table of test_gpu_gradients.py the errors ran from 0.3 .. 5.6e6 eps before to 0 .. 0.45 eps after.
"""
import ctypes as C

import numpy as np
import pytest

from refine_support import EPS, field_errors, hard_problem, refine_loop, residual_dd
from support import refined_solution
from test_gpu_gradients import ARGS, SCHEDULE_CASES, SCHEDULE_FAMILIES, _FLAGS, adjoint_problem, check_directions, stack, synth
from test_refine_host import AT_ROUNDING, AT_ROUNDING_SCALES

pytestmark = pytest.mark.gpu


def solver(ndlqr, probs, flags):
    p0 = probs[0]
    bs = ndlqr.BatchSolver(p0.n, p0.m, p0.N, len(probs), flags=flags)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    return bs


def refine_code(bs, name="ndlqr_RefineBatch", max_steps=2):
    """The C return code with every output NULL."""
    return getattr(bs.L, name)(bs.h, max_steps, None, None, None)


def bar_of(oracle, prob, truth):
    """The bar of a refined solution per field: four times the error the CPU restatement loop reaches on the same problem
    (the fast re-solve rounds differently from the oracle), floored at 4 eps ||field||_inf."""
    z_cpu = refine_loop(oracle, prob, oracle.solve(prob, 1)[0][: prob.nvars], 2)[0]
    err_cpu, size = field_errors(prob, z_cpu, truth)
    return np.maximum(4 * err_cpu, 4 * EPS * size), err_cpu, size


def check_refined(oracle, prob, z_before, z_after, label, never_worse=False):
    truth = refined_solution(oracle, prob, iters=5)
    bar, err_cpu, size = bar_of(oracle, prob, truth)
    before, _ = field_errors(prob, z_before, truth)
    after, _ = field_errors(prob, z_after, truth)
    print(label, "err/(eps|f|) before", (before / (EPS * size)).round(2), "after", (after / (EPS * size)).round(2),
          "cpu", (err_cpu / (EPS * size)).round(2))
    assert np.all(after <= bar), (label, after / (EPS * size), bar / (EPS * size))
    if never_worse:
        assert np.all(after <= before), (label, before / (EPS * size), after / (EPS * size))


# ------------------------------------------------------------------------------------------------ 1. the residual vector

# row-broadcast, matrix-core, zero-padded, runtime-sized, and N = 2: the first and the last knot only
RESIDUAL_SHAPES = [(6, 3, 8), (12, 4, 16), (7, 9, 8), (16, 4, 8), (6, 3, 2), (12, 4, 2)]


@pytest.mark.parametrize("n,m,N", RESIDUAL_SHAPES)
@pytest.mark.parametrize("strict", [False, True])
def test_residual_vector_bit_exact(ndlqr, n, m, N, strict):
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 40 + p) for p in range(2)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_STRICT_FP if strict else 0)
    z = bs.solutions()
    r = bs.kkt_residual_vector()
    assert np.array_equal(bs.solutions(), z)
    for p, prob in enumerate(probs):
        ref = residual_dd(prob, z[p])[0]
        assert np.array_equal(r[p], ref), (p, np.max(np.abs(r[p] - ref)))
    rd = bs.kkt_residual_vector(ndlqr.DeviceArray((2, bs.nvars))).get()
    assert np.array_equal(rd, r)
    bs.close()


# ------------------------------------------------------------------------------------------------ 2. strict mode

@pytest.mark.parametrize("n,m,N,seed", AT_ROUNDING)
def test_strict_refinement_bit_exact(ndlqr, oracle, n, m, N, seed):
    """A problem at rounding (rejected at step 1) beside a weak-R one (accepted): z, steps and both eta equal the
    restatement loop on the oracle bit for bit."""
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, seed, *AT_ROUNDING_SCALES),
             hard_problem(ndlqr.generate_synthetic, n, m, N, seed)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_FACT | ndlqr.FLAG_STRICT_FP)
    z0 = bs.solutions().copy()
    steps, before, after = bs.refine(2)
    z = bs.solutions()
    want_steps = []
    for p, prob in enumerate(probs):
        assert np.array_equal(z0[p], oracle.solve(prob, 1)[0][: prob.nvars])
        zr, st, eb, ea = refine_loop(oracle, prob, z0[p], 2)
        want_steps.append(st)
        assert steps[p] == st and before[p] == eb and after[p] == ea, (p, steps[p], st, before[p], eb, after[p], ea)
        assert np.array_equal(z[p], zr), (p, np.max(np.abs(z[p] - zr)))
    assert want_steps[0] == 0 and want_steps[1] >= 1, want_steps
    assert z[0].tobytes() == z0[0].tobytes()
    bs.close()


# ------------------------------------------------------------------------------------------------ 3. fast mode

@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 4), (6, 3, 32, 4), (7, 9, 16, 2), (16, 4, 32, 2)])
def test_fast_mode_reaches_the_cpu_loop(ndlqr, oracle, n, m, N, batch):
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 300 + p) for p in range(batch)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    z0 = bs.solutions().copy()
    steps, before, after = bs.refine(2)
    z = bs.solutions()
    print((n, m, N), "steps", steps, "eta", before, "->", after)
    assert np.all(after <= before) and np.all(steps >= 0) and np.all(steps <= 2)
    for p, prob in enumerate(probs):
        check_refined(oracle, prob, z0[p], z[p], ((n, m, N), p), never_worse=True)
    bs.close()


# ------------------------------------------------------------------------------------------------ 4. guard

def test_nan_and_problems_at_rounding(ndlqr):
    n, m, N = 6, 3, 8
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 61), hard_problem(ndlqr.generate_synthetic, n, m, N, 62),
             hard_problem(ndlqr.generate_synthetic, n, m, N, 63)]
    probs[1].q[3, 2] = np.nan
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    z0 = bs.solutions().copy()
    steps, before, after = bs.refine(2)
    z = bs.solutions()
    assert steps[1] == 0 and z[1].tobytes() == z0[1].tobytes()
    assert steps[0] >= 1 and steps[2] >= 1 and after[0] < before[0] and after[2] < before[2]
    # the refined problems are at rounding now: 0 steps or 1, and 0 steps leave every bit
    steps2, before2, after2 = bs.refine(2)
    z2 = bs.solutions()
    assert steps2[1] == 0 and z2[1].tobytes() == z0[1].tobytes()
    for p in (0, 2):
        assert steps2[p] in (0, 1) and after2[p] <= before2[p] and before2[p] == after[p]
        if steps2[p] == 0:
            assert z2[p].tobytes() == z[p].tobytes()
    bs.close()


# ------------------------------------------------------------------------------------------------ 5. state

def test_refusals(ndlqr, monkeypatch):
    monkeypatch.setenv("NDLQR_TREE", "0")
    n, m, N, batch = 12, 4, 64, 2
    probs = [synth(ndlqr, n, m, N, 800 + p) for p in range(batch)]
    g = np.random.default_rng(7).standard_normal((batch, (2 * n + m) * N - m))
    bs = solver(ndlqr, probs, 0)  # no kept factorisation
    assert refine_code(bs) == -1 and refine_code(bs, "ndlqr_RefineBatchAdjoint") == -1
    bs.kkt_residual_vector()  # (needs none)
    bs.close()
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    assert refine_code(bs, max_steps=0) == -1 and refine_code(bs, max_steps=9) == -1
    assert refine_code(bs, "ndlqr_RefineBatchAdjoint") == -1  # no adjoint
    assert refine_code(bs) == 0
    # after a step that computed a slice alone
    bs.set_step_selection(0, 8, ndlqr.SOLN_INPUT | ndlqr.SOLN_ONLY)
    x0 = ndlqr.pinned_empty((batch, n))
    x0[:] = np.stack([p.x0 for p in probs])
    out = ndlqr.pinned_empty((batch, 8, m))
    assert bs.step_async(None, None, None, x0, out) == 0
    assert bs.synchronize() == 0
    assert refine_code(bs) == -1
    with pytest.raises(RuntimeError):
        bs.kkt_residual_vector()
    bs.set_step_selection()
    assert bs.solve() == 0 and refine_code(bs) == 0
    # after a constrained solve
    bs.set_bounds(ulo=-0.5 * np.ones(m), uhi=0.5 * np.ones(m))
    bs.solve_box(max_iter=50)
    assert refine_code(bs) == -1
    # an adjoint taken before the refinement is refused afterwards
    assert bs.solve() == 0 and bs.solve_adjoint(g) == 0
    assert refine_code(bs, "ndlqr_RefineBatchAdjoint") == 0
    bs.adjoint()
    assert refine_code(bs) == 0
    assert refine_code(bs, "ndlqr_RefineBatchAdjoint") == -1
    with pytest.raises(RuntimeError):
        bs.adjoint()
    bs.close()


@pytest.mark.parametrize("flags", ["records", "fact"])
def test_kept_state_untouched(ndlqr, monkeypatch, flags):
    """An rhs-only re-solve after refine equals one from an identical solver that never refined, bit for bit; the
    factorisation count does not move; the residual norms, the getters and the device pack see the refined solution."""
    monkeypatch.setenv("NDLQR_TREE", "0")
    n, m, N, batch = 12, 4, 64, 3
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 900 + p) for p in range(batch)]
    fl = getattr(ndlqr, _FLAGS[flags])
    a, b = solver(ndlqr, probs, fl), solver(ndlqr, probs, fl)
    count = a.factor_count()
    res0 = a.kkt_residuals()[0]
    steps, before, after = a.refine(2)
    assert a.factor_count() == count and a.L.ndlqr_BatchGetFlags(a.h) == fl
    assert np.all(steps >= 1) and np.all(a.kkt_residuals()[0] < res0)
    z = a.solutions()
    assert not np.array_equal(z, b.solutions())
    dev = ndlqr.DeviceArray((batch, a.nvars))
    a.solutions_to_device(dev.ptr)
    assert a.synchronize() == 0 and np.array_equal(dev.get(), z)
    # pinned and device outputs deliver the same as pageable ones (a second refinement of the same state: solver b)
    st_h, eb_h, ea_h = b.refine(2)
    assert np.array_equal(st_h, steps) and np.array_equal(eb_h, before) and np.array_equal(ea_h, after)
    assert np.array_equal(b.solutions(), z)
    rng = np.random.default_rng(12)
    rhs = [rng.standard_normal(s) for s in ((batch, N, n), (batch, N, m), (batch, N, n), (batch, n))]
    c = solver(ndlqr, probs, fl)  # never refined
    for s in (a, c):
        s.set_rhs_flat(*rhs)
        assert s.solve_rhs_only() == 0
    assert np.array_equal(a.solutions(), c.solutions())
    for s in (a, b, c):
        s.close()


def test_output_pointer_kinds(ndlqr):
    n, m, N, batch = 6, 3, 32, 3
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 950 + p) for p in range(batch)]
    a, b = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS), solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    steps, before, after = a.refine(2)
    eb, ea = ndlqr.DeviceArray((batch,)), ndlqr.pinned_empty((batch,))
    ip = C.POINTER(C.c_int)
    st = np.zeros(batch, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    assert b.L.ndlqr_RefineBatch(b.h, 2, st.ctypes.data_as(ip), C.cast(C.c_void_p(eb.ptr), dp), ea.ctypes.data_as(dp)) == 0
    assert np.array_equal(st, steps) and np.array_equal(eb.get(), before) and np.array_equal(np.array(ea), after)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 6. reach

@pytest.mark.parametrize("n,m,N,batch,flags,tree,want,check", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
@pytest.mark.parametrize("a_scale,q_scale,r_scale", SCHEDULE_FAMILIES)
def test_every_schedule_refines(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want, check, a_scale, q_scale,
                                r_scale):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 1500 + p, a_scale, q_scale, r_scale) for p in range(batch)]
    fl = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT if flags == "strict" else getattr(ndlqr, _FLAGS[flags])
    bs = solver(ndlqr, probs, fl)
    assert bs.schedule() == want, bs.schedule()
    p = check[0]
    z0 = bs.solution(p)
    steps, before, after = bs.refine(2)
    assert np.all(after <= before), (before, after)
    check_refined(oracle, probs[p], z0, bs.solution(p), (want, (n, m, N), p))
    bs.close()


# ------------------------------------------------------------------------------------------------ 7. adjoint, autograd

@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 2), (7, 9, 16, 2)])
def test_refined_adjoint_and_gradients(ndlqr, oracle, n, m, N, batch):
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 700 + p) for p in range(batch)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    g = np.random.default_rng(21).standard_normal((batch, bs.nvars))
    bs.refine(2)
    z = bs.solutions().copy()
    assert bs.solve_adjoint(g) == 0
    w0 = bs.adjoint().copy()
    steps, before, after = bs.refine_adjoint(2)
    assert np.all(after <= before)
    assert np.array_equal(bs.solutions(), z)  # (the adjoint's refinement changes w alone)
    w = bs.adjoint()
    grads = bs.gradients()
    for p, prob in enumerate(probs):
        ap = adjoint_problem(prob, g[p])
        z_true, w_true = refined_solution(oracle, prob, iters=5), refined_solution(oracle, ap, iters=5)
        check_refined(oracle, ap, w0[p], w[p], ("adjoint", (n, m, N), p))
        zbar, _, _ = bar_of(oracle, prob, z_true)
        assert np.all(field_errors(prob, z[p], z_true)[0] <= zbar)
        check_directions(prob, {k: grads[k][p] for k in ARGS}, z[p], w[p], z_true, w_true, 30 + p)
    bs.close()


def test_torch_refine():
    """lqr_solve(refine=2) gives what the explicit calls give, refine=0 what the solver gives without refinement."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_refine as T\n"
            "T._case_torch_refine(rslqr_amd)\n"
            "print('case ok')\n" % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _case_torch_refine(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve
    n, m, N, batch = 12, 4, 32, 2
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 1000 + p) for p in range(batch)]
    t = {}
    for k, a in zip(ARGS, stack(probs)):
        if k in ("A", "B"):
            cols = n if k == "A" else m
            a = a.reshape(batch, N, cols, n).transpose(0, 1, 3, 2)  # column-major flat -> row-major matrices
        t[k] = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    for refine in (0, 2):
        for v in t.values():
            v.grad = None
        z = lqr_solve(*[t[k] for k in ARGS], refine=refine)
        (z * gz).sum().backward()
        bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
        if refine:
            bs.refine(refine)
        assert np.array_equal(z.detach().cpu().numpy(), bs.solutions()), refine
        assert bs.solve_adjoint(gz.cpu().numpy()) == 0
        if refine:
            bs.refine_adjoint(refine)
        grads = bs.gradients()
        for k in ARGS:
            got = t[k].grad.detach().cpu().numpy()
            if k in ("A", "B"):
                got = np.ascontiguousarray(got.transpose(0, 1, 3, 2)).reshape(grads[k].shape)
            assert np.array_equal(got, grads[k]), (refine, k)
        bs.close()
