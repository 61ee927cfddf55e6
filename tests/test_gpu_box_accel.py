"""Anderson acceleration of the box-constrained batch solve (ndlqr_BatchSetBoxAcceleration, ndlqr_CopyBatchBoxAcceleration;
DESIGN.md section 3.15) on the device, against box_accel_support.admm_accel_reference -- the numpy restatement of the
rule driving the oracle -- and the references of box_support.py.

The comparisons with the restatement hold to a tolerance: 100 x what a permutation of the restatement's own sums moves
the result by (test_box_accel_host.GPU_TOLERANCE_12 for the 12-iteration runs; computed in the test, from two runs of the
restatement, for the 40-iteration rejection case). Relative differences are max |a - b| / max |b| per problem, as in the
host test that measures them. The restatement adds its dot products in the order of the kernel's reduction
(box_accel_support.tree_dot), so in strict mode and on an unpadded shape it follows the device down to the last bit --
gamma included, which a different order of the sums moves by up to 2e-12; the 12-iteration tests print whether it did
(measured on the MI355X: solution, mu and gamma bit for bit in all four cases)."""
import numpy as np
import pytest

from box_accel_support import admm_accel_reference
from box_support import masks
from test_box_accel_host import GPU_TOLERANCE_12, MEM, _family, sensitivity_cases
from test_gpu_box import check_certificate, input_bounded_states, input_box, solver, state_box, synth

pytestmark = pytest.mark.gpu

ALPHA = 1.6


def maxrel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def strict_flags(ndlqr):
    return ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT


def results(bs):
    mux, muu = bs.bound_multipliers()
    return bs.solutions().copy(), mux.copy(), muu.copy()


# ------------------------------------------------------------------------------------------------ 1. off is off

@pytest.mark.parametrize("strict", [False, True])
def test_memory_set_back_to_zero_is_bit_identical_to_never_set(ndlqr, oracle, strict):
    n, m, N, batch = 12, 4, 16, 2
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    fl = strict_flags(ndlqr) if strict else 0
    kw = dict(rho=float(np.mean([p.Q.mean() for p in probs])), alpha=ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=300)
    a = solver(ndlqr, probs, fl)
    a.set_bounds(xlo, xhi, ulo, uhi)
    it_a, st_a = a.solve_box(**kw)
    with pytest.raises(RuntimeError):  # (no accelerated solve: nothing to read out)
        a.box_acceleration()
    b = solver(ndlqr, probs, fl)
    b.set_bounds(xlo, xhi, ulo, uhi)
    b.set_box_acceleration(MEM)
    it_on, st_on = b.solve_box(**kw)
    assert b.box_acceleration()[0].sum() > 0
    b.set_box_acceleration(0)
    it_b, st_b = b.solve_box(**kw)
    assert np.array_equal(it_a, it_b) and np.array_equal(st_a, st_b), (it_a, it_b, st_a, st_b)
    assert not np.array_equal(it_a, it_on)  # (the setting did something while it was on)
    for x, y in zip(results(a), results(b)):
        assert np.array_equal(x, y)
    with pytest.raises(RuntimeError):  # (the latest solve ran without acceleration)
        b.box_acceleration()
    # refusals leave the previous setting
    for bad in ((-1, 0.0, 0.0), (17, 0.0, 0.0), (5, -1.0, 0.0), (5, float("inf"), 0.0), (5, 0.0, float("nan")), (5, 0.0, -1e-3)):
        with pytest.raises(RuntimeError):
            b.set_box_acceleration(*bad)
    it_b, st_b = b.solve_box(**kw)
    assert np.array_equal(it_a, it_b)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2. twelve iterations

def twelve_iterations(ndlqr, oracle, bounds):
    """the device's 12 strict iterations at memory 5 of (12,4,16) x 2 and the restatement's: per problem
    (z, mu, gamma, accepted, rejected, columns) of the device, and the restatement's namespace"""
    probs, per, shared = sensitivity_cases(ndlqr, oracle)
    rows = per if bounds == "per_problem" else shared
    rho = 0.37
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    if bounds == "shared":
        bs.set_bounds(*rows[0])
    else:
        bs.set_bounds(*[np.stack([r[i] for r in rows]) for i in range(4)])
    bs.set_box_acceleration(MEM)
    it, st = bs.solve_box(rho=rho, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=12)
    assert (it == 12).all() and (st == 2).all(), (it, st)
    sol, mux, muu = results(bs)
    accepted, rejected, gamma, columns = bs.box_acceleration()
    bs.close()
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    out = []
    for p, prob in enumerate(probs):
        ref = admm_accel_reference(prob, solve, *rows[p], rho, ALPHA, 1e-300, 1e-300, 12, mem=MEM)
        assert ref.drops > 0  # (the ring wrapped)
        ref.z = np.concatenate([ref.lam, ref.x, ref.u], axis=1).reshape(-1)[: prob.nvars]
        ref.mu = np.concatenate([ref.mu_x, ref.mu_u], axis=1)
        out.append(((sol[p], np.concatenate([mux[p], muu[p]], axis=1), gamma[p], accepted[p], rejected[p], columns[p]), ref))
    return out


@pytest.mark.parametrize("bounds", ["per_problem", "shared"])
def test_twelve_strict_iterations_match_the_restatement(ndlqr, oracle, bounds):
    """[lam, v] and mu within the recorded tolerance, the counts equal"""
    for p, ((z, mu, gamma, accepted, rejected, columns), ref) in enumerate(twelve_iterations(ndlqr, oracle, bounds)):
        figures = (maxrel(z, ref.z), maxrel(mu, ref.mu))
        print("problem %d: relative difference of [lam, v] %.3g, mu %.3g (tolerance %.3g; bit for bit: %s); accepted %d, "
              "rejected %d, columns %d" % ((p,) + figures + (GPU_TOLERANCE_12, np.array_equal(z, ref.z) and np.array_equal(mu, ref.mu),
                                                            accepted, rejected, columns)))
        assert (accepted, rejected, columns) == (ref.accepted, ref.rejected, ref.columns), p
        assert max(figures) <= GPU_TOLERANCE_12, (p, figures)


@pytest.mark.parametrize("bounds", ["per_problem", "shared"])
def test_twelve_strict_iterations_gamma_matches_the_restatement(ndlqr, oracle, bounds):
    """gamma of the latest accelerated step within the same recorded tolerance. gamma solves normal equations that the
    weight 1e-10 leaves ill-conditioned: sums in another order move it by 1e-13 .. 2e-12 (the restatement's own figures
    between two orders), which is why the restatement adds in the kernel's order."""
    for p, ((z, mu, gamma, accepted, rejected, columns), ref) in enumerate(twelve_iterations(ndlqr, oracle, bounds)):
        figure = maxrel(gamma, ref.gamma)
        print("problem %d: relative difference of gamma %.3g (tolerance %.3g; bit for bit: %s)"
              % (p, figure, GPU_TOLERANCE_12, np.array_equal(gamma, ref.gamma)))
        assert figure <= GPU_TOLERANCE_12, (p, figure)


# ------------------------------------------------------------------------------------------------ 3. rejection

def test_safeguard_rejections_match_the_restatement(ndlqr, oracle):
    """(4,2,16), state and input bounds, rho = mean diag R, 40 iterations: five rejections in the restatement, every
    safeguard decision at least 1e-6 away from the threshold (measured: 7e-3). Tolerance of the final solution: 100 x
    what a permutation of the restatement's sums moves it by over these 40 iterations (measured: 3e-12 .. 9e-12, so
    3e-10 .. 9e-10; the shape runs unpadded, and the device's solution and mu were the restatement's bit for bit)."""
    prob, solve, fam = _family(ndlqr, oracle)
    b = fam["xu"]
    rho, iters = float(prob.R.mean()), 40
    run = lambda perm: admm_accel_reference(prob, solve, *b, rho, ALPHA, 1e-300, 1e-300, iters, mem=MEM, perm=perm)
    ref = run(None)
    assert ref.rejected >= 1 and ref.accepted >= 1, (ref.accepted, ref.rejected)
    assert all(abs(r - 1.0) > 1e-6 for _, r in ref.ratios), ref.ratios
    Mx, Mu = masks(prob.n, prob.m, prob.N, *b)
    other = run(np.random.default_rng(40).permutation(int(Mx.sum() + Mu.sum())))
    assert (other.accepted, other.rejected) == (ref.accepted, ref.rejected)
    pack = lambda r: (np.concatenate([r.lam, r.x, r.u], axis=1).reshape(-1)[: prob.nvars], np.concatenate([r.mu_x, r.mu_u], axis=1))
    tol = 100.0 * max(maxrel(x, y) for x, y in zip(pack(other), pack(ref)))
    assert 0.0 < tol <= 1e-8, tol
    bs = solver(ndlqr, [prob], strict_flags(ndlqr))
    bs.set_bounds(*b)
    bs.set_box_acceleration(MEM)
    it, st = bs.solve_box(rho=rho, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
    assert it[0] == iters and st[0] == 2
    accepted, rejected, gamma, columns = bs.box_acceleration()
    sol, mux, muu = results(bs)
    zr, mr = pack(ref)
    figures = (maxrel(sol[0], zr), maxrel(np.concatenate([mux[0], muu[0]], axis=1), mr))
    print("rejections %d, accepted %d; relative difference of [lam, v] %.3g, mu %.3g (tolerance %.3g)"
          % (rejected[0], accepted[0], figures[0], figures[1], tol))
    assert (accepted[0], rejected[0], columns[0]) == (ref.accepted, ref.rejected, ref.columns)
    assert max(figures) <= tol, (figures, tol)
    bs.close()


# ------------------------------------------------------------------------------------------------ 4. launch classes

LAUNCH_CASES = [(5, 2, 2, 3, "records", None, "generic-reduced-records"),   # 2 bounded entries: a singular Gram matrix
                (12, 4, 64, 3, "records", "0", "reduced-compact-records"),  # 1008 entries: strides of 256, a ragged last
                (7, 9, 16, 2, "records", "0", "reduced-compact-records"),   # padded shape
                (16, 4, 32, 2, "none", None, None),                         # runtime-sized
                (12, 4, 16, 2, "strict", None, "knot-strict")]


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", LAUNCH_CASES, ids=["%d.%d.%d.x%d-%s" % c[:5] for c in LAUNCH_CASES])
def test_launch_classes_converge_in_fewer_iterations(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want):
    """bounds, penalties and settings of test_gpu_box.test_every_schedule_meets_the_certificate"""
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 1500 + p) for p in range(batch)]
    fl = {"records": ndlqr.FLAG_KEEP_RECORDS, "none": 0, "strict": strict_flags(ndlqr)}[flags]
    bs = solver(ndlqr, probs, fl)
    ulo, uhi = input_box(oracle, probs, 0.5)
    rho_r = float(np.mean([p.R.mean() for p in probs]))
    rho = float(np.mean([p.Q.mean() for p in probs]))
    if N >= 4:
        xlo, xhi = state_box(oracle, probs, 0.9, input_bounded_states(bs, ulo, uhi, rho_r))
    else:
        xlo, xhi, rho = None, None, rho_r
    bs.set_bounds(xlo, xhi, ulo, uhi)
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25)
    it0, st0 = bs.solve_box(**kw)
    assert (st0 == 1).all(), (it0, st0)
    bs.set_box_acceleration(MEM)
    it, st = bs.solve_box(**kw)
    accepted, rejected, _, _ = bs.box_acceleration()
    print("iterations: plain %s, accelerated %s (accepted %s, rejected %s)" % (it0.tolist(), it.tolist(), accepted.tolist(),
                                                                              rejected.tolist()))
    assert want is None or bs.schedule() == want, bs.schedule()
    assert (st == 1).all(), (it, st)
    sol, mux, muu = results(bs)
    inf = np.full((N, n), np.inf)
    for p in range(batch):
        check_certificate(probs[p], sol[p], mux[p], muu[p], -inf if xlo is None else xlo[p], inf if xhi is None else xhi[p],
                          ulo[p], uhi[p])
    assert int(it.sum()) < int(it0.sum()), (it, it0)
    bs.close()


# ------------------------------------------------------------------------------------------------ 5. independence

def test_problems_iterate_independently_and_a_warm_start_works(ndlqr, oracle):
    n, m, N, batch = 12, 4, 16, 3
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    for a in (ulo, xlo):
        a[1] = -np.inf
    for a in (uhi, xhi):
        a[1] = np.inf
    kw = dict(rho=float(np.mean([p.Q.mean() for p in probs])), alpha=ALPHA, eps_abs=1e-9, eps_rel=1e-9, max_iter=2000, check_every=1)
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(xlo, xhi, ulo, uhi)
    bs.set_box_acceleration(MEM)
    it, st = bs.solve_box(**kw)
    assert (st == 1).all() and it[1] == 1 and it[0] > 1 and it[2] > 1, (it, st)
    sol, mux, muu = results(bs)
    accepted = bs.box_acceleration()[0]
    assert accepted[1] == 0 and accepted[0] > 0 and accepted[2] > 0
    free = solver(ndlqr, [probs[1]], strict_flags(ndlqr))
    assert free.solve() == 0
    assert np.array_equal(sol[1], free.solutions()[0])  # the unconstrained solution
    free.close()
    for p in (0, 2):
        one = solver(ndlqr, [probs[p]], strict_flags(ndlqr))
        one.set_bounds(xlo[p], xhi[p], ulo[p], uhi[p])
        one.set_box_acceleration(MEM)
        it1, st1 = one.solve_box(**kw)
        assert it1[0] == it[p] and st1[0] == 1
        for x, y in zip(results(one), (sol[p:p + 1], mux[p:p + 1], muu[p:p + 1])):
            assert np.array_equal(x, y), p
        one.close()
    it2, st2 = bs.solve_box(warm_start=True, **kw)
    assert (st2 == 1).all() and (it2 <= 2).all(), (it2, st2)
    bs.close()


# ------------------------------------------------------------------------------------------------ 6. adaptive penalty

def test_with_the_adaptive_penalty(ndlqr, oracle):
    n, m, N, batch = 12, 4, 32, 3
    probs = [synth(ndlqr, n, m, N, 60 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.6)
    bs = solver(ndlqr, probs)
    rho = float(np.mean([p.R.mean() for p in probs]))
    xlo, xhi = state_box(oracle, probs, 0.7, input_bounded_states(bs, ulo, uhi, rho))
    bs.set_bounds(xlo, xhi, ulo, uhi)
    kw = dict(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, adapt_every=25)
    it0, st0 = bs.solve_box(**kw)
    assert (st0 == 1).all(), (it0, st0)
    bs.set_box_acceleration(MEM)
    it, st = bs.solve_box(**kw)
    print("iterations: adaptive %s, adaptive and accelerated %s, rho %s" % (it0.tolist(), it.tolist(), bs.box_penalties().tolist()))
    assert (st == 1).all(), (it, st)
    assert (bs.box_penalties() != rho).any()
    sol, mux, muu = results(bs)
    for p, prob in enumerate(probs):
        check_certificate(prob, sol[p], mux[p], muu[p], xlo[p], xhi[p], ulo[p], uhi[p])
    assert int(it.sum()) < int(it0.sum()), (it, it0)
    bs.close()


# ------------------------------------------------------------------------------------------------ 7. infeasibility detection

def test_with_infeasibility_detection(ndlqr, oracle, monkeypatch):
    """The two settings combine: the infeasible member of test_gpu_box_infeas's compact case is
    certified within that test's iteration budget, its certificate passes the long-double test, the others converge."""
    from test_gpu_box_infeas import EPS, EVERY, Case
    case = Case(ndlqr, oracle, "compact")
    bs = case.solver(ndlqr, monkeypatch)
    bs.set_bounds(*case.bounds)
    bs.set_box_infeasibility(EVERY, EPS)
    bs.set_box_acceleration(MEM)
    it, st = case.solve_box(bs)
    print("iterations %s, status %s (the plain reference certifies at %d)" % (it.tolist(), st.tolist(), case.ref[1]))
    assert st[1] == 4 and (np.delete(st, 1) == 1).all(), (it, st)
    assert it[1] % EVERY == 0 and it[1] <= case.max_iter
    case.check_certificate(bs, st)
    assert bs.box_acceleration()[0].sum() > 0
    bs.close()


# ------------------------------------------------------------------------------------------------ 8. torch
# In a fresh process that initialises torch's device first, as test_gpu_box_gradients._run_case.

def _case_torch(ndlqr, mode):
    """test_gpu_box_gradients._case_dense_reference with the keyword on: its problem, loss and tolerances"""
    import torch
    import test_gpu_box_gradients as G
    from rslqr_amd.autograd import lqr_solve_box
    n, m, N, batch = 6, 3, 16, 3
    t = G._torch_problem(ndlqr, n, m, N, batch, 2000)
    bnd = G._torch_bounds(t, n, m, N, batch, mode)
    leaves = dict(t, **bnd)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    kw = dict(rho=1.0, eps_abs=1e-11, eps_rel=1e-11, max_iter=20000, accel_mem=MEM)
    args = [t[k] for k in G.ARGS] + [bnd[k] for k in G.BOUNDS]
    z, got = G._grads12(lambda: lqr_solve_box(*args, **kw), leaves, gz)
    zr, ref = G._grads12(lambda: G._dense_box_solve(t, bnd, z, n, m, N, batch), leaves, gz)
    assert G.rel(z.cpu().numpy(), zr.cpu().numpy()) <= 1e-8
    for k in G.ARGS + G.BOUNDS:
        gr = ref[k] if ref[k] is not None else torch.zeros_like(got[k])
        assert G.rel(got[k].cpu().numpy(), gr.cpu().numpy()) <= 1e-6, (k, G.rel(got[k].cpu().numpy(), gr.cpu().numpy()))


def test_torch_keyword():
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_box_accel as T\n"
            "T._case_torch(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, json.dumps(["per_problem"])))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
