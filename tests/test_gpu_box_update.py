"""The element-wise kernels every constrained solve runs in every iteration -- box_bounds, box_shift_qr, box_start,
box_update, box_finish, box_multipliers (kernels_box.hpp) and box_adjoint_update (kernels_box_grad.hpp) -- per entry and
per iteration, through the read-out of the convergence test (ndlqr_CopyBatchBoxResiduals,
ndlqr_CopyBatchBoxAdjointResiduals: r_prim | r_dual | sp | sd of every problem's last update) and against the numpy
restatement of box_update_support.py, which returns the state after every iteration. Acceleration stays off (mem = 0),
infeasibility detection off, the penalty fixed except in the one adaptive case of part a.

The shapes, by the 256-thread loop of box_update / box_adjoint_update over the N * w entries of a problem (w: the padded
n + m); test_box_update_host.py holds the same table against a restatement of the padding rules:

    shape (n, m, N)   padded     N * w   passes   chosen for
    (6, 3, 4)         --         36      1        idle threads
    (1, 1, 8)         (6, 3)     72      1        most entries are pad entries that must never count
    (12, 4, 16)       --         256     1        one exact pass
    (5, 2, 32)        --         224     1        (5, 2) is an instance of its own: not padded, one pass with 32 idle
                                                  threads and 7-entry knots that straddle the wavefronts
    (5, 3, 32)        (6, 3)     288     2        a padded instance with a short tail (32 entries in the second pass)
    (7, 9, 16)        (8, 16)    384     2        pad columns in the middle of a knot
    (20, 6, 16)       --         416     2        runtime-sized strict path
    (12, 4, 256)      --         4096    16       many passes
    (130, 5, 4)       (144, 8)   608     3        per-knot loops of five passes (box_start / box_finish over 296 rows) and
                                                  a padding beyond 128 states
    (12, 4, 64)       --         1024    4        part c only: compact records in fast mode

The mixed bound pattern (box_update_support.mixed_bounds): by (k + j) % 4 an entry has both bounds, the upper one only,
the lower one only or none, and one input has lo == hi. test_box_update_host.py asserts that every seed used here has
entries on lo, on hi, strictly inside and unbounded after each of the first three iterations.

Parts: a. strict mode per iteration, bit for bit (solution, multipliers, the four numbers, iters, status), per-problem
and shared bounds, and one adaptive case; b. warm starts with the same and with a changed pattern, termination with
check_every 1 and 7, the box adjoint; c. every entry counted once, fast and strict; d. fast mode against the restatement
over three iterations; e. the getters' destinations and refusals, and the rows of problems that are not iterated.

Fast mode, part d, measured on an MI355X: the largest error over the three iterations, both problems and the six
quantities (v, y, r_prim, r_dual, sp, sd), as a fraction of its bound 2 k 1e-9 ||z_ref||_2 (times rho for r_dual, sd):
    (6,3,4) 3.2e-7   (1,1,8) 6.8e-7   (12,4,16) 9.4e-7   (5,2,32) 3.2e-7   (5,3,32) 4.2e-7   (7,9,16) 2.8e-7
    (20,6,16) 7.9e-7   (12,4,256) 1.0e-6   (130,5,4) 3.8e-7
-- the fast re-solves are at rounding level on these problems, six orders inside what the project promises of them. Part c
measures |r_prim / D - 1| and |sd / (rho D) - 1| <= 2.3e-16 in both modes against its derived 1e-7.

Measured on an MI355X: the 50 cases take 2.3 s together; the slowest are the first case (0.32 s, it loads the library),
(130,5,4) of part a (0.17 s), (12,4,256) of part a and of the box adjoint (0.11 s each), the termination case
(12,4,16) with check_every 1 (0.10 s, 273 iterations) and (130,5,4) of part c (0.09 s).

What the cases catch, each change made once in a scratch build and this file run once against it, together with the
strict tests that existed before (test_gpu_box.py part 4 and test_batch_behaviour, test_gpu_box_gradients.py part 1,
test_gpu_residuals.py part 4, the strict test of test_gpu_box_adaptive.py); only changes that skip work or drop a term:
  1. the entry loop of box_update cut to its first pass: 21 cases fail -- every shape of two passes or more in parts a
     and d, (7,9,16) in the shared, warm-start and termination cases, (7,9,16), (130,5,4) and (12,4,64) in part c. Before:
     only the termination cases (7,9,16) and (20,6,16) of test_gpu_residuals.py; test_gpu_box.py part 4 passes.
  2. the LDS reduction started at s = 64: 35 cases fail, in every part but the box adjoint's (its kernel has a reduction
     of its own); (6,3,4) and (1,1,8), with fewer than 128 entries, pass as they should, and so does the same-pattern
     warm start at (7,9,16), whose maxima sit in the first 128 threads. Before: the two termination cases with 256 entries or more that stop
     early, and the adaptive strict test; test_gpu_box.py part 4 and test_gpu_box_gradients.py part 1 pass.
  3. the rhs_next = rhs_cur copy of a frozen problem removed: five termination cases fail ((12,4,16) and (7,9,16) with
     both check_every, (1,1,8) with 7). Before: three of the four termination cases and the adaptive strict test.
  4. y of an entry that is no longer bounded not zeroed by box_start: both changed-pattern warm starts fail. Before:
     test_batch_behaviour (through a converged solution).
  5. ym dropped from sd: 45 cases fail, everything that reads sd or a decision made from it. Before: three termination
     cases and the adaptive strict test; test_gpu_box.py part 4 passes (eps 1e-300 decides nothing).
  6. change 1 in box_adjoint_update: the box adjoint cases (7,9,16) and (12,4,256) fail. Before: nothing fails.
"""
import numpy as np
import pytest

from box_adaptive_support import admm_adaptive_reference
from box_grad_support import active_codes, bound_grads, full_bounds
from box_support import split
from box_update_support import (ALPHA, PLANT_RHO, RHO, addressable, adjoint_trace, forward_trace, loose_bounds, mixed_bounds,
                                oracle_solve, plant, planted, planted_positions, stack_bounds)
from test_gpu_box import solver, synth

pytestmark = pytest.mark.gpu

SHAPES = [(6, 3, 4), (1, 1, 8), (12, 4, 16), (5, 2, 32), (5, 3, 32), (7, 9, 16), (20, 6, 16), (12, 4, 256), (130, 5, 4)]
SHARED_SHAPES = [(12, 4, 16), (7, 9, 16)]
WARM_SHAPES = [(7, 9, 16), (5, 2, 32)]
TERMINATION_SHAPES = [(12, 4, 16), (7, 9, 16), (5, 2, 32), (1, 1, 8)]
TERMINATION = dict(eps=1e-4, max_iter=400)  # (seeds 80 and 81)
ADJOINT_SHAPES = [(12, 4, 16), (7, 9, 16), (5, 2, 32), (12, 4, 256)]
COUNT_SHAPES = [(12, 4, 16), (7, 9, 16), (1, 1, 8), (5, 2, 32), (130, 5, 4), (12, 4, 64)]
# the two problems of a case; (1, 1, 8) has twelve bounded entries, and seed 81 leaves none of them on its lower bound
# after the first iteration (test_box_update_host.py holds every pair to that condition)
SEEDS = {(1, 1, 8): (80, 92)}
ADAPT_SEEDS = (80, 85, 88)  # of the adaptive case: the first keeps its penalty at iteration 2, the others move it
REL_TOL = 1e-9  # what the project holds a fast solve to (relative l2)
BOUNDS = ("xlo", "xhi", "ulo", "uhi")


def strict_flags(ndlqr):
    return ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT


def ids(shapes):
    return ["%d.%d.%d" % s for s in shapes]


def delivered(tr, k, M, rho):
    """(x, u, mu_x, mu_u, lam) a solve delivers when iteration k of the trace is its last"""
    s = tr.its[k - 1]
    n = tr.x.shape[1]
    xu = np.where(M, s["v"], s["Z"][:, n:])
    mu = rho * s["y"]
    return xu[:, :n], xu[:, n:], mu[:, :n], mu[:, n:], s["Z"][:, :n]


def packed(prob, tr):
    """the solution vector [nvars] a trace delivers at its end"""
    return np.concatenate([tr.lam, tr.x, tr.u], axis=1).reshape(-1)[: prob.nvars]


_CASES = {}


def case(ndlqr, oracle, shape, seeds=None, **kw):
    """(problems, their mixed bounds) of one shape: computed once"""
    seeds = seeds or SEEDS.get(shape, (80, 81))
    key = (shape, seeds, tuple(sorted(kw.items())))
    if key not in _CASES:
        probs = [synth(ndlqr, *shape, s) for s in seeds]
        _CASES[key] = (probs, [mixed_bounds(oracle, p, **kw) for p in probs])
    return _CASES[key]


_TRACES = {}


def traces(ndlqr, oracle, shape, max_iter=3, eps=1e-300, seeds=None):
    """the restatement of every problem of a case: computed once, never changed"""
    key = (shape, max_iter, eps, seeds)
    if key not in _TRACES:
        probs, bounds = case(ndlqr, oracle, shape, seeds)
        solve = oracle_solve(oracle)
        _TRACES[key] = [forward_trace(p, solve, b, max_iter, eps=eps) for p, b in zip(probs, bounds)]
    return _TRACES[key]


def assert_delivered(bs, p, prob, want, tag):
    """solution and multipliers of problem p equal (x, u, mu_x, mu_u, lam) bit for bit"""
    n, m, N = prob.n, prob.m, prob.N
    x, u, rx, ru, lam = want
    lg, xg, ug = split(bs.solutions()[p], n, m, N)
    mux, muu = bs.bound_multipliers()
    assert np.array_equal(xg, x) and np.array_equal(ug, u[: N - 1]) and np.array_equal(lg, lam), tag
    assert np.array_equal(mux[p], rx) and np.array_equal(muu[p], ru), tag


def row_bytes(row):
    return np.asarray(row, dtype=np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ a. strict, per iteration

@pytest.mark.parametrize("n,m,N", SHAPES, ids=ids(SHAPES))
def test_strict_mode_per_iteration_bit_for_bit(ndlqr, oracle, n, m, N):
    """max_iter = 1, 2, 3 on the mixed pattern: solution, mu, the four numbers, iters and status are the restatement's"""
    probs, bounds = case(ndlqr, oracle, (n, m, N))
    trs = traces(ndlqr, oracle, (n, m, N))
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    if (n, m, N) == (130, 5, 4):  # (not among the strict cases of test_gpu_parity.py: what everything below rests on)
        assert bs.solve() == 0
        for p, prob in enumerate(probs):
            assert np.array_equal(bs.solutions()[p], oracle.solve(prob, 1)[0][: prob.nvars])
    bs.set_bounds(*stack_bounds(bounds))
    for iters in (1, 2, 3):
        it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
        assert (it == iters).all() and (st == 2).all(), (it, st)
        resid = bs.box_residuals()
        assert resid.shape == (len(probs), 4)
        for p, prob in enumerate(probs):
            M = full_bounds(n, m, N, *bounds[p])[2]
            assert_delivered(bs, p, prob, delivered(trs[p], iters, M, RHO), (iters, p))
            assert row_bytes(resid[p]) == row_bytes(trs[p].its[iters - 1]["resid"]), (iters, p, resid[p], trs[p].its[iters - 1]["resid"])
    bs.close()


@pytest.mark.parametrize("n,m,N", SHARED_SHAPES, ids=ids(SHARED_SHAPES))
def test_shared_bounds_are_the_same_bounds_per_problem(ndlqr, oracle, n, m, N):
    """the mixed pattern of problem 0 for both problems, once as shared bounds [N, .] (bstride 0 in box_shift_qr,
    box_start, box_update, box_finish) and once per problem: both are the restatement"""
    probs, bounds = case(ndlqr, oracle, (n, m, N))
    b0 = bounds[0]
    solve = oracle_solve(oracle)
    trs = [forward_trace(prob, solve, b0, 3) for prob in probs]
    M = full_bounds(n, m, N, *b0)[2]
    for given in (b0, stack_bounds([b0, b0])):
        bs = solver(ndlqr, probs, strict_flags(ndlqr))
        bs.set_bounds(*given)
        for iters in (1, 3):
            it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
            assert (it == iters).all() and (st == 2).all()
            resid = bs.box_residuals()
            for p, prob in enumerate(probs):
                assert_delivered(bs, p, prob, delivered(trs[p], iters, M, RHO), (given[0].ndim, iters, p))
                assert row_bytes(resid[p]) == row_bytes(trs[p].its[iters - 1]["resid"]), (given[0].ndim, iters, p)
        bs.close()


def test_adaptive_penalty_second_pass_on_the_mixed_pattern(ndlqr, oracle):
    """three iterations at (12,4,16) with adapt_every = 2: at iteration 2 the first problem keeps its penalty and the
    other two halve it (test_box_update_host.py), so the second pass of box_update rescales their y and rewrites their
    next right-hand side, and the read-out is that of the rule's restatement -- iteration 3 with the new penalty"""
    n, m, N = 12, 4, 16
    probs, bounds = case(ndlqr, oracle, (n, m, N), seeds=ADAPT_SEEDS)
    solve = oracle_solve(oracle)
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(*stack_bounds(bounds))
    for iters in (2, 3):
        it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters, adapt_every=2)
        assert (it == iters).all() and (st == 2).all()
        resid, pen = bs.box_residuals(), bs.box_penalties()
        for p, prob in enumerate(probs):
            its = []
            ref = admm_adaptive_reference(prob, solve, *bounds[p], RHO, ALPHA, 1e-300, 1e-300, iters, 2, trace=its)
            assert_delivered(bs, p, prob, ref[:5], (iters, p))
            assert pen[p] == ref[7] and (ref[7] != RHO) == (iters == 3 and p > 0), (iters, p, pen[p], ref[7])
            assert row_bytes(resid[p]) == row_bytes(its[-1]["resid"]), (iters, p)
    bs.close()


# ------------------------------------------------------------------------------------------------ b. continuing and stopping

@pytest.mark.parametrize("changed", [False, True], ids=["same-pattern", "changed-pattern"])
@pytest.mark.parametrize("n,m,N", WARM_SHAPES, ids=ids(WARM_SHAPES))
def test_warm_start_continues_the_restatement(ndlqr, oracle, n, m, N, changed):
    """two iterations, new bounds -- every finite one scaled by 0.9, and with `changed` one two-sided entry per knot
    turned unbounded --, two warm-started iterations: the restatement started from the first run's (v, y). The same
    pattern reuses the factorisation; a changed one zeroes y of the released entries, ignores their v and factors again."""
    probs, bounds = case(ndlqr, oracle, (n, m, N))
    first = traces(ndlqr, oracle, (n, m, N), 2)
    _, second = case(ndlqr, oracle, (n, m, N), scale=0.9, release=changed)
    solve = oracle_solve(oracle)
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(*stack_bounds(bounds))
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=2)
    for p, prob in enumerate(probs):
        M = full_bounds(n, m, N, *bounds[p])[2]
        assert_delivered(bs, p, prob, delivered(first[p], 2, M, RHO), ("first", p))
        if changed:  # (the released entries carry a multiplier that must go)
            M2 = full_bounds(n, m, N, *second[p])[2]
            assert (first[p].its[-1]["y"][M & ~M2] != 0).any()
    f0 = bs.factor_count()
    bs.set_bounds(*stack_bounds(second))
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=2, warm_start=True)
    assert (it == 2).all() and (st == 2).all()
    assert bs.factor_count() == f0 + (1 if changed else 0)
    resid = bs.box_residuals()
    for p, prob in enumerate(probs):
        tr = forward_trace(prob, solve, second[p], 2, start=first[p].state())
        M2 = full_bounds(n, m, N, *second[p])[2]
        assert_delivered(bs, p, prob, delivered(tr, 2, M2, RHO), ("second", p))
        assert row_bytes(resid[p]) == row_bytes(tr.resid), p
        cold = forward_trace(prob, solve, second[p], 2)
        assert row_bytes(cold.resid) != row_bytes(tr.resid)  # (the start matters)
    bs.close()


@pytest.mark.parametrize("check_every", [1, 7])
@pytest.mark.parametrize("n,m,N", TERMINATION_SHAPES, ids=ids(TERMINATION_SHAPES))
def test_termination_is_the_restatements(ndlqr, oracle, n, m, N, check_every):
    """eps 1e-4: the two problems stop by convergence at iteration counts of their own (test_box_update_host.py pins
    them). iters, status, solution, multipliers and the read-out row are the restatement's at its last iteration: the
    problem frozen first keeps its row, and the re-solves of the iterations the other one still takes (and, with
    check_every = 7, of those before the host looks) reproduce its z -- lambda is delivered from the last of them."""
    probs, bounds = case(ndlqr, oracle, (n, m, N), seeds=(80, 81))
    trs = traces(ndlqr, oracle, (n, m, N), TERMINATION["max_iter"], TERMINATION["eps"], seeds=(80, 81))
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(*stack_bounds(bounds))
    eps = TERMINATION["eps"]
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=eps, eps_rel=eps, max_iter=TERMINATION["max_iter"], check_every=check_every)
    print("iterations", it.tolist(), "restatement", [t.iters for t in trs])
    resid = bs.box_residuals()
    for p, prob in enumerate(probs):
        tr = trs[p]
        assert (it[p], st[p]) == (tr.iters, tr.status) and tr.status == 1, (p, it[p], st[p], tr.iters, tr.status)
        M = full_bounds(n, m, N, *bounds[p])[2]
        assert_delivered(bs, p, prob, delivered(tr, tr.iters, M, RHO), p)
        assert row_bytes(resid[p]) == row_bytes(tr.resid), (p, resid[p], tr.resid)
        assert resid[p][0] <= eps + eps * resid[p][2] and resid[p][1] <= eps + eps * resid[p][3]
    assert it[0] != it[1]
    bs.close()


@pytest.mark.parametrize("n,m,N", ADJOINT_SHAPES, ids=ids(ADJOINT_SHAPES))
def test_box_adjoint_per_iteration_bit_for_bit(ndlqr, oracle, n, m, N):
    """three forward iterations on the mixed pattern (status 2), then the box adjoint with max_iter = 1, 3: w, the bound
    gradients per problem and summed, and the adjoint's read-out row are adjoint_admm_reference's"""
    probs, bounds = case(ndlqr, oracle, (n, m, N))
    solve = oracle_solve(oracle)
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(*stack_bounds(bounds))
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=3)
    assert (st == 2).all()
    sol = bs.solutions().copy()
    forward_row = bs.box_residuals().copy()
    g = np.random.default_rng(7).standard_normal((len(probs), bs.nvars))
    with pytest.raises(RuntimeError):
        bs.box_adjoint_residuals()  # no box adjoint of this solution yet
    for iters in (1, 3):
        ait, ast = bs.solve_box_adjoint(g, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
        assert (ait == iters).all() and (ast == 2).all()
        w = bs.adjoint()
        bg = bs.bound_gradients()
        summed = bs.bound_gradients(summed=True)
        resid = bs.box_adjoint_residuals()
        for p, prob in enumerate(probs):
            codes = active_codes(prob, sol[p], *bounds[p])
            assert set(np.unique(codes)) == {0, 1, 2, 3}, p
            at = adjoint_trace(prob, solve, codes, g[p], iters)
            assert np.array_equal(w[p], at.w), (iters, p)
            bref = bound_grads(codes, at.nu, n)
            for k in BOUNDS:
                assert np.array_equal(bg[k][p], bref[k]), (iters, p, k)
            assert any(np.abs(bref[k]).max() > 0 for k in BOUNDS)
            assert row_bytes(resid[p]) == row_bytes(at.resid), (iters, p, resid[p], at.resid)
        for k in BOUNDS:  # the batch sum: the problems added in order
            acc = np.zeros_like(bg[k][0])
            for p in range(len(probs)):
                acc = acc + bg[k][p]
            assert np.array_equal(summed[k], acc), (iters, k)
        assert row_bytes(bs.box_residuals()) == row_bytes(forward_row)  # (the forward's rows are its own)
    bs.close()


# ------------------------------------------------------------------------------------------------ c. every entry counted once

@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
@pytest.mark.parametrize("n,m,N", COUNT_SHAPES, ids=ids(COUNT_SHAPES))
def test_update_counts_every_entry_once(ndlqr, oracle, n, m, N, strict):
    """Every addressable entry bounded by +-B, alpha 1, rho 0.25, one iteration from a cold start: with z the solution of
    the shifted problem the loose entries give v+ = z, y+ = 0 exactly -- 0 in r_prim and in sd. One entry e of problem
    1 of 3 pinned at c = z_e + D (D a power of two >= 16 max |z|, B = 4 D) then carries all four numbers:
        r_dual == rho |c| and sp == |c| exactly; r_prim = |z_e - c| and sd = rho |z_e - c|, D and rho D up to the error of z_e.
    Fast mode: against the oracle's z within 1e-7 -- derived, not measured: a fast solve is held to 1e-9 relative l2,
    nvars <= 5000, so the error of z_e is below 1e-9 sqrt(5000) max |z| <= 5e-9 D. Strict mode: exact, against the z the
    solver itself delivers for the unpinned problem (v = z on loose entries), which is the oracle's bit for bit wherever
    the strict solve is ((130,5,4) included: part a asserts it). The rows of problems 0 and 2 do not move, nothing is
    factored again, and a pin on x of knot 0 or u of the last knot -- entries that are not entries -- moves no row at all.
    One position probes zm: lo == hi == 0 at the arg-max of |z| leaves sp = |z_e| to max |z| alone."""
    seeds = (80, 81, 82)
    probs = [synth(ndlqr, n, m, N, s) for s in seeds]
    zs, Ds = zip(*[planted(oracle, p)[:2] for p in probs])
    D = max(Ds)
    B = 4.0 * D
    z_ref = zs[1]
    loose = [loose_bounds(p, B) for p in probs]
    bs = solver(ndlqr, probs, strict_flags(ndlqr) if strict else 0)
    args = dict(rho=PLANT_RHO, alpha=1.0, eps_abs=1e-300, eps_rel=1e-300, max_iter=1)

    def run(b1):
        bs.set_bounds(*stack_bounds([loose[0], b1, loose[2]]))
        it, st = bs.solve_box(**args)
        assert (it == 1).all() and (st == 2).all()
        return bs.box_residuals().copy()

    base = run(loose[1])
    lam_own, x_own, u_own = split(bs.solutions()[1], n, m, N)
    z_own = np.concatenate([x_own, np.concatenate([u_own, np.zeros((1, m))])], axis=1)
    A = addressable(n, m, N)
    for p in range(3):  # the unpinned rows: r_prim = 0, r_dual = rho max |z|, sp = max |z|, sd = 0
        assert base[p][0] == 0.0 and base[p][3] == 0.0 and base[p][1] == PLANT_RHO * base[p][2]
        assert abs(base[p][2] / np.abs(zs[p][A]).max() - 1.0) <= 1e-7
    if strict:
        assert base[1][2] == np.abs(z_own[A]).max()
        assert np.array_equal(z_own[A], z_ref[A])
    f0 = bs.factor_count()
    worst = 0.0
    for k, j in planted_positions(n, m, N):
        c = z_ref[k, j] + D
        rows = run(plant(loose[1], n, k, j, c))
        assert row_bytes(rows[0]) == row_bytes(base[0]) and row_bytes(rows[2]) == row_bytes(base[2]), (k, j)
        r_prim, r_dual, sp, sd = rows[1]
        assert r_dual == PLANT_RHO * abs(c) and sp == abs(c), (k, j, rows[1], c)
        worst = max(worst, abs(r_prim / D - 1.0), abs(sd / (PLANT_RHO * D) - 1.0))
        assert abs(r_prim / D - 1.0) <= 1e-7 and abs(sd / (PLANT_RHO * D) - 1.0) <= 1e-7, (k, j, rows[1], D)
        if strict:
            assert r_prim == abs(z_own[k, j] - c) and sd == PLANT_RHO * abs(z_own[k, j] - c), (k, j, rows[1])
    print("largest |r_prim / D - 1|, |sd / (rho D) - 1|: %.2e" % worst)
    # entries that are not entries
    for k, j in ((0, 0), (0, n - 1), (N - 1, n), (N - 1, n + m - 1)):
        rows = run(plant(loose[1], n, k, j, z_ref.max() + D))
        assert row_bytes(rows) == row_bytes(base), (k, j)
    # zm
    k, j = np.unravel_index(np.argmax(np.where(A, np.abs(z_ref), -1.0)), z_ref.shape)
    rows = run(plant(loose[1], n, int(k), int(j), 0.0))
    assert row_bytes(rows[0]) == row_bytes(base[0]) and row_bytes(rows[2]) == row_bytes(base[2])
    assert abs(rows[1][2] / abs(z_ref[k, j]) - 1.0) <= 1e-7 and abs(rows[1][0] / abs(z_ref[k, j]) - 1.0) <= 1e-7
    if strict:
        assert rows[1][2] == abs(z_own[k, j]) == rows[1][0]
    assert bs.factor_count() == f0
    bs.close()


# ------------------------------------------------------------------------------------------------ d. fast mode, three iterations

@pytest.mark.parametrize("n,m,N", SHAPES, ids=ids(SHAPES))
def test_fast_mode_follows_the_restatement(ndlqr, oracle, n, m, N):
    """After iteration k = 1, 2, 3 on the mixed pattern, over the bounded entries,
        ||v - v_ref||_2 and ||y - y_ref||_2 <= 2 k 1e-9 ||z_ref||_2.
    Derivation: for 0 < alpha < 2 the map w = v + y -> w+ is nonexpansive (Douglas-Rachford), and so are w -> clip(w) = v
    and w -> w - clip(w) = y; each re-solve enters with alpha <= 2 times its own error, which the project holds to
    1e-9 relative l2. The four numbers are max-norms of differences of such vectors, so their error is at most the l2
    bound, times rho for r_dual and sd. (y is read as mu / rho: one rounding, 1e-16 relative.)"""
    probs, bounds = case(ndlqr, oracle, (n, m, N))
    trs = traces(ndlqr, oracle, (n, m, N))
    bs = solver(ndlqr, probs, 0)
    bs.set_bounds(*stack_bounds(bounds))
    worst = 0.0
    for iters in (1, 2, 3):
        it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
        assert (it == iters).all() and (st == 2).all()
        sol = bs.solutions()
        mux, muu = bs.bound_multipliers()
        resid = bs.box_residuals()
        for p, prob in enumerate(probs):
            M = full_bounds(n, m, N, *bounds[p])[2]
            s = trs[p].its[iters - 1]
            bound = 2 * iters * REL_TOL * np.linalg.norm(s["Z"])
            _, xg, ug = split(sol[p], n, m, N)
            v = np.concatenate([xg, np.concatenate([ug, np.zeros((1, m))])], axis=1)
            y = np.concatenate([mux[p], muu[p]], axis=1) / RHO
            ev, ey = np.linalg.norm((v - s["v"])[M]), np.linalg.norm((y - s["y"])[M])
            er = np.abs(resid[p] - np.array(s["resid"])) / np.array([1.0, RHO, 1.0, RHO])
            ratios = [ev / bound, ey / bound] + (er / bound).tolist()
            print("(%d,%d,%d) problem %d iteration %d: error / bound of v, y, r_prim, r_dual, sp, sd = %s"
                  % (n, m, N, p, iters, " ".join("%.1e" % r for r in ratios)))
            worst = max(worst, max(ratios))
            assert ev <= bound and ey <= bound, (iters, p, ev, ey, bound)
            assert (er <= bound).all(), (iters, p, resid[p], s["resid"], bound)
    print("(%d,%d,%d) largest error / bound: %.2e" % (n, m, N, worst))
    bs.close()


# ------------------------------------------------------------------------------------------------ e. the getters

def test_read_out_destinations_refusals_and_rows_of_problems_not_iterated(ndlqr, oracle):
    n, m, N, batch = 6, 3, 4, 3
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(batch)]
    bounds = [mixed_bounds(oracle, p) for p in probs]
    inf = [np.full((N, n), np.inf), np.full((N, m), np.inf)]
    bounds[1] = (-inf[0], inf[0], -inf[1], inf[1])  # problem 1: no bounded entry
    bs = solver(ndlqr, probs, strict_flags(ndlqr))
    bs.set_bounds(*stack_bounds(bounds))
    with pytest.raises(RuntimeError):
        bs.box_residuals()  # no constrained solve yet
    assert bs.solve() == 0
    with pytest.raises(RuntimeError):
        bs.box_residuals()
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=3, check_every=1)
    assert it.tolist() == [3, 1, 3] and st.tolist() == [2, 1, 2]
    rows = bs.box_residuals()
    assert (rows[1] == 0).all() and (rows[[0, 2]][:, :3] > 0).all()  # (converges at iteration 1 with a row of zeros)
    # host, pinned and device destinations
    pinned = ndlqr.pinned_empty((batch, 4))
    bs.box_residuals(pinned)
    dev = ndlqr.DeviceArray((batch, 4))
    bs.box_residuals(dev)
    assert row_bytes(pinned) == row_bytes(rows) and row_bytes(dev.get()) == row_bytes(rows)
    L = bs.L
    assert L.ndlqr_CopyBatchBoxResiduals(bs.h, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_CopyBatchBoxAdjointResiduals(bs.h, None) == ndlqr.api.ERR_INVALID
    # the box adjoint: refused before it ran, nonzero rows for the iterated problems afterwards
    with pytest.raises(RuntimeError):
        bs.box_adjoint_residuals()
    g = np.random.default_rng(3).standard_normal((batch, bs.nvars))
    bs.solve_box_adjoint(g, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=2)
    arows = bs.box_adjoint_residuals()
    assert (arows[[0, 2]][:, 2] > 0).all() and (arows[1] == 0).all()
    adev = ndlqr.DeviceArray((batch, 4))
    bs.box_adjoint_residuals(adev)
    assert row_bytes(adev.get()) == row_bytes(arows)
    assert row_bytes(bs.box_residuals()) == row_bytes(rows)
    # new bounds: the resident solution is no longer that of a constrained solve with the current bounds (the box adjoint
    # refuses it too); the adjoint that ran stays readable, as its bound gradients do
    bs.set_bounds(*stack_bounds(bounds))
    with pytest.raises(RuntimeError):
        bs.box_residuals()
    assert row_bytes(bs.box_adjoint_residuals()) == row_bytes(arows)
    # a NaN in the data of problem 2: frozen as status 3 at iteration 1 with its NaN stored as it is; the box adjoint
    # does not iterate it and reports a row of zeros (not what the adjoint before left there)
    from test_gpu_box import stack
    x0 = np.stack([p.x0 for p in probs])
    x0[2, 1] = np.nan
    bs.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
    it, st = bs.solve_box(rho=RHO, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=3, check_every=1)
    assert it.tolist() == [3, 1, 1] and st.tolist() == [2, 1, 3]
    nan_rows = bs.box_residuals()
    assert np.isnan(nan_rows[2]).any() and row_bytes(nan_rows[:2]) == row_bytes(rows[:2])
    ait, ast = bs.solve_box_adjoint(g, alpha=ALPHA, eps_abs=1e-300, eps_rel=1e-300, max_iter=2)
    assert ast.tolist() == [2, 1, 3]
    arows2 = bs.box_adjoint_residuals()
    assert (arows2[2] == 0).all() and row_bytes(arows2[:2]) == row_bytes(arows[:2])
    bs.close()
