"""Box-constrained batch solve (ndlqr_BatchSetBounds, ndlqr_SolveBatchBoxConstrained, ndlqr_CopyBatchBoundMultipliers) on
the device against the independent references of box_support.py: the exact bvls solution of the condensed problem for
input bounds, an extended-precision optimality certificate plus the active-set QP for state bounds, and the numpy
restatement of the iteration driving the oracle for strict mode (bit for bit)."""
import numpy as np
import pytest

from box_support import active_set_qp, admm_reference, bvls_inputs, certificate, split
from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def stack(probs, keys=ARGS):
    return [np.stack([getattr(p, k) for p in probs]) for k in keys]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def solver(ndlqr, probs, flags=0):
    p = probs[0]
    bs = ndlqr.BatchSolver(p.n, p.m, p.N, len(probs), flags=flags)
    bs.initialize_flat(*stack(probs))
    return bs


def unconstrained(oracle, prob):
    return oracle.solve(prob, 1)[0][: prob.nvars]


def input_box(oracle, probs, frac):
    """symmetric input bounds at `frac` of the mean unconstrained |u| of each input channel, [batch, N, m]"""
    out = []
    for prob in probs:
        u = split(unconstrained(oracle, prob), prob.n, prob.m, prob.N)[2]
        out.append(np.tile(frac * np.abs(u).mean(axis=0), (prob.N, 1)))
    hi = np.stack(out)
    return -hi, hi


def state_box(oracle, probs, frac, xb=None):
    """symmetric state bounds at `frac` of the largest |x| of each state -- of the unconstrained solution, or of the
    states xb [batch, N, n] of the solution with input bounds alone --, widened where the trajectory of u = 0 (inside
    every input box here) needs more: feasible by construction, [batch, N, n]. Where xb leaves the box, the solution
    with state bounds has an active state bound (else, by convexity, it would be xb)."""
    out = []
    for i, prob in enumerate(probs):
        x = split(unconstrained(oracle, prob), prob.n, prob.m, prob.N)[1] if xb is None else xb[i]
        roll = np.zeros_like(x)
        roll[0] = prob.x0
        for k in range(prob.N - 1):
            roll[k + 1] = prob.A[k].reshape(prob.n, prob.n).T @ roll[k] + prob.d[k]
        out.append(np.maximum(np.tile(frac * np.abs(x[1:]).max(axis=0), (prob.N, 1)), 1.5 * np.abs(roll)))
    hi = np.stack(out)
    return -hi, hi


def input_bounded_states(bs, ulo, uhi, rho):
    """x [batch, N, n] of the solution with the input bounds alone (eps 1e-10)"""
    bs.set_bounds(None, None, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, check_every=25)
    assert (st == 1).all(), (it, st)
    n, m, N = bs.n, bs.m, bs.N
    return np.stack([split(z, n, m, N)[1] for z in bs.solutions()])


def assert_state_bounds_active(bs, sol, mux, xlo, xhi):
    """some state sits at one of its bounds with a nonzero multiplier"""
    x = np.stack([split(z, bs.n, bs.m, bs.N)[1] for z in sol])
    at = (x == xhi) | (x == xlo)
    at[:, 0] = False
    assert at.any(), "no state at a bound"
    assert (np.abs(mux[at]) > 1e-8).any(), "no state bound with a nonzero multiplier"


def check_certificate(prob, z, mux, muu, xlo, xhi, ulo, uhi, tol=1e-6):
    _, x, u = split(z, prob.n, prob.m, prob.N)
    cert = certificate(prob, z, mux, muu, xlo, xhi, ulo, uhi, tol)
    assert cert["stationarity"] <= tol and cert["bounds"] <= 0 and cert["complementarity"] <= tol, cert
    ua, _, _ = active_set_qp(prob, xlo, xhi, ulo, uhi, x, u, mux, muu, tol)
    assert rel(u[: prob.N - 1], ua) <= 1e-6


# ------------------------------------------------------------------------------------------------ 1. no active bounds

@pytest.mark.parametrize("strict", [False, True])
def test_no_finite_bounds_is_the_unconstrained_solve(ndlqr, oracle, strict):
    n, m, N, batch = 12, 4, 16, 3
    probs = [synth(ndlqr, n, m, N, 10 + p) for p in range(batch)]
    fl = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT if strict else 0
    bs = solver(ndlqr, probs, fl)
    assert bs.solve() == 0
    ref = bs.solutions().copy()
    inf = np.full((N, n), np.inf)
    bs.set_bounds(-inf, inf, None, None)
    it, st = bs.solve_box(max_iter=50)
    assert (it == 1).all() and (st == 1).all(), (it, st)
    sol = bs.solutions()
    if strict:
        assert np.array_equal(sol, ref)
    else:
        assert max(rel(sol[p], ref[p]) for p in range(batch)) <= REL_TOL
    # loose finite bounds (never active): the unconstrained solution to the tolerance
    big = 10.0 * np.abs(ref).max()
    bs.set_bounds(np.full(n, -big), np.full(n, big), np.full(m, -big), np.full(m, big))
    it, st = bs.solve_box(rho=float(probs[0].R.mean()), eps_abs=1e-12, eps_rel=1e-12, max_iter=3000)
    assert (st == 1).all(), (it, st)
    sol = bs.solutions()
    assert max(rel(sol[p], ref[p]) for p in range(batch)) <= 1e-8
    bs.close()


# ------------------------------------------------------------------------------------------------ 2. active input bounds

@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 8), (6, 3, 32, 4), (7, 9, 16, 2)])
def test_active_input_bounds_match_bvls(ndlqr, oracle, n, m, N, batch):
    probs = [synth(ndlqr, n, m, N, 40 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    bs = solver(ndlqr, probs)
    bs.set_bounds(None, None, ulo, uhi)
    it, st = bs.solve_box(rho=float(np.mean([p.R.mean() for p in probs])), eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    print("iterations", it.tolist())
    assert (st == 1).all(), (it, st)
    sol = bs.solutions()
    for p, prob in enumerate(probs):
        u = split(sol[p], n, m, N)[2]
        assert (u <= uhi[p][: N - 1]).all() and (u >= ulo[p][: N - 1]).all()
        ub, _ = bvls_inputs(prob, ulo[p], uhi[p])
        assert rel(u, ub) <= 1e-6, (p, rel(u, ub))
        assert (np.abs(u) == uhi[p][: N - 1]).mean() > 0.2  # a good fraction of the inputs at a bound
    bs.close()


# ------------------------------------------------------------------------------------------------ 3. state and input bounds

def test_state_and_input_bounds_pass_the_certificate(ndlqr, oracle):
    n, m, N, batch = 12, 4, 32, 4
    probs = [synth(ndlqr, n, m, N, 60 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.6)
    bs = solver(ndlqr, probs)
    rho = float(np.mean([p.R.mean() for p in probs]))
    xlo, xhi = state_box(oracle, probs, 0.7, input_bounded_states(bs, ulo, uhi, rho))
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    print("iterations", it.tolist())
    assert (st == 1).all(), (it, st)
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    assert_state_bounds_active(bs, sol, mux, xlo, xhi)
    for p, prob in enumerate(probs):
        check_certificate(prob, sol[p], mux[p], muu[p], xlo[p], xhi[p], ulo[p], uhi[p])
    bs.close()


# ------------------------------------------------------------------------------------------------ 4. strict bit-exactness

@pytest.mark.parametrize("iters", [1, 2, 3])
def test_strict_mode_is_the_numpy_restatement_bit_for_bit(ndlqr, oracle, iters):
    n, m, N, batch = 12, 4, 16, 2
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(batch)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    rho, alpha = 0.37, 1.6
    bs = solver(ndlqr, probs, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=rho, alpha=alpha, eps_abs=1e-300, eps_rel=1e-300, max_iter=iters)
    assert (it == iters).all() and (st == 2).all(), (it, st)
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    for p, prob in enumerate(probs):
        x, u, rx, ru, lam, rit, rst = admm_reference(prob, solve, xlo[p], xhi[p], ulo[p], uhi[p], rho, alpha, 1e-300, 1e-300,
                                                     iters)
        lg, xg, ug = split(sol[p], n, m, N)
        assert np.array_equal(xg, x) and np.array_equal(ug, u[: N - 1]) and np.array_equal(lg, lam), p
        assert np.array_equal(mux[p], rx) and np.array_equal(muu[p], ru), p
    bs.close()


# ------------------------------------------------------------------------------------------------ 5. every schedule

SCHEDULE_CASES = [(12, 4, 64, 160, "records", None, "reduced-compact-records"),
                  (12, 4, 64, 3, "records", "0", "reduced-compact-records"),
                  (12, 4, 256, 1, "records", None, "reduced-tree"),
                  (6, 3, 64, 3, "records", None, "reduced-tree"),
                  (32, 8, 128, 1, "records", None, "generic-reduced-records"),
                  (5, 2, 2, 3, "records", None, "generic-reduced-records"),
                  (6, 3, 4, 2, "records", None, "generic-reduced-records"),
                  (144, 16, 8, 1, "records", None, "generic-keep"),
                  (7, 9, 16, 2, "records", "0", "reduced-compact-records"),
                  (11, 3, 64, 2, "records", "0", "reduced-compact-records"),
                  (1, 1, 16, 3, "records", None, "reduced-tree"),
                  (2, 1, 64, 3, "records", None, "knot-lean"),
                  (20, 6, 32, 2, "fact", None, "generic-keep"),
                  (12, 4, 64, 2, "fact", None, "knot-keep"),
                  (6, 3, 4, 2, "fact", None, "generic-keep"),
                  (12, 4, 16, 2, "strict", None, "knot-strict"),
                  (20, 6, 16, 2, "strict", None, "generic-strict"),
                  (16, 4, 32, 2, "none", None, None)]


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
    # rho near diag R for input bounds alone; with active state bounds near diag Q (three times that for the large-block
    # case): at diag R these take over 6000 iterations to 1e-10, at diag Q 200-1000
    rho_r = float(np.mean([p.R.mean() for p in probs]))
    rho = float(np.mean([p.Q.mean() for p in probs])) * (3.0 if n > 128 else 1.0)
    if N >= 4:
        xlo, xhi = state_box(oracle, probs, 0.9, input_bounded_states(bs, ulo, uhi, rho_r))
    else:
        xlo, xhi, rho = None, None, rho_r
    bs.set_bounds(xlo, xhi, ulo, uhi)
    # (one of the 160 problems of the first case needs more than 6000 iterations: DESIGN.md section 3.9)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_every=25)
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


# ------------------------------------------------------------------------------------------------ 6. state rules

def test_state_rules(ndlqr, oracle):
    n, m, N, batch = 12, 4, 64, 4
    probs = [synth(ndlqr, n, m, N, 200 + p) for p in range(batch)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    before = bs.solutions().copy()
    ulo, uhi = input_box(oracle, probs, 0.5)
    bs.set_bounds(None, None, ulo, uhi)
    rho = float(np.mean([p.R.mean() for p in probs]))
    it, st = bs.solve_box(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    assert (st == 1).all()
    # the plain re-solves refuse the shifted records ...
    assert bs.solve_rhs_only() != 0
    assert bs.solve_adjoint(np.ones((batch, bs.nvars))) != 0
    # ... a plain solve is bit-identical to the one before and brings them back
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), before)
    assert bs.solve_rhs_only() == 0
    assert bs.solve_adjoint(np.ones((batch, bs.nvars))) == 0
    # the remembered shifted factorisation: a second constrained solve after new x0 factors nothing
    it, st = bs.solve_box(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)  # (factors: a plain solve came between)
    f0 = bs.factor_count()
    x0 = np.stack([0.5 * p.x0 for p in probs])
    bs.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    assert bs.factor_count() == f0
    assert (st == 1).all()
    warm_sol = bs.solutions().copy()
    cold = solver(ndlqr, [Problem(n, m, N, *(p.arrays()[:7] + (0.5 * p.x0,))) for p in probs], ndlqr.FLAG_KEEP_RECORDS)
    cold.set_bounds(None, None, ulo, uhi)
    cold.solve_box(rho=rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    assert max(rel(warm_sol[p], cold.solutions()[p]) for p in range(batch)) <= 1e-6
    cold.close()
    # a new rho refactors; warm start from a converged point takes at most 2 iterations
    it, st = bs.solve_box(rho=2 * rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    assert bs.factor_count() == f0 + 1
    it, st = bs.solve_box(rho=2 * rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000, warm_start=True)
    assert (it <= 2).all() and (st == 1).all(), it
    assert bs.factor_count() == f0 + 1
    # new inputs drop the remembered factorisation
    bs.initialize_flat(*stack(probs))
    bs.solve_box(rho=2 * rho, eps_abs=1e-9, eps_rel=1e-9, max_iter=6000)
    assert bs.factor_count() == f0 + 2
    # and resident inputs are untouched: the plain solve is still the one from before
    assert bs.solve() == 0
    assert np.array_equal(bs.solutions(), before)
    bs.close()


# ------------------------------------------------------------------------------------------------ 7. batch behaviour

def test_batch_behaviour(ndlqr, oracle):
    n, m, N, batch = 6, 3, 32, 4
    probs = [synth(ndlqr, n, m, N, 300 + p) for p in range(batch)]
    rho = float(np.mean([p.R.mean() for p in probs]))
    ulo, uhi = input_box(oracle, probs, 0.5)
    # mixed: problems 0 and 2 unbounded
    ulo_m, uhi_m = ulo.copy(), uhi.copy()
    ulo_m[[0, 2]] = -np.inf
    uhi_m[[0, 2]] = np.inf
    bs = solver(ndlqr, probs)
    bs.set_bounds(None, None, ulo_m, uhi_m)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, check_every=1)
    assert (st == 1).all() and it[0] == 1 and it[2] == 1 and it[1] > 1 and it[3] > 1, it
    # max_iter reached: status 2, no error
    it, st = bs.solve_box(rho=rho, eps_abs=1e-300, eps_rel=1e-300, max_iter=5)
    assert (it[[1, 3]] == 5).all() and (st[[1, 3]] == 2).all() and (st[[0, 2]] == 1).all(), (it, st)
    # shared bounds equal the same bounds per problem, bit for bit
    shared = uhi[0]
    bs.set_bounds(None, None, -shared, shared)
    bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    a = bs.solutions().copy()
    ma = bs.bound_multipliers()
    bs.set_bounds(None, None, np.broadcast_to(-shared, (batch, N, m)), np.broadcast_to(shared, (batch, N, m)))
    bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    assert np.array_equal(bs.solutions(), a)
    mb = bs.bound_multipliers()
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    # host, pinned and device pointers for bounds and multipliers
    for kind in ("pinned", "device"):
        if kind == "pinned":
            lo, hi = ndlqr.pinned_empty((batch, N, m)), ndlqr.pinned_empty((batch, N, m))
            lo[...] = -shared
            hi[...] = shared
            mux, muu = ndlqr.pinned_empty((batch, N, n)), ndlqr.pinned_empty((batch, N, m))
        else:
            lo = ndlqr.DeviceArray((batch, N, m)).set(np.broadcast_to(-shared, (batch, N, m)))
            hi = ndlqr.DeviceArray((batch, N, m)).set(np.broadcast_to(shared, (batch, N, m)))
            mux, muu = ndlqr.DeviceArray((batch, N, n)), ndlqr.DeviceArray((batch, N, m))
        bs.set_bounds(None, None, lo, hi)
        bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
        assert np.array_equal(bs.solutions(), a), kind
        bs.bound_multipliers(mux, muu)
        got = (mux.get(), muu.get()) if kind == "device" else (mux, muu)
        assert np.array_equal(got[0], ma[0]) and np.array_equal(got[1], ma[1]), kind
    # a warm start after a change of the bounded pattern: no multiplier on an entry that is no longer bounded
    lo2, hi2 = np.broadcast_to(-shared, (batch, N, m)).copy(), np.broadcast_to(shared, (batch, N, m)).copy()
    lo2[:, :, 0], hi2[:, :, 0] = -np.inf, np.inf
    assert (np.abs(ma[1][:, : N - 1, 0]) > 0).any()  # (input 0 was active before)
    bs.set_bounds(None, None, lo2, hi2)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, warm_start=True)
    assert (st == 1).all(), (it, st)
    assert (bs.bound_multipliers()[1][:, :, 0] == 0).all()
    bs.set_bounds(None, None, -shared, shared)
    bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    # lo > hi is refused, and the previous bounds stay
    with pytest.raises(RuntimeError):
        bs.set_bounds(None, None, shared, -shared - 1.0)
    bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    assert np.array_equal(bs.solutions(), a)
    bs.close()


# ------------------------------------------------------------------------------------------------ 8. MPC loop

def test_mpc_loop_with_warm_start(ndlqr, oracle):
    n, m, N, batch = 12, 4, 64, 16
    probs = [synth(ndlqr, n, m, N, 400 + p) for p in range(batch)]
    rho = float(np.mean([p.R.mean() for p in probs]))
    ulo, uhi = input_box(oracle, probs, 0.5)
    bs = solver(ndlqr, probs)
    bs.set_bounds(None, None, ulo[0], uhi[0])
    q, r, d = stack(probs, ("q", "r", "d"))
    x = np.stack([p.x0 for p in probs])
    counts = []
    for step in range(10):
        bs.set_rhs_flat(q, r, d, x)
        it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, warm_start=step > 0)
        assert (st == 1).all(), (step, it)
        counts.append(int(it.max()))
        sol = bs.solutions()
        u0 = np.stack([split(sol[p], n, m, N)[2][0] for p in range(batch)])
        assert (u0 <= uhi[0][0]).all() and (u0 >= ulo[0][0]).all()
        cold = solver(ndlqr, [Problem(n, m, N, *(p.arrays()[:7] + (x[i],))) for i, p in enumerate(probs)])
        cold.set_bounds(None, None, ulo[0], uhi[0])
        cold.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
        u0c = np.stack([split(cold.solutions()[p], n, m, N)[2][0] for p in range(batch)])
        cold.close()
        assert rel(u0, u0c) <= 1e-6, (step, rel(u0, u0c))
        x = np.stack([probs[p].A[0].reshape(n, n).T @ x[p] + probs[p].B[0].reshape(m, n).T @ u0[p] + probs[p].d[0]
                      for p in range(batch)])
    print("iterations per step", counts)
    bs.close()


# ------------------------------------------------------------------------------------------------ 9. failures

def test_non_positive_pivot_and_non_finite_data_are_reported(ndlqr, oracle):
    n, m, N, batch = 12, 4, 32, 3
    probs = [synth(ndlqr, n, m, N, 500 + p) for p in range(batch)]
    rho = float(np.mean([p.R.mean() for p in probs]))
    ulo, uhi = input_box(oracle, probs, 0.5)
    # problem 1 has Q <= 0 on a state entry that stays unbounded: the shift does not touch it
    bad = [Problem(n, m, N, *[a.copy() for a in p.arrays()]) for p in probs]
    bad[1].Q[5, 0] = -5.0
    bs = solver(ndlqr, bad)
    assert bs.solve() == ndlqr.api.ERR_NOT_SPD  # (the plain solve refuses the problem)
    bs.set_bounds(None, None, ulo, uhi)
    for _ in range(2):  # a failed shifted factorisation is not remembered: the second call factors (and fails) again
        f0 = bs.factor_count()
        assert bs.L.ndlqr_SolveBatchBoxConstrained(bs.h, None, None, None) == ndlqr.api.ERR_NOT_SPD
        assert bs.factor_count() == f0 + 1
        with pytest.raises(RuntimeError):  # no resident solution after it
            bs.solutions()
    assert bs.solve() == ndlqr.api.ERR_NOT_SPD  # (Q, R restored: the plain solve sees the same problem)
    # the same solver with valid data works again
    bs.initialize_flat(*stack(probs))
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000)
    assert (st == 1).all(), (it, st)
    # a NaN in the data of one problem: that problem stops as status 3, the others converge
    x0 = np.stack([p.x0 for p in probs])
    x0[2, 3] = np.nan
    bs.set_rhs_flat(*stack(probs, ("q", "r", "d")), x0)
    it, st = bs.solve_box(rho=rho, eps_abs=1e-10, eps_rel=1e-10, max_iter=6000, check_every=1)
    assert st[2] == 3 and it[2] == 1 and (st[:2] == 1).all(), (it, st)
    bs.close()
