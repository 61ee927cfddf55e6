"""box_certify (kernels_box_infeas.hpp) tested as what it is -- a function of two consecutive
iterates -- in every launch class, through its read-out (ndlqr_CopyBatchInfeasibilityMeasures): the four numbers it
decides on, E = ||e||_inf, D = ||dmu||_inf, I = the largest |dmu_i| toward an infinite bound and S, against the plain
high-precision evaluation of box_infeas_measures_support.measures_reference.

The inputs of a check come from the public API alone. For a check at iteration K, two solvers with the same data and
settings run K - 1 and K iterations (eps_abs = eps_rel = 1e-300: both end as status 2; detection every K, so the second
run's only check is at it == max_iter). Repeated solves are bitwise identical, so the first run is the second's state one
iteration earlier: dlam is the difference of their lambda (solutions()), dmu that of their bound_multipliers(), which
forms rho y as the kernel does -- the kernel's dlam and dmu bit for bit. K = 4, alpha = 1.6, rho = the mean of diag Q.

The launch classes (G knots per pass; test_box_infeas_measures_host.py holds the table against a restatement of
certify_group and the kernel's loops):

    shape (n, m, N)   padded     w     G    passes        chosen for
    (12, 4, 16)       --         16    16   16            one pass of exactly 256 tasks, no knot behind it
    (12, 4, 32)       --         16    16   16, 16        two full passes, dlam of the knot behind the first
    (13, 4, 16)       --         17    15   15, 1         a tail pass of one knot
    (20, 6, 16)       --         26    9    9, 7          passes of 9 + 7
    (7, 9, 16)        (8, 16)    24    10   10, 6         small padded block: pad columns are no entries
    (1, 1, 8)         (6, 3)     9     28   8             the smallest padded instance
    (64, 16, 8)       --         80    3    3, 3, 2       a dlam load of exactly 256
    (96, 16, 4)       --         112   2    2, 2          strided dlam load (288)
    (144, 16, 4)      --         160   1    1, 1, 1, 1    one knot per pass, strided load
    (130, 5, 4)       (144, 8)   152   1    1, 1, 1, 1    padding beyond 128 states
    (256, 32, 2)      --         288   1    1, 1          w >= 256: strided task loop, load of 512

Every shape solves in both modes (beyond 128 states fast mode keeps the factor array instead of records), so none is
left out.

Measured on an MI355X: the 29 cases take 2.3 s together; the slowest are the first case (0.28 s, it loads the library),
part 2 at (130, 5, 4) and (256, 32, 2) (0.26 and 0.21 s: 21 pairs of solves each resp. 9) and part 1 at (256, 32, 2) in
fast mode (0.14 s). A case runs 2 K - 1 = 7 iterations (11 with K = 6), and the reference side one oracle solve per
problem, for the unconstrained solution that places the bounds.

What the cases catch, each change made once in a scratch build of box_certify and the file run once against it (every
change only skips work or reads LDS the kernel owns):
  - the task loop of a pass without its stride: the three cases at (256, 32, 2) fail -- part 1 in both modes, part 2;
  - the dlam load without its stride: the 10 cases at the four shapes with nl * n > 256 fail -- part 1 in both modes at
    (96, 16, 4), (144, 16, 4), (130, 5, 4) and (256, 32, 2), part 2 at the last two;
  - the knot loop ended after its first pass: 22 cases fail -- part 1 in both modes at the nine shapes of two passes or
    more (all but (12, 4, 16) and (1, 1, 8)), part 2 at its three shapes, the adaptive case;
  - nl = nk, the knot behind a pass never loaded: 20 cases fail -- part 1 at eight of those nine shapes in either mode
    (all but (13, 4, 16) in fast and (7, 9, 16) in strict mode, where the row of LDS read instead leaves the maximum where
    it was), part 2 at its three shapes, the adaptive case.
test_infeasible_member_is_certified_in_every_family (test_gpu_box_infeas.py) passes in all eight families under the first
two; under the last two its padded and strict-generic cases fail (problem 1 is never certified), the other six pass.
"""
import functools

import numpy as np
import pytest

from box_infeas_measures_support import conditions, measures_reference
from box_support import blocks, split
from support import Problem

pytestmark = pytest.mark.gpu

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
K, ALPHA, EPS, SEED0, TINY = 4, 1.6, 1e-4, 2100, 1e-300
SHAPES = [(12, 4, 16), (12, 4, 32), (13, 4, 16), (20, 6, 16), (7, 9, 16), (1, 1, 8), (64, 16, 8), (96, 16, 4), (144, 16, 4),
          (130, 5, 4), (256, 32, 2)]
ENTRY_SHAPES = [(12, 4, 32), (130, 5, 4), (256, 32, 2)]
ENTRY_SEED = {(12, 4, 32): 2110, (130, 5, 4): 2110, (256, 32, 2): 2110}  # (chosen on the CPU: see part 2)


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def stack(probs, keys=ARGS):
    return [np.stack([getattr(p, k) for p in probs]) for k in keys]


class Data:
    """batch problems of one shape, their unconstrained x [N, n], u [N - 1, m] (one oracle solve each), rho, and the bounds
    of part 1: |u| <= half the mean unconstrained |u| of the channel, every state of the knots >= 1 within 0.7 of its
    unconstrained range"""

    def __init__(self, ndlqr, oracle, n, m, N, batch, seed):
        self.n, self.m, self.N, self.batch = n, m, N, batch
        self.probs = [synth(ndlqr, n, m, N, seed + p) for p in range(batch)]
        self.rho = float(np.mean([p.Q.mean() for p in self.probs]))
        self.x, self.u = [], []
        for prob in self.probs:
            _, x, u = split(oracle.solve(prob, 1)[0][: prob.nvars], n, m, N)
            self.x.append(x.copy())
            self.u.append(u.copy())
        uhi = np.stack([np.tile(0.5 * np.abs(u).mean(axis=0), (N, 1)) for u in self.u])
        xhi = np.stack([np.tile(0.7 * np.abs(x[1:]).max(axis=0), (N, 1)) for x in self.x])
        self.bounds = [-xhi, xhi, -uhi, uhi]

    def of(self, bounds, p):
        return [a[p] for a in bounds]


@functools.lru_cache(maxsize=None)
def _data(ndlqr, oracle, n, m, N, batch=3, seed=SEED0):
    return Data(ndlqr, oracle, n, m, N, batch, seed)


class Pair:
    """two solvers with the same data: run A stops one iteration before the check, run B at it"""

    def __init__(self, ndlqr, data, strict):
        fl = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT if strict else ndlqr.FLAG_KEEP_RECORDS
        self.data = data
        self.solvers = [ndlqr.BatchSolver(data.n, data.m, data.N, data.batch, flags=fl) for _ in range(2)]
        for bs in self.solvers:
            bs.initialize_flat(*stack(data.probs))

    def check(self, bounds, k=K, every=None, eps_admm=TINY, **kw):
        """both runs with these bounds; returns a dict: dlam, dmu_x, dmu_u [batch, N, .], measures [batch, 4], at, and run
        B's iterations, status and certificate"""
        d = self.data
        out = []
        for bs, max_iter in zip(self.solvers, (k - 1, k)):
            bs.set_bounds(*bounds)
            bs.set_box_infeasibility(k if every is None else every, EPS)
            args = dict(rho=d.rho, alpha=ALPHA, eps_abs=eps_admm, eps_rel=eps_admm, max_iter=max_iter, check_every=k)
            args.update(kw)
            it, st = bs.solve_box(**args)
            lam = np.stack([blocks(z, d.n, d.m, d.N)[:, : d.n] for z in bs.solutions()])
            mux, muu = bs.bound_multipliers()
            out.append((it, st, lam.copy(), mux.copy(), muu.copy()))
        (_, _, lam_a, mux_a, muu_a), (it, st, lam_b, mux_b, muu_b) = out
        measures, at = self.solvers[1].infeasibility_measures()
        return {"dlam": lam_b - lam_a, "dmu_x": mux_b - mux_a, "dmu_u": muu_b - muu_a, "measures": measures, "at": at,
                "it": it, "st": st, "cert": self.solvers[1].infeasibility_certificate(), "first": out[0]}

    def close(self):
        for bs in self.solvers:
            bs.close()


def assert_measures(prob, bounds, got, p, k=K, where=None):
    """the read-out of problem p against the reference on the same differences; returns the reference"""
    ref = measures_reference(prob, bounds, got["dlam"][p], got["dmu_x"][p], got["dmu_u"][p])
    E, D, I, S = got["measures"][p]
    print("  problem %d%s: E %.17g (ref %.17g, tol %.3g)  D %.17g  I %.17g  S %.17g (ref %.17g, tol %.3g, %d terms)"
          % (p, "" if where is None else " " + str(where), E, ref["E"], ref["tol_E"], D, I, S, ref["S"], ref["tol_S"],
             ref["terms"]))
    assert got["at"][p] == k, (where, p, got["at"])
    assert D == ref["D"] and I == ref["I"], (where, p, D, ref["D"], I, ref["I"])
    assert abs(E - ref["E"]) <= ref["tol_E"], (where, p, E, ref["E"], ref["tol_E"])
    assert abs(S - ref["S"]) <= ref["tol_S"], (where, p, S, ref["S"], ref["tol_S"])
    return ref


def assert_undecided(ref, got, p):
    """status 2 and a zero certificate, unless the reference's four conditions hold at 2 eps"""
    if conditions(ref, 2 * EPS):
        return
    assert got["st"][p] == 2 and got["it"][p] == got["at"][p], (p, got["st"], got["it"])
    assert not any(c[p].any() for c in got["cert"]), p


# ------------------------------------------------------------------------------------------ 1. every launch class

@pytest.mark.parametrize("n,m,N", SHAPES)
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_measures_in_every_launch_class(ndlqr, oracle, n, m, N, strict):
    data = _data(ndlqr, oracle, n, m, N)
    pair = Pair(ndlqr, data, strict)
    got = pair.check(data.bounds)
    print((n, m, N), "strict" if strict else "fast", "schedule", pair.solvers[1].schedule())
    assert got["first"][1].tolist() == [2] * data.batch and got["first"][0].tolist() == [K - 1] * data.batch
    for p, prob in enumerate(data.probs):
        ref = assert_measures(prob, data.of(data.bounds, p), got, p)
        assert ref["D"] > 0 and ref["E"] > 0, (p, ref)
        assert_undecided(ref, got, p)
    pair.close()


# ------------------------------------------------------------------------------------------ 2. one entry at a time

def entry_positions(n, m, N):
    """("x" | "u", knot, entry): the first and last state of knot 1, of a middle knot and of knot N - 1; the first and
    last input of knot 0 and of knot N - 2"""
    pos = [("x", k, i) for k in sorted({1, max(1, N // 2), N - 1}) for i in sorted({0, n - 1})]
    return pos + [("u", k, i) for k in sorted({0, N - 2}) for i in sorted({0, m - 1})]


def entry_bounds(data, kind, k, i, frac=0.5):
    """the bounds of part 1 for problems 0 and 2; problem 1 unbounded but for one entry (kind None: none at all), bounded at
    `frac` of its unconstrained value on that value's own side"""
    b = [a.copy() for a in data.bounds]
    for a, v in zip(b, (-np.inf, np.inf, -np.inf, np.inf)):
        a[1] = v
    if kind is not None:
        v = float((data.x if kind == "x" else data.u)[1][k, i])
        assert v != 0.0
        lo, hi = (b[0], b[1]) if kind == "x" else (b[2], b[3])
        (hi if v > 0 else lo)[1, k, i] = frac * v
    return b


@pytest.mark.parametrize("n,m,N", ENTRY_SHAPES)
def test_certify_counts_every_entry_once(ndlqr, oracle, n, m, N):
    """Fast mode, problem 1 with a single bounded entry, at half its unconstrained value on its own side: D is that
    entry's |dmu| -- zero if the kernel misses it --, E and S keep their bounds, and the other problems' numbers are those
    of a run without that bound, bit for bit.

    I > 0 -- a dmu that points to the infinite side of its entry -- needs a multiplier that recedes between iterations 3
    and 4. On the CPU, with the strict restatement: at (12, 4, 32) and seed 2110 both inputs of knot 0 do that under the
    bound at half the value. At (130, 5, 4) and (256, 32, 2) no position did for any of 760 seeds (2100 .. 6000): with a
    horizon that short against that many states every entry is stiff, h > 0.6 rho for its curvature h in the reduced
    problem, and the multiplier of an active bound then climbs monotonically (its error shrinks by 1 - alpha rho / (h + rho)
    in (0, 1) per iteration). So every shape runs its positions a second time with the bound AT the unconstrained value: it
    binds in the first, over-relaxed iterations only, the multiplier recedes, and I > 0 at 8 of 10 positions of
    (130, 5, 4) and at all 4 of (256, 32, 2), the input columns j >= 256 among them. There D may be zero (a multiplier
    already back at zero); the numbers keep their bounds all the same."""
    data = _data(ndlqr, oracle, n, m, N, 3, ENTRY_SEED[(n, m, N)])
    pair = Pair(ndlqr, data, False)
    base = pair.check(entry_bounds(data, None, 0, 0))
    # (without a bounded entry problem 1 has nothing to iterate on: converged at iteration 1, never examined)
    assert base["st"].tolist() == [2, 1, 2] and base["at"].tolist() == [K, 0, K] and not base["measures"][1].any(), base
    others = [0, 2]
    toward_inf = {0.5: [], 1.0: []}
    for frac in (0.5, 1.0):
        for kind, k, i in entry_positions(n, m, N):
            bounds = entry_bounds(data, kind, k, i, frac)
            got = pair.check(bounds)
            ref = assert_measures(data.probs[1], data.of(bounds, 1), got, 1, where=(frac, kind, k, i))
            dm = got["dmu_x"][1][k, i] if kind == "x" else got["dmu_u"][1][k, i]
            assert ref["D"] == abs(dm), (frac, kind, k, i)
            assert np.count_nonzero(got["dmu_x"][1]) + np.count_nonzero(got["dmu_u"][1]) == (dm != 0), (frac, kind, k, i)
            if frac == 0.5:
                assert ref["D"] > 0, (kind, k, i)
            if ref["I"] > 0:
                assert ref["I"] == ref["D"]
                toward_inf[frac].append((kind, k, i))
            assert_undecided(ref, got, 1)
            assert got["measures"][others].tobytes() == base["measures"][others].tobytes(), (frac, kind, k, i)
            assert got["at"][others].tolist() == [K, K]
    print((n, m, N), "positions whose dmu points to the infinite side:", toward_inf)
    assert toward_inf[0.5] + toward_inf[1.0]
    if (n, m, N) == (12, 4, 32):
        assert toward_inf[0.5]
    if n + m > 256:
        assert any(kind == "u" for kind, _, _ in toward_inf[1.0])  # (columns j >= 256: the second stride of the task loop)
    pair.close()


# ------------------------------------------------------------------------------------------ 3. what the read-out reports otherwise

def test_a_problem_frozen_before_the_check_reports_nothing(ndlqr, oracle):
    """Problem 0 without a bounded entry converges at iteration 1 (both residuals are exactly zero): no check examines
    it -- measured_at 0 and a row of zeros; the others are examined at K."""
    n, m, N = 12, 4, 16
    data = _data(ndlqr, oracle, n, m, N)
    bounds = [a.copy() for a in data.bounds]
    for a, v in zip(bounds, (-np.inf, np.inf, -np.inf, np.inf)):
        a[0] = v
    pair = Pair(ndlqr, data, False)
    got = pair.check(bounds)
    print("iterations", got["it"].tolist(), "status", got["st"].tolist(), "measured at", got["at"].tolist())
    assert got["st"][0] == 1 and got["it"][0] < K, (got["it"], got["st"])
    assert got["at"][0] == 0 and not got["measures"][0].any(), (got["at"], got["measures"])
    for p in (1, 2):
        assert got["st"][p] == 2
        assert_measures(data.probs[p], data.of(bounds, p), got, p)
    pair.close()


def test_nan_data_is_no_certificate(ndlqr, oracle):
    n, m, N = 12, 4, 16
    data = _data(ndlqr, oracle, n, m, N)
    bs = ndlqr.BatchSolver(n, m, N, data.batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    x0 = np.stack([p.x0 for p in data.probs])
    x0[2, 3] = np.nan
    bs.initialize_flat(*stack(data.probs)[:-1], x0)
    bs.set_bounds(*data.bounds)
    bs.set_box_infeasibility(1, EPS)
    it, st = bs.solve_box(rho=data.rho, alpha=ALPHA, eps_abs=TINY, eps_rel=TINY, max_iter=K, check_every=1)
    measures, at = bs.infeasibility_measures()
    print("iterations", it.tolist(), "status", st.tolist(), "measured at", at.tolist(), "row", measures[2].tolist())
    assert st[2] == 3 and st[0] == 2 and st[1] == 2, (it, st)
    assert (at[2] == 0 and not measures[2].any()) or np.isnan(measures[2]).any(), (at, measures[2])
    assert not any(c[2].any() for c in bs.infeasibility_certificate())
    assert at[0] == K and at[1] == K and np.isfinite(measures[:2]).all() and (measures[:2, 1] > 0).all()
    bs.close()


def test_measures_across_changes_of_the_adaptive_penalty(ndlqr, oracle):
    """adapt_every = 2 and a check at 6: both runs adapt at iterations 2 and 4 and neither at 5 or 6 (the last iteration
    never adapts), so the first run still is the second one iteration earlier, and dmu = rho y - rho y with the final
    penalties. From a tenth of the penalty of the other tests, so that the rule moves it."""
    n, m, N = 12, 4, 32
    data = _data(ndlqr, oracle, n, m, N)
    pair = Pair(ndlqr, data, False)
    got = pair.check(data.bounds, k=6, rho=0.1 * data.rho, adapt_every=2)
    rho_a, rho_b = [bs.box_penalties() for bs in pair.solvers]
    print("penalties", rho_b.tolist(), "from", 0.1 * data.rho)
    assert np.array_equal(rho_a, rho_b) and np.any(rho_b != 0.1 * data.rho)
    for p, prob in enumerate(data.probs):
        ref = assert_measures(prob, data.of(data.bounds, p), got, p, k=6)
        assert ref["D"] > 0 and ref["E"] > 0
        assert_undecided(ref, got, p)
    pair.close()


def test_destinations_and_refusals(ndlqr, oracle):
    n, m, N = 12, 4, 16
    data = _data(ndlqr, oracle, n, m, N)
    B = data.batch
    bs = ndlqr.BatchSolver(n, m, N, B, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(data.probs))
    bs.set_bounds(*data.bounds)
    args = dict(rho=data.rho, alpha=ALPHA, eps_abs=TINY, eps_rel=TINY, max_iter=K, check_every=K)
    # detection off (the initial state): refused
    bs.solve_box(**args)
    with pytest.raises(RuntimeError):
        bs.infeasibility_measures()
    bs.set_box_infeasibility(K, EPS)
    bs.solve_box(**args)
    measures, at = bs.infeasibility_measures()
    assert at.tolist() == [K] * B and (measures[:, 1] > 0).all()
    # device and pinned destinations; either pointer alone
    dm, di = ndlqr.DeviceArray((B, 4)), ndlqr.DeviceArray(((B + 1) // 2,))
    bs.infeasibility_measures(dm, di)
    assert dm.get().tobytes() == measures.tobytes()
    assert di.get().view(np.int32)[:B].tolist() == at.tolist()
    pm = ndlqr.pinned_empty((B, 4))
    pm[...] = -1.0
    bs.infeasibility_measures(pm)
    assert pm.tobytes() == measures.tobytes()
    L = ndlqr.lib()
    only = np.zeros((B, 4))
    assert L.ndlqr_CopyBatchInfeasibilityMeasures(bs.h, only.ctypes.data_as(ndlqr.api.dp), None) == 0
    assert only.tobytes() == measures.tobytes()
    ints = np.zeros(B, dtype=np.int32)
    assert L.ndlqr_CopyBatchInfeasibilityMeasures(bs.h, None, ints.ctypes.data_as(ndlqr.api.C.POINTER(ndlqr.api.C.c_int))) == 0
    assert ints.tolist() == at.tolist()
    assert L.ndlqr_CopyBatchInfeasibilityMeasures(bs.h, None, None) == ndlqr.api.ERR_INVALID
    # a solve with detection off, or a plain solve, drops them
    bs.set_box_infeasibility(0)
    bs.solve_box(**args)
    with pytest.raises(RuntimeError):
        bs.infeasibility_measures()
    bs.set_box_infeasibility(K, EPS)
    bs.solve_box(**args)
    assert bs.infeasibility_measures()[0].tobytes() == measures.tobytes()  # (and a repeated solve repeats every bit)
    assert bs.solve() == 0
    with pytest.raises(RuntimeError):
        bs.infeasibility_measures()
    bs.close()
