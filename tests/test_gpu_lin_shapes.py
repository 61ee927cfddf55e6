"""The kernels of the solve with linear inequality constraints (kernels_lin.hpp, kernels_lin_infeas.hpp; DESIGN.md sections
3.17, 3.19, 3.20) in every row and launch class: the row loops `r < p; r += 64` beyond their first pass, the column loop
of lin_next_rhs beyond 64 columns, lin_multipliers with several workgroups per problem and lin_certify beyond its first
pass of G = 256 / (n + m) knots. Every kernel is tested as what it is -- a function of the iterates two or three cold
solves stopped one iteration apart deliver through the public read-outs -- against a plain longdouble restatement
(lin_shape_support.update_reference, lin_support.shifted_problem / kkt_ld, lin_infeas_support.farkas_check_rows).

Cases (n, m, p, N); lin_shape_support.py holds the table as data and test_lin_shapes_host.py holds it to a restatement of
the kernels' loop bounds, the LDS of every case to the 160 KiB of a workgroup, and the inputs to the conditions below:

    case              row passes   columns    lin_multipliers   G    lin_certify passes   chosen for
    (6, 3, 1, 2)      1            9          1 workgroup       28   2                    one row, two knots: waves 2-3 and 63 lanes idle
    (12, 4, 64, 8)    1, exact     16         2, exact          16   8                    N p = 512; strided dmu load (512)
    (12, 4, 65, 5)    2, tail 1    16         2                 16   5                    padded horizon 5 -> 8, one-row second pass
    (6, 3, 130, 8)    3, tail 2    9          5                 28   8                    p far above n + m; N p = 1040
    (12, 4, 6, 32)    1            16         1                 16   16, 16               the knot behind the first pass; 8 knots a wavefront
    (12, 4, 6, 20)    1            16         1                 16   16, 4                horizon padded 20 -> 32
    (13, 4, 6, 16)    1            17         1                 15   15, 1                a tail pass of one knot
    (20, 5, 7, 16)    1            25         1                 10   10, 6
    (40, 2, 8, 8)     1            42         1                 6    6, 2                 dlam load 7 * 40 = 280 > 256; n > 32
    (48, 20, 8, 4)    1            68: 2      1                 3    3, 1                 two column passes of lin_next_rhs; 152 208 bytes of LDS

No case was refused by the library. A class n + m >= 256 (G clamped to 1) cannot exist: the LDS limit refuses it by name.
Batch 3, the problems of cost_support.family(n, m, N, "moderate"), rows of lin_shape_support.dense_rows in the "mixed"
pattern (both bounds / upper / lower / none by (k + r) % 4, one row with lo == hi) and, in part b, also "two_sided";
rho = 1, alpha = 1.6, fast and strict mode, eps_abs = eps_rel = 1e-300 (every solve ends as status 2 at max_iter).
Input conditions (host file): for p > 64 the rows >= 64 of every problem hold an entry on lo, on hi, inside and (mixed)
unbounded at every iteration compared -- which takes the fraction 0.15 resp. 0.3 instead of 0.6 for the rows >= 64 of
(12,4,65,5) and (6,3,130,8) and chosen seeds at the former --; the columns >= 64 of (48,20,8,4) carry >= 10 % of the
largest entry of G'M(y - v); every check of part d has D > 0 and terms of S from both sides, every case a row toward an
infinite bound; part e moves at least one problem and leaves none undecided.

a. Shifted costs per entry (lin_bounds, lin_shift_cost; p >= 64 and the wide case): the rule of
   test_gpu_lin.test_shifted_reduction_per_entry, whose code it calls (8 x the float64 restatement's own largest error
   against the longdouble one, at least 16 eps of the array's largest entry), in both modes.

b. One update as a function of its inputs (lin_update, lin_multipliers, lin_finish), K = 3. Run A (K - 1 iterations) gives
   v0, y0, run B (K) the delivered x, u and v+, y+, mu, the four numbers. lin_update forms x, u in LDS with
   cost_knot_S<false> and lin_finish delivers them with cost_knot_S<true>: the same sequence on the x and u rows -- the
   back-substitutions cost_trsv_lower_t on L^ and L_R, then u = u~ - G x by one fma chain; LAMBDA only adds the product
   L^ lambda~ -- on the same z~, so the delivered x, u are the bits the update worked on and no term is added for them.
   With u = 2^-53 and eps = 2 u, |.| the sums of absolute terms update_reference returns:
     w = C x + D u   one fma chain of n + m terms on exact inputs: within (n + m) u |w|_1 (1 + ..); taken as
                     b_w = (n + m + 2) eps |w|_1, |w|_1 = |C||x| + |D||u|;
     t = wh + y0     fast: fl(oma v0), one fma, one sum; strict: two products, two sums. Each rounding is u times a
                     partial sum of alpha |w| + |oma v0| + |y0| = |t|_1, at most 3 u |t|_1 (1 + 3 u) in all, on top of
                     alpha b_w: b_t = alpha b_w + 2 eps |t|_1;
     v+ = clip(t)    min and max are exact and 1-Lipschitz: b_t. A row whose reference t lies beyond a bound by more than
                     b_t is beyond it on the device too: v+ IS that bound, bit for bit;
     y+ = (y0 + wh) - v+   the sum is t again (the same two operands), the difference rounds once:
                     b_y = 2 b_t + eps |y+|;
     r_prim = max |w - v+|: b_w + b_t + eps (|w| + |v+|), the largest over the bounded rows (a maximum moves by no more
                     than its entries); s_prim = max(max |w|, max |v+|): max(b_w, b_t) likewise;
     r_dual = rho max |G'M(v+ - v0)|, s_dual = rho max |G'M y+|: functions of read-out values alone -- v+ - v0 is one
                     double subtraction of read-out numbers, the same bits in numpy --, each entry a p-term fma chain
                     and one product with rho: (p + 3) eps rho x the largest sum of absolute terms of an entry.
   Exact: v == 0 and y == 0 on the unbounded rows, v+ on its bound as above, mu == rho y. Measured: v+ within 0.12 of its
   bound, y+ 0.06, the four numbers 0.10.

c. The next right-hand side (lin_next_rhs of lin_update; lin_start warm). z of a cold solve stopped at K + 1, of a warm
   start with max_iter = 1 behind K iterations, and of a second one whose bounds release rows >= 64 (the last row where
   p <= 64) at the even knots -- y of those reads 0 afterwards -- satisfies, in longdouble, K^ z = b^ - [C'; D'] rho M (y - v)
   with (v, y) as read before it, to 1e-9 max(1, ||rhs||_inf): the residual bar of test_compact1_records. A dropped row or
   column leaves rho |G' t|, 1e3 of the bar or more (host file). Measured: 9e-12 at most.

d. lin_certify in every pass class: test_gpu_lin_infeas.test_kept_lambda_is_the_delivered_one at all ten cases and both
   modes, one check at K = 4 (lin_infeas_support.check_kept_lambda, which both files call): D and the infinite-side
   maximum bit for bit, ||e||_inf within (n + p + 2) eps e_scale, S within 4 eps^2 S_scale + eps |S|.

e. A penalty move with p > 64 (lin_tail_new_penalty, lin_start in its restart mode). The rule is never evaluated at the
   last iteration of a solve (it < max_iter: kernels_lin.hpp, lin_adaptive_support), so no solve ends behind a move and
   y as the tail leaves it has no read-out; every = 2 with max_iter = 2 moves nothing. The move at iteration 2 is
   therefore held through iteration 3 of a solve with max_iter = 3: the penalties are those of the float64 restatement
   (its decisions are off a power of two by the margin of lin_adaptive_support); for a problem that moved, iteration 3
   passes part b and part c as a function of v_2 and y_2 rho / rho+ -- v_2, y_2 and mu_2 from the solve without
   adaptation stopped at 2, the rescaling exact in numpy (a power of two: rho+ (y_2 rho / rho+) == mu_2 bit for bit is
   asserted) -- and mu == rho+ y bit for bit; a problem that did not move has the bits of the solve without adaptation.
   A rescaling skipped on the rows >= 64 leaves |1 - rho / rho+| |y_2| in y+ of a row on its bound: 1e6 of b_y (host file).

What the cases catch. Each change below was made once in a scratch build of hip_lin.hip, and this file and the existing
test_gpu_lin*.py files (151 tests) were run once against it; every change only skips work or drops a term:
  1. the row loop of lin_update_knot without its stride: 10 cases fail -- parts b (both patterns), c, d and e at
     (12,4,65,5) and (6,3,130,8);
  2. the column loop of lin_next_rhs cut to its first 64: 3 cases -- part b (both patterns) and part c at (48,20,8,4);
  3. lin_multipliers ignoring blockIdx.x: 14 cases -- parts b (both patterns), c and d at the three cases with p >= 64,
     part e at its two;
  4. the k0 loop of lin_certify ended after its first pass: 6 cases -- part d at the six cases of two passes;
  5. nl = nk in lin_certify: 5 of those 6 -- all but (20,5,7,16), where the row of LDS read instead leaves the maximum
     of |e| where it was;
  6. the dlam load of lin_certify without its stride: 1 case -- part d at (40,2,8,8).
Under every one of the six all 151 existing tests pass.

Measured on an MI355X: the 46 cases take 3.7 s together; the slowest are part a at (12,4,64,8) (0.31 s, it loads the
library) and at (48,20,8,4) (0.22 s: the longdouble reduction of n = 48), part c at (40,2,8,8) and part b two-sided at
(12,4,6,32) (0.20 s each: their CPU reference), nothing else above 0.18 s. A case runs 2 to 9 solves of 1 to 4 iterations.
"""
import functools

import numpy as np
import pytest

import cost_support as cs
import lin_infeas_support as li
import lin_shape_support as sh
from test_gpu_lin import check_shifted_reduction, constrained_solver

pytestmark = pytest.mark.gpu

LD = np.longdouble
K = sh.K_UPDATE
TINY = dict(rho=sh.RHO, alpha=sh.ALPHA, eps_abs=1e-300, eps_rel=1e-300)
RESIDUAL_BAR = 1e-9  # (test_compact1_records.test_solution_and_residual)


def modes(ndlqr):
    return [0, ndlqr.FLAG_STRICT_FP]


def ids(case):
    return "%d-%d-%d-%d" % case


def run(bs, max_iter, **kw):
    """one solve that must end as status 2 at max_iter, and everything it leaves"""
    iters, status = bs.solve_constrained(max_iter=max_iter, **dict(TINY, **kw))
    assert (iters == max_iter).all() and (status == 2).all(), (iters, status)
    red = bs.constraint_reduction()
    return dict(Z=bs.solutions(), v=red["v"], y=red["y"], mu=bs.constraint_multipliers(), resid=bs.constraint_residuals())


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def cold_runs(ndlqr, case, pattern, flags):
    """three cold solves of batch(case, pattern), stopped at K - 1, K and K + 1 iterations; shared by parts b and c"""
    n, m, p, N = case
    bs = constrained_solver(ndlqr, sh.batch(case, pattern), flags)
    out = {mi: run(bs, mi) for mi in (K - 1, K, K + 1)}
    bs.close()
    return out


def check_update(c, Z, v0, y0, got, rho, label):
    """Part b for one problem: the read-out of an update (v, y, mu, resid of `got`) against update_reference() fed with the
    delivered iterate Z and the inputs v0, y0, to the bounds of update_bars(); the exact assertions."""
    n, m, N = cs.dims(c["p"])
    p = c["C"].shape[1]
    lo, hi = c["lo"], c["hi"]
    _, x, u = cs.split(Z, n, m, N)
    ref = sh.update_reference(c["p"], c["C"], c["D"], x, u, v0, y0, lo, hi, rho, sh.ALPHA, vn_read=got["v"], yn_read=got["y"])
    bars = sh.update_bars(ref, n, m, p, rho)
    M = ref["M"]
    ev, ey = np.abs(got["v"] - ref["vn"]), np.abs(got["y"] - ref["yn"])
    er = [abs(LD(got["resid"][q]) - ref["resid"][q]) for q in range(4)]
    print(*label, "v+ %.2f of its bound, y+ %.2f, r_prim r_dual s_prim s_dual" % (float((ev[M] / bars["t"][M]).max()),
          float((ey[M] / bars["y"][M]).max())), ["%.2f" % float(e / b) if b > 0 else "-" for e, b in zip(er, bars["resid"])])
    assert (ev <= bars["t"]).all(), (label, float((ev - bars["t"]).max()))
    assert (ey <= bars["y"]).all(), (label, float((ey - bars["y"]).max()))
    for q in range(4):
        assert er[q] <= bars["resid"][q], (label, q, got["resid"], [float(a) for a in ref["resid"]], float(bars["resid"][q]))
    # exact: the unbounded rows, the rows beyond a bound by more than their own bound, mu = rho y
    assert not got["v"][~M].any() and not got["y"][~M].any(), label
    above, below = M & (ref["t"] > hi + bars["t"]), M & (ref["t"] < lo - bars["t"])
    assert np.array_equal(got["v"][above], hi[above]) and np.array_equal(got["v"][below], lo[below]), label
    assert np.array_equal(got["mu"], rho * got["y"]), label
    return int(above.sum()), int(below.sum())


def check_residual(c, rho, Z, v, y, label, lo=None, hi=None):
    """Part c for one problem: K^ Z = b^ - [C'; D'] rho M (y - v) in longdouble to 1e-9 max(1, ||rhs||_inf)"""
    lo, hi = c["lo"] if lo is None else lo, c["hi"] if hi is None else hi
    res, size = sh.kkt_residual(c["p"], c["C"], c["D"], lo, hi, rho, Z, v, y)
    print(*label, "residual %.3e of a right-hand side of %.3e" % (res, size))
    assert res <= RESIDUAL_BAR * max(1.0, size), (label, res, size)


# ---------------------------------------------------------------------------- a: shifted costs per entry
@pytest.mark.parametrize("case", sh.TALL + [sh.WIDE], ids=ids)
def test_shifted_costs_per_entry(ndlqr, case):
    cases = sh.batch(case, "mixed")
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        run(bs, 1)
        got = bs.constraint_reduction()
        bs.close()
        check_shifted_reduction(got, cases, (case, "flags", flags))


# ---------------------------------------------------------------------------- b: one update as a function of its inputs
@pytest.mark.parametrize("pattern", sh.PATTERNS)
@pytest.mark.parametrize("case", sh.CASES, ids=ids)
def test_update_as_a_function_of_its_inputs(ndlqr, case, pattern):
    cases = sh.batch(case, pattern)
    clipped = np.zeros(2, dtype=int)
    for flags in modes(ndlqr):
        runs = cold_runs(ndlqr, case, pattern, flags)
        A, B = runs[K - 1], runs[K]
        if pattern == "mixed":  # (once per case and mode: a repeated solve gives the same bits)
            bs = constrained_solver(ndlqr, cases, flags)
            assert same(run(bs, K), B) and same(run(bs, K - 1), A) and same(run(bs, K), B)
            bs.close()
        for i, c in enumerate(cases):
            got = {k: B[k][i] for k in ("v", "y", "mu", "resid")}
            clipped += check_update(c, B["Z"][i], A["v"][i], A["y"][i], got, sh.RHO, ("update", case, pattern, "flags", flags, i))
    if case[2] > 1:
        assert clipped.min() >= 1, clipped


# ---------------------------------------------------------------------------- c: the next right-hand side
@pytest.mark.parametrize("case", sh.CASES, ids=ids)
def test_next_right_hand_side(ndlqr, case):
    n, m, p, N = case
    cases = sh.batch(case, "mixed")
    lo2, hi2 = (np.stack(a) for a in zip(*[sh.released_bounds(c["lo"], c["hi"]) for c in cases]))
    for flags in modes(ndlqr):
        runs = cold_runs(ndlqr, case, "mixed", flags)
        B, Cn = runs[K], runs[K + 1]
        label = ("rhs", case, "flags", flags)
        for i, c in enumerate(cases):  # lin_next_rhs of lin_update
            check_residual(c, sh.RHO, Cn["Z"][i], B["v"][i], B["y"][i], label + ("cold", i))
        bs = constrained_solver(ndlqr, cases, flags)
        assert same(run(bs, K), B)
        W = run(bs, 1, warm_start=True)  # lin_start, warm, from (v_K, y_K)
        for i, c in enumerate(cases):
            check_residual(c, sh.RHO, W["Z"][i], B["v"][i], B["y"][i], label + ("warm", i))
        bs.set_constraint_bounds(lo2, hi2)  # ... and with rows that left the splitting
        W2 = run(bs, 1, warm_start=True)
        bs.close()
        for i, c in enumerate(cases):
            released = sh.bounded(c["lo"], c["hi"]) & ~sh.bounded(lo2[i], hi2[i])
            assert released.sum() >= 1 and (p <= 64 or released[:, 64:].any())
            if p > 64:  # (they carried a multiplier: test_lin_shapes_host.py holds the restatement to it)
                assert np.abs(W["y"][i][:, 64:][released[:, 64:]]).max() > 0
            assert not W2["y"][i][released].any() and not W2["mu"][i][released].any()
            check_residual(c, sh.RHO, W2["Z"][i], W["v"][i], W["y"][i], label + ("released", i), lo2[i], hi2[i])


# ---------------------------------------------------------------------------- d: lin_certify in every pass class
@pytest.mark.parametrize("case", sh.CASES, ids=ids)
def test_certify_in_every_pass_class(ndlqr, case):
    cases = sh.batch(case, "mixed")
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        chk = li.check_kept_lambda(bs, cases, sh.K_CERTIFY, sh.K_CERTIFY, 1e-4, TINY, ("certify", case, "flags", flags))
        bs.close()
        if case[2] > 1:
            assert any(c["inf_max"] > 0 for c in chk)


# ---------------------------------------------------------------------------- e: a penalty move with p > 64
@pytest.mark.parametrize("case", sh.ADAPT_CASES, ids=ids)
def test_penalty_move_behind_the_first_row_pass(ndlqr, case):
    n, m, p, N = case
    cases = sh.batch(case, "mixed")
    want = [a["run"]["rho"] for a in sh.adaptive_runs(case)]
    for flags in modes(ndlqr):
        bs = constrained_solver(ndlqr, cases, flags)
        X2, X3 = run(bs, sh.ADAPT_EVERY), run(bs, sh.ADAPT_ITERS)
        bs.set_constraint_adaptation(sh.ADAPT_EVERY)
        Y = run(bs, sh.ADAPT_ITERS)
        rho = bs.constraint_penalties()
        bs.close()
        print("penalties", case, "flags", flags, list(rho), "restatement", want)
        assert list(rho) == want
        for i, c in enumerate(cases):
            label = ("move", case, "flags", flags, i)
            got = {k: Y[k][i] for k in ("v", "y", "mu", "resid")}
            if rho[i] == sh.RHO:  # (a problem that did not move: the bits of the solve without adaptation)
                assert all(np.array_equal(Y[k][i], X3[k][i]) for k in Y), label
                continue
            y0 = X2["y"][i] * (sh.RHO / rho[i])  # (a power of two: exact)
            assert np.array_equal(rho[i] * y0, X2["mu"][i])
            check_update(c, Y["Z"][i], X2["v"][i], y0, got, rho[i], label)
            check_residual(c, rho[i], Y["Z"][i], X2["v"][i], y0, label)
