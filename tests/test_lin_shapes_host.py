"""The cases of tests/test_gpu_lin_shapes.py held to what they were chosen for, without a GPU: the loop classes of
lin_shape_support.TABLE against the restatement of the kernels' loop bounds (launch_classes), the LDS of every case against
the limit of a workgroup, and the input conditions of the GPU tests on the float64 restatement of the iteration
(lin_support.admm, lin_adaptive_support.admm_adaptive) -- for every case, pattern, problem and iteration the GPU file
compares. They are conditions on the inputs, not measurements of the device: a case that stops meeting one fails here,
and no GPU test skips or excuses a case at run time.

The reference side of the GPU file is what batch() and adaptive_runs() compute here, once per (case, pattern): the test
below holds the work of each case to REFERENCE_FLOPS, a second of one processor core at a few Gflop/s, and prints the
time it took (measured: 1.0 s at (12,4,6,32), whose dense KKT matrix has order 896; 0.3 s at most elsewhere)."""
import time

import numpy as np
import pytest

import cost_support as cs
import lin_adaptive_support as las
import lin_infeas_support as li
import lin_shape_support as sh
import lin_support as ls

REFERENCE_FLOPS = 4e9
ORDERS = 1e3  # "orders above the bar": what a dropped row or column must leave, in units of the residual bar of part c


def tail(p):
    return slice(64, None) if p > 64 else slice(None)


# ---------------------------------------------------------------------------- the table
@pytest.mark.parametrize("case", sh.CASES)
def test_table_is_the_restated_loops(case):
    got = sh.launch_classes(*case)
    for k, want in sh.TABLE[case].items():
        assert got[k] == want, (case, k, got[k], want)


def test_every_class_has_its_case():
    cl = {c: sh.launch_classes(*c) for c in sh.CASES}
    assert sorted(sh.TABLE) == sorted(sh.CASES) and len(sh.CASES) == 10
    # row loops: one pass with one row, an exact pass, a second pass of one row, a third pass
    assert cl[(6, 3, 1, 2)]["row_tail"] == 1 and cl[(12, 4, 64, 8)]["row_tail"] == 64
    assert (cl[(12, 4, 65, 5)]["row_passes"], cl[(12, 4, 65, 5)]["row_tail"]) == (2, 1)
    assert (cl[(6, 3, 130, 8)]["row_passes"], cl[(6, 3, 130, 8)]["row_tail"]) == (3, 2)
    # the column loop of lin_next_rhs: only the wide case goes round twice
    assert [c for c in sh.CASES if cl[c]["col_passes"] > 1] == [sh.WIDE]
    # lin_multipliers: more than one workgroup per problem, one of them exact
    assert [c for c in sh.CASES if cl[c]["groups"] > 1] == sh.TALL and 8 * 64 == 2 * 256
    # lin_certify: a knot behind a pass (nl = nk + 1), tail passes of 1 and of more, a strided dlam load and a strided dmu load
    behind = [c for c in sh.CASES if any(nl == nk + 1 for nk, nl in cl[c]["passes"])]
    assert behind == sh.CASES[4:]
    assert cl[(13, 4, 6, 16)]["passes"][-1] == (1, 1) and cl[(12, 4, 6, 32)]["passes"][-1] == (16, 16)
    assert [c for c in sh.CASES if cl[c]["dlam"] > 256] == [(40, 2, 8, 8)]
    assert [c for c in sh.CASES if cl[c]["dmu"] > 256] == sh.TALL
    # padded horizons (the device's horizon is a power of two)
    assert [c for c in sh.CASES if c[3] & (c[3] - 1)] == [(12, 4, 65, 5), (12, 4, 6, 20)]


def test_lds_of_every_case_and_the_class_that_cannot_exist():
    sizes = {c: sh.lds_bytes(*c[:3]) for c in sh.CASES}
    for c, b in sizes.items():
        assert b <= sh.LDS_LIMIT, (c, b)
    assert max(sizes, key=sizes.get) == sh.WIDE and sizes[sh.WIDE] == 152208
    # n + m >= 256: the record of one knot alone is beyond the limit, whatever the split and with a single row
    for n in range(1, 256):
        assert sh.lds_bytes(n, 256 - n, 1) > sh.LDS_LIMIT, n


# ---------------------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("case", sh.CASES)
def test_reference_stays_within_the_cap(case):
    """what a GPU case computes on the CPU, past the caches: the family, the rows and the iterates of both patterns and
    the adaptive runs"""
    n, m, p, N = case
    t0 = time.perf_counter()
    cs.family.__wrapped__(n, m, N, "moderate")
    for pattern in sh.PATTERNS:
        sh.batch.__wrapped__(case, pattern)
    if case in sh.ADAPT_CASES:
        sh.adaptive_runs.__wrapped__(case)
    print("reference", case, "%.2f s" % (time.perf_counter() - t0))
    # a stopwatch is no assertion; the work is: per problem and pattern one dense LU of order N (2n + m) and at most
    # K_CERTIFY + ADAPT_ITERS + 1 (a refactorisation) substitutions, and the rows' dot products
    order = N * (2 * n + m)
    flops = cs.BATCH * len(sh.PATTERNS) * (2 * order ** 3 // 3 + 16 * (2 * order ** 2 + 8 * N * p * (n + m)))
    assert order <= 1024 and flops <= REFERENCE_FLOPS, (case, order, flops)


# ---------------------------------------------------------------------------- rows
@pytest.mark.parametrize("pattern", sh.PATTERNS)
@pytest.mark.parametrize("case", sh.CASES)
def test_rows_of_every_class_behind_the_first_pass(case, pattern):
    """Every problem, at each of the iterations compared (the update of part b, the two iterates of part d): the rows
    >= 64 hold an entry on lo, one on hi and one strictly inside, in the mixed pattern also an unbounded one. Every case:
    bounded rows on a bound and inside among all rows of the batch, and the pinned row of the mixed pattern."""
    n, m, p, N = case
    total = np.zeros(4, dtype=int)
    for i, c in enumerate(sh.batch(case, pattern)):
        M = sh.bounded(c["lo"], c["hi"])
        if pattern == "mixed":
            k, r = sh.pinned_row(N, p)
            assert c["lo"][k, r] == c["hi"][k, r] and np.isfinite(c["lo"][k, r])
            assert ((c["lo"] == c["hi"]).sum()) == 1
            assert np.array_equal(M, sh.row_kind(N, p) != 3)
        else:
            assert M.all() and (c["lo"] < c["hi"]).all()
        for it in (sh.K_UPDATE, sh.K_CERTIFY):
            v = c["its"][it - 1]["v"]
            assert c["its"][it - 1]["it"] == it
            total += sh.row_classes(c["lo"], c["hi"], v)
            if p > 64:
                on_lo, on_hi, inside, unbounded = sh.row_classes(c["lo"], c["hi"], v, tail(p))
                assert on_lo >= 1 and on_hi >= 1 and inside >= 1, (case, pattern, i, it, on_lo, on_hi, inside)
                assert unbounded >= 1 or pattern == "two_sided", (case, pattern, i, it)
    if p > 1:  # (the single row of (6,3,1,2) is pinned at knot 0 and one-sided at knot 1)
        assert total[0] >= 1 and total[1] >= 1 and total[2] >= 1, (case, pattern, total)


@pytest.mark.parametrize("case", sh.CASES)
def test_a_dropped_row_or_column_is_orders_above_the_residual_bar(case):
    """Part c holds K^ z = b^ - [C'; D'] rho M (y - v) to 1e-9 max(1, ||rhs||). What the right-hand side loses with the
    columns >= 64 of [C D] (the second pass of lin_next_rhs's column loop) or with the rows >= 64 of its dot products is
    rho |G' t| over those: ORDERS above the bar, for every problem; and the columns >= 64 carry at least 10 % of the
    largest entry of G'M(y - v)."""
    n, m, p, N = case
    if case != sh.WIDE and p <= 64:
        return  # (one pass of either loop: nothing to drop; the classes are asserted above)
    for i, c in enumerate(sh.batch(case, "mixed")):
        s = c["its"][sh.K_UPDATE - 1]
        M = sh.bounded(c["lo"], c["hi"])
        t = np.where(M, sh.RHO * (s["y"] - s["v"]), 0.0)
        K, b = ls.kkt_ld(ls.shifted_problem(c["p"], c["C"], c["D"], c["lo"], c["hi"], sh.RHO))
        g = ls.perturbation(c["p"], c["C"], c["D"], t)
        bar = 1e-9 * max(1.0, float(np.abs(b - g).max()))
        _, gx, gu = cs.split(g, n, m, N)
        if case == sh.WIDE:
            cols = np.concatenate([gx, gu], axis=1)[:, 64:]
            share = float(np.abs(cols).max() / np.abs(g).max())
            print("columns >= 64", case, i, "share of the largest entry %.2f" % share)
            assert share >= 0.10, (i, share)
            assert float(np.abs(cols).max()) >= ORDERS * bar, (i, float(np.abs(cols).max()), bar)
        if p > 64:
            # the rows >= 64 the second warm start releases carry a multiplier after the K_UPDATE + 1 iterations before it
            lo2, hi2 = sh.released_bounds(c["lo"], c["hi"])
            released = M & ~sh.bounded(lo2, hi2)
            assert released[:, 64:].any() and not released[:, :64].any()
            assert np.abs(c["its"][sh.K_UPDATE]["y"][released]).max() > 0, i
            t_tail = t.copy()
            t_tail[:, :64] = 0.0
            lost = float(np.abs(ls.perturbation(c["p"], c["C"], c["D"], t_tail)).max())
            assert lost >= ORDERS * bar, (i, lost, bar)


# ---------------------------------------------------------------------------- the certificate inputs
@pytest.mark.parametrize("case", sh.CASES)
def test_certificate_inputs_reach_every_branch(case):
    """Part d, mixed pattern. Every problem: ||dmu||_inf > 0 and terms of S from upper and from lower bounds. Every case:
    a problem with a row whose dmu points to an infinite bound (the infinite-side maximum is > 0; y of a one-sided row
    has one sign, so this needs a multiplier that shrinks over the iteration). The single-row case, whose two rows per
    problem cannot hold all of it: one side of S somewhere in the batch."""
    n, m, p, N = case
    seen = np.zeros(3, dtype=int)
    for i, c in enumerate(sh.batch(case, "mixed")):
        dlam, dmu = sh.certificate_inputs(c)
        chk = li.farkas_check_rows(c["p"], c["C"], c["D"], c["lo"], c["hi"], dlam, dmu, 1e-4)
        assert chk["dmu_inf"] > 0 and np.abs(dlam).max() > 0, (case, i)
        upper = int(((dmu > 0) & np.isfinite(c["hi"])).sum())
        lower = int(((dmu < 0) & np.isfinite(c["lo"])).sum())
        here = np.array([chk["inf_max"] > 0, upper > 0, lower > 0], dtype=int)
        seen += here
        if p > 1:
            assert here[1:].all(), (case, i, here)
    print("certificate inputs", case, "problems with an infinite-side row, upper terms, lower terms:", seen)
    assert seen[1] + seen[2] >= 1, (case, seen)
    if p > 1:
        assert seen[0] >= 1, (case, seen)


# ---------------------------------------------------------------------------- the penalty move
@pytest.mark.parametrize("case", sh.ADAPT_CASES)
def test_penalty_moves_are_decided_and_reach_the_rows_behind_the_first_pass(case):
    """Part e: no problem is left undecided by the margin, at least one moves at iteration ADAPT_EVERY, by a power of
    two; and for a problem that moves, a rescaling y <- y rho / rho+ skipped on the rows >= 64 would leave y+ of the
    next iteration 1e6 of its rounding bound away on one of them."""
    n, m, p, N = case
    moved = 0
    for i, (c, a) in enumerate(zip(sh.batch(case, "mixed"), sh.adaptive_runs(case))):
        run, its = a["run"], a["its"]
        print("adaptive", case, i, "rho", run["rho"], "margin %.3e" % a["margin"])
        assert a["margin"] >= las.DECIDED, (case, i, a["margin"])
        assert run["iters"] == sh.ADAPT_ITERS and run["status"] == 2
        assert [t["adapt"] for t in its] == [False, True, False]
        if run["rho"] == sh.RHO:
            assert not run["moves"]
            continue
        moved += 1
        mv, = run["moves"]
        assert mv["it"] == sh.ADAPT_EVERY and not mv["clamped"] and np.log2(mv["rho_new"]) == int(np.log2(mv["rho_new"]))
        s = sh.RHO / run["rho"]
        y2, v2 = its[1]["y"], its[1]["v"]
        _, x, u = cs.split(its[2]["z"], n, m, N)
        M = sh.bounded(c["lo"], c["hi"])
        ref = sh.update_reference(c["p"], c["C"], c["D"], x, u, v2, y2 * s, c["lo"], c["hi"], run["rho"], sh.ALPHA)
        bars = sh.update_bars(ref, n, m, p, run["rho"])
        # a row that ends on a bound has y+ = (y0 + wh) - bound: it carries the error of y0 as it is
        on_bound = M & (ref["vn"] != ref["t"])
        on_bound[:, :64] = False
        effect = np.where(on_bound, abs(1.0 - s) * np.abs(y2), 0.0)
        k, r = np.unravel_index(np.argmax(effect), effect.shape)
        assert effect[k, r] >= 1e6 * float(bars["y"][k, r]), (case, i, effect[k, r], float(bars["y"][k, r]))
    assert moved >= 1, case


# ---------------------------------------------------------------------------- the restated update
@pytest.mark.parametrize("case", [(6, 3, 130, 8), (48, 20, 8, 4)])
def test_update_reference_is_the_restated_iteration(case):
    """update_reference() fed with the float64 restatement's own iterates returns that restatement's next ones within its
    own bars (numpy's dot products are not fma chains, but no longer ones either), and its bars are small against the
    bounds: the exact assertions of part b apply to rows on a bound."""
    n, m, p, N = case
    for c in sh.batch(case, "mixed"):
        a, b = c["its"][sh.K_UPDATE - 2], c["its"][sh.K_UPDATE - 1]
        _, x, u = cs.split(b["z"], n, m, N)
        ref = sh.update_reference(c["p"], c["C"], c["D"], x, u, a["v"], a["y"], c["lo"], c["hi"], sh.RHO, sh.ALPHA,
                                  vn_read=b["v"], yn_read=b["y"])
        bars = sh.update_bars(ref, n, m, p, sh.RHO)
        assert (np.abs(b["v"] - ref["vn"]) <= bars["t"]).all() and (np.abs(b["y"] - ref["yn"]) <= bars["y"]).all()
        for q in range(4):
            assert abs(np.longdouble(b["resid"][q]) - ref["resid"][q]) <= bars["resid"][q], (q, b["resid"], ref["resid"])
        assert float(bars["t"].max()) <= 1e-12 * float(np.abs(c["hi"][np.isfinite(c["hi"])]).min())
        clipped = sh.bounded(c["lo"], c["hi"]) & ((ref["t"] > c["hi"] + bars["t"]) | (ref["t"] < c["lo"] - bars["t"]))
        assert clipped.sum() >= 2
