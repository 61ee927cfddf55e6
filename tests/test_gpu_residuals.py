"""The two device residual kernels the rest of the suite trusts as witnesses, tested themselves: kkt_residual_dd
(ndlqr_BatchKktResidualVector, the eta and the acceptance of ndlqr_RefineBatch) bit for bit against
refine_support.residual_dd in every launch shape, kkt_residual_generic (ndlqr_BatchKktResiduals) row class by row class
against the plain extended-precision rows of residual_support.kkt_rows_ld, and the strict-mode termination (iters, status)
of the box-constrained solve against the numpy restatement driving the oracle.

Launch shape of kkt_residual_dd per case of VECTOR_SHAPES (launch_residual_dd: 64 / 128 / 256 threads by rows + n of the
padded block; the [A | B] tile staged in LDS while 8 (n (w | 1) + 2 rows) + 64 <= 160 KiB, else read in place; passes =
ceil((rows + n) / threads) of the task loop in block 0). test_residual_support_host.py holds the same table against a
restatement of the launcher, so a change of the launcher or of the padding shows which cases need new shapes:

    shape (n, m, N)   padded     threads   tile       passes   chosen for
    (32, 8, 4)        --         128       staged     1        the 128-thread block
    (48, 16, 4)       --         256       staged     1        the 256-thread block, one pass
    (96, 16, 2)       --         256       staged     2        the strided task loop over a staged tile
    (128, 16, 2)      --         256       staged     2        the largest staged tile (152 896 B)
    (144, 16, 2)      --         256       in place   2        in place; block 0 and the last block only
    (144, 16, 4)      --         256       in place   2        in place, with middle knots
    (130, 5, 4)       (144, 8)   256       in place   2        live-row masks of a block padded beyond 128 states
    (150, 10, 2)      (160, 12)  256       in place   2        the same, another padding
    (256, 32, 2)      --         256       in place   4        four passes
    (1, 1, 8)         (6, 3)     64        staged     1        the smallest padded instance (live masks, 64 threads)

Row counts, not horizons, select the branch, so the horizons are the smallest that have the knots wanted.

Every strict-mode solve of these shapes succeeds, so part 1 runs all of them in both modes.

Measured on an MI355X: the 42 cases take 2.3 s together; the slowest are the first case (0.30 s, it loads the library),
(6, 3, 8192) x 2 of part 3 (0.17 s), the strict box solve at (20, 6, 16) (0.13 s) and (256, 32, 4) x 3 of part 3 (0.07 s).

What the cases catch, each change made once in a scratch build and the file run once against it:
  - the task loop of kkt_residual_dd cut to a single pass: 20 cases of parts 1 and 2 fail, every shape of two passes or
    more ((96, 16, 2) in fast mode only through part 2 and strict mode: the rows of the second pass there are the
    lambda_0 rows, whose residual is exactly zero after a fast solve);
  - zk read for zn in the x rows of the branch that reads [A | B] in place: the 15 cases of parts 1 and 2 at the five
    in-place shapes fail;
  - the u rows of knot N - 2 dropped from kkt_residual_generic, or column 0 dropped from its dynamics rows: all eight
    cases of part 3 fail.
test_residual_vector_bit_exact (test_gpu_refine.py) passes under the first two; test_device_kkt_residual_matches_oracle
(test_gpu_parity.py) fails under the last two as well.
"""
import numpy as np
import pytest

from box_support import split
from refine_support import eta, hard_problem, residual_dd
from residual_support import (BOX_TERMINATION, BOX_TERMINATION_CASES, box_termination_reference, kkt_rows_ld, mixed_problem,
                              norm_ld, rhs_ld)
from support import Problem
from test_gpu_parity import stack, synth

pytestmark = pytest.mark.gpu

VECTOR_SHAPES = [(32, 8, 4), (48, 16, 4), (96, 16, 2), (128, 16, 2), (144, 16, 2), (144, 16, 4), (130, 5, 4), (150, 10, 2),
                 (256, 32, 2), (1, 1, 8)]
RHS = ("q", "r", "d", "x0")


def solver(ndlqr, probs, flags):
    p0 = probs[0]
    bs = ndlqr.BatchSolver(p0.n, p0.m, p0.N, len(probs), flags=flags)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    return bs


# ------------------------------------------------------------------------------------ 1. the double-double vector

@pytest.mark.parametrize("n,m,N", VECTOR_SHAPES)
@pytest.mark.parametrize("strict", [False, True], ids=["fast", "strict"])
def test_residual_vector_bit_exact_in_every_launch_shape(ndlqr, n, m, N, strict):
    """One weak-R problem and one plain synthetic one: the vector equals the numpy restatement bit for bit, in fast and in
    strict mode (the kernel is compiled without contraction in both), the call leaves the solution alone, and the
    device-pointer output is the host one."""
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 40), synth(ndlqr, n, m, N, 41)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT if strict else 0)
    z = bs.solutions().copy()
    r = bs.kkt_residual_vector()
    assert bs.solutions().tobytes() == z.tobytes()
    for p, prob in enumerate(probs):
        ref = residual_dd(prob, z[p])[0]
        bad = np.nonzero(r[p] != ref)[0]
        assert np.array_equal(r[p], ref), (p, bad.size, bad[:8], np.max(np.abs(r[p] - ref)))
        assert np.any(ref != 0.0)
    rd = bs.kkt_residual_vector(ndlqr.DeviceArray((2, bs.nvars))).get()
    assert np.array_equal(rd, r)
    bs.close()


# ------------------------------------------------------------------------------------ 2. delta and the norm slots

@pytest.mark.parametrize("n,m,N", VECTOR_SHAPES)
def test_refinement_norms_and_delta_path_exact_in_fast_mode(ndlqr, n, m, N):
    """One refinement step of three weak-R problems in fast mode: eta before is that of the restatement on z as found; an
    accepted step leaves z + delta in fp64, which is what the kernel evaluated, so eta after is that of the restatement on
    the committed z, and its residual norm is below the old one; a rejected step leaves every bit and reports eta before
    twice."""
    batch = 3
    probs = [hard_problem(ndlqr.generate_synthetic, n, m, N, 300 + p) for p in range(batch)]
    bs = solver(ndlqr, probs, ndlqr.FLAG_KEEP_RECORDS)
    z0 = bs.solutions().copy()
    steps, before, after = bs.refine(1)
    z1 = bs.solutions().copy()
    print((n, m, N), "steps", steps.tolist(), "eta", before.tolist(), "->", after.tolist())
    assert set(steps.tolist()) <= {0, 1} and np.any(steps == 1), steps
    r1 = bs.kkt_residual_vector()
    for p, prob in enumerate(probs):
        _, rho0, scale0 = residual_dd(prob, z0[p])
        ref1, rho1, scale1 = residual_dd(prob, z1[p])
        assert before[p] == eta(rho0, scale0), (p, before[p], eta(rho0, scale0))
        if steps[p] == 1:
            assert after[p] == eta(rho1, scale1), (p, after[p], eta(rho1, scale1))
            assert rho1 < rho0, (p, rho0, rho1)
        else:
            assert z1[p].tobytes() == z0[p].tobytes() and after[p] == before[p], p
        assert np.array_equal(r1[p], ref1), (p, np.max(np.abs(r1[p] - ref1)))
    bs.close()


# ------------------------------------------------------------------------------------ 3. kkt_residual_generic

def _perturbed(base, p, name, k, i, delta):
    """(the four stacked right-hand-side arrays with `delta` added to one entry of problem p, the difference stored)"""
    arrs = {key: a.copy() for key, a in base.items()}
    at = (p, i) if name == "x0" else (p, k, i)
    old = arrs[name][at]
    arrs[name][at] = old + delta
    return [arrs[key] for key in RHS], float(arrs[name][at] - old)


def _positions(n, m, N):
    """(name, knot, entry) of the right-hand-side entries that are rows of the system, at the first and the last entry of
    a block and the first, a middle and the last knot that has the row; and the entries of r that are no row."""
    ii, jj = sorted({0, n - 1}), sorted({0, m - 1})
    rows = [("x0", None, i) for i in ii]
    rows += [("d", k, i) for k in sorted({0, N // 2, N - 2}) for i in ii]
    rows += [("q", k, i) for k in sorted({0, N // 2, N - 1}) for i in ii]
    rows += [("r", k, i) for k in sorted({0, N - 2}) for i in jj]
    return rows, [("r", N - 1, i) for i in jj]


@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 3), (7, 9, 16, 3), (1, 1, 8, 3), (64, 16, 32, 3), (130, 5, 4, 3),
                                         (144, 16, 8, 3), (256, 32, 4, 3), (6, 3, 8192, 2)])
def test_norm_kernel_counts_every_row_once(ndlqr, n, m, N, batch):
    first = [synth(ndlqr, n, m, N, 40 + p) for p in range(batch)]
    other = [synth(ndlqr, n, m, N, 90 + p) for p in range(batch)]
    bs = solver(ndlqr, first, 0)
    sol = bs.solutions().copy()
    # (a) the suite's bound on the solution
    res0, bn0 = bs.kkt_residuals()
    bound = 1e-9 * np.maximum(1.0, bn0)
    print((n, m, N), "res", res0.tolist(), "bn", bn0.tolist())
    assert np.all(res0 <= bound), (res0, bound)
    for p, prob in enumerate(first):
        assert abs(bn0[p] - norm_ld(rhs_ld(prob))) <= 1e-10 * bn0[p]
    # (b) the coefficients: a stale solution against another right-hand side
    bs.set_rhs_flat(*[np.stack([getattr(pr, key) for pr in other]) for key in RHS])
    res, bn = bs.kkt_residuals()
    for p in range(batch):
        _, _, want_res, want_bn = kkt_rows_ld(mixed_problem(first[p], other[p]), sol[p])
        assert want_res > 1e-3
        assert abs(res[p] - want_res) <= 1e-10 * want_res, (p, res[p], float(want_res))
        assert abs(bn[p] - want_bn) <= 1e-10 * want_bn, (p, bn[p], float(want_bn))
    # (c) one row at a time, on problem 1
    base = {key: np.stack([getattr(pr, key) for pr in first]) for key in RHS}
    bs.set_rhs_flat(*[base[key] for key in RHS])
    res_u, bn_u = bs.kkt_residuals()
    assert np.all(res_u <= bound)
    delta = 2.0 ** round(np.log2(max(1.0, bn_u[1]) / 16))
    others = [p for p in range(batch) if p != 1]
    rows, no_rows = _positions(n, m, N)
    for name, k, i in rows:
        arrs, stored = _perturbed(base, 1, name, k, i, delta)
        bs.set_rhs_flat(*arrs)
        res, bn = bs.kkt_residuals()
        where = (name, k, i, res[1], stored)
        assert abs(res[1] / abs(stored) - 1.0) <= 1e-7, where
        moved = Problem(n, m, N, first[1].A, first[1].B, first[1].Q, first[1].R, *[a[1] for a in arrs])
        want_bn = norm_ld(rhs_ld(moved))
        assert abs(bn[1] - want_bn) <= 1e-10 * want_bn, where
        assert res[others].tobytes() == res_u[others].tobytes() and bn[others].tobytes() == bn_u[others].tobytes(), where
    # (d) the slot that is not a row
    for name, k, i in no_rows:
        arrs, stored = _perturbed(base, 1, name, k, i, delta)
        assert stored != 0.0
        bs.set_rhs_flat(*arrs)
        res, bn = bs.kkt_residuals()
        assert res[1] <= bound[1], (name, k, i, res[1])
        assert abs(bn[1] - bn_u[1]) <= 1e-12 * bn_u[1], (name, k, i, bn[1], bn_u[1])
    bs.close()


# ------------------------------------------------------------------------------------ 4. strict-mode termination

@pytest.mark.parametrize("n,m,N,seed", BOX_TERMINATION_CASES)
def test_strict_box_solve_terminates_like_the_restatement(ndlqr, oracle, n, m, N, seed):
    """With tolerances that trigger (1e-4, checked every iteration), both problems of a pair stop by convergence at
    iteration counts of their own: iters, status, the iterate and the multipliers equal the numpy restatement driving the
    oracle, bit for bit."""
    probs, (xlo, xhi, ulo, uhi), ref = box_termination_reference(ndlqr, oracle, n, m, N, seed)
    s = BOX_TERMINATION
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    bs.initialize_flat(*stack(probs))
    bs.set_bounds(xlo, xhi, ulo, uhi)
    it, st = bs.solve_box(rho=s["rho"], alpha=s["alpha"], eps_abs=s["eps_abs"], eps_rel=s["eps_rel"], max_iter=s["max_iter"],
                          check_every=1)
    sol = bs.solutions()
    mux, muu = bs.bound_multipliers()
    print((n, m, N), "iterations", it.tolist(), "status", st.tolist(), "restatement", [(r[5], r[6]) for r in ref])
    for p in range(len(probs)):
        x, u, rx, ru, lam, rit, rst = ref[p]
        assert rst == 1 and rit < s["max_iter"]
        assert it[p] == rit and st[p] == rst, (p, it[p], rit, st[p], rst)
        lg, xg, ug = split(sol[p], n, m, N)
        assert np.array_equal(xg, x) and np.array_equal(ug, u[: N - 1]) and np.array_equal(lg, lam), p
        assert np.array_equal(mux[p], rx) and np.array_equal(muu[p], ru), p
    bs.close()
