"""The device-side gradients of dense-cost and constrained batch solves (ndlqr_BatchGradientsDense, BatchSolver.
gradients_dense) against grad_dense_support.py -- the numpy restatement with strict mode's
operation order, on the device's own z and w -- and against cost_support.gradient_reference on the refined z and w.
Batch 3 unless stated; the shapes and horizons of cost_support.py ((7,9): n < m; N = 2: one dynamics knot, 5: padded,
16: two chunks of knots) and the constrained cases of lin_grad_support.py.

Bars. Strict mode: bit for bit. Default mode, per entry: 2 eps (|t1| + |t2|) against the strict restatement on the same z, w
-- the rounding of one contracted against one uncontracted sum; Q, R and the vectors are not contracted and stay bit for
bit. Against the independent reference: GRAD_TOL = 1e-8 in the relative norm per output, the bar test_gpu_cost.py holds
lqr_solve_dense to. Batch sums, per entry: batch eps sum |per-problem| against the exactly rounded sum of the per-problem
outputs, and two calls give the same bits.

The flags of the default-mode cases are cost_support's keep rule (test_gpu_cost.keep_flags): NDLQR_FLAG_KEEP_RECORDS, but
NDLQR_FLAG_KEEP_FACT at N = 2, where the device horizon has no record-based re-solve and the adjoint needs the factor array;
neither flag is strict mode, so A, B, H are contracted there too."""
import ctypes as C

import numpy as np
import pytest

import cost_support as cs
import grad_dense_support as gd
import lin_grad_support as lg
import lin_support as ls

pytestmark = pytest.mark.gpu

EPS = gd.EPS
GRAD_TOL = 1e-8
CASES = [(n, m, N) for (n, m) in cs.SHAPES for N in cs.HORIZONS]
LIN_CASES = [(6, 3, 5), (12, 4, 8), (7, 9, 16), (20, 5, 2)]
LIN_SET = dict(rho=ls.RHO, alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=2000)
ADJ_SET = dict(alpha=ls.ALPHA, eps_abs=1e-8, eps_rel=1e-8, max_iter=2000)
WHO = "ndlqr_hip_gradients_dense: "


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def fast_flags(ndlqr, N):
    # (a device horizon below 8 has no record-based re-solve: the factor array there, as test_gpu_cost.keep_flags)
    return ndlqr.FLAG_KEEP_FACT if N < 5 else ndlqr.FLAG_KEEP_RECORDS


def dense_solved(ndlqr, probs, flags, g):
    """dense initialise, solve, adjoint"""
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat_dense(*cs.flat(probs))
    assert bs.solve() == 0 and bs.cholesky_failures() == 0
    assert bs.solve_adjoint(np.ascontiguousarray(g)) == 0, bs.L.ndlqr_hip_last_error().decode()
    return bs


def lin_solved(ndlqr, cases, flags):
    """constrained initialise, constrained solve, constrained adjoint; returns (solver, forward status, adjoint status)"""
    probs = [c["p"] for c in cases]
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat_constrained(*cs.flat(probs), *ls.flat_rows(cases))
    _, fstatus = bs.solve_constrained(**LIN_SET)
    _, status = bs.solve_constrained_adjoint(np.stack([c["g"] for c in cases]), **ADJ_SET)
    return bs, fstatus, status


def check_against_restatement(bs, got, strict, label, skipped=None):
    """per-problem outputs against the restatement on the solver's own z and w (skipped: the members a constrained adjoint
    did not iterate -- exact zeros)"""
    n, m, N = bs.n, bs.m, bs.N
    ref, mag = gd.restate(bs.solutions(), bs.adjoint(), n, m, N, mags=True)
    for i in ([] if skipped is None else np.flatnonzero(skipped)):
        for k in gd.NAMES:
            ref[k][i] = 0.0
    for k in gd.NAMES:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), k
        if strict or k not in ("A", "B", "H"):
            assert same_bits(got[k], ref[k]), (label, k, float(np.abs(got[k] - ref[k]).max()))
        else:
            over = np.abs(got[k] - ref[k]) - 2 * EPS * mag[k]
            print(label, k, "largest |fast - strict| / (eps (|t1| + |t2|)): %.3f"
                  % float((np.abs(got[k] - ref[k]) / np.maximum(EPS * mag[k], np.finfo(float).tiny)).max()))
            assert (over <= 0).all(), (label, k, float(over.max()))
    for k in ("Q", "R"):
        r = gd.rows_of(k, n, m)
        M = got[k].reshape(bs.batch, N, r, r)
        assert same_bits(M, M.transpose(0, 1, 3, 2)), (label, k)
    for k in ("A", "B", "H", "R", "r", "d"):
        assert same_bits(got[k][:, N - 1], np.zeros_like(got[k][:, N - 1])), (label, k)
    return ref


def check_sums(per, summed, batch, label):
    """|s - fsum(per-problem)| <= batch eps sum |per-problem| per entry"""
    for k in summed:
        exact = gd.fsum(per[k])
        bar = batch * EPS * np.abs(per[k]).sum(axis=0)
        assert summed[k].shape == exact.shape, (label, k)
        assert (np.abs(summed[k] - exact) <= bar).all(), (label, k, float((np.abs(summed[k] - exact) - bar).max()))


# ---------------------------------------------------------------------------- 1, 2: per-problem outputs, both FP modes
@pytest.mark.parametrize("n,m,N", CASES)
def test_strict_mode_bit_for_bit(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solved(ndlqr, fam["probs"], ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT, fam["g"])
    got = bs.gradients_dense()
    assert bs.solve_ms() > 0
    check_against_restatement(bs, got, True, "strict %s" % ((n, m, N),))
    bs.close()


@pytest.mark.parametrize("n,m,N", CASES)
def test_default_mode_per_entry(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solved(ndlqr, fam["probs"], fast_flags(ndlqr, N), fam["g"])
    got = bs.gradients_dense()
    check_against_restatement(bs, got, False, "default %s" % ((n, m, N),))
    bs.close()


# ---------------------------------------------------------------------------- 3: the independent reference
@pytest.mark.parametrize("n,m,N", CASES)
def test_against_the_independent_reference(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solved(ndlqr, fam["probs"], fast_flags(ndlqr, N), fam["g"])
    got = bs.gradients_dense()
    bs.close()
    for i, p in enumerate(fam["probs"]):
        ref = cs.gradient_reference(p, fam["z"][i], fam["w"][i])
        for k in gd.NAMES:
            a = gd.to_math(k, got[k][i], n, m)
            assert a.shape == ref[k].shape, k
            err = float(np.linalg.norm(a - ref[k]) / np.linalg.norm(ref[k]))
            print("reference", (n, m, N), i, k, "%.3e" % err)
            assert err <= GRAD_TOL, (i, k, err)


# ---------------------------------------------------------------------------- 4: batch sums
ALL = (1 << 9) - 1


@pytest.mark.parametrize("n,m,N", [(6, 3, 2), (12, 4, 5), (7, 9, 16), (20, 5, 8), (32, 8, 16)])
def test_batch_sums(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    for flags in (ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT, fast_flags(ndlqr, N)):
        bs = dense_solved(ndlqr, fam["probs"], flags, fam["g"])
        per = bs.gradients_dense()
        summed = bs.gradients_dense(ALL)
        again = bs.gradients_dense(ALL)
        check_sums(per, summed, cs.BATCH, (n, m, N, flags))
        for k in gd.NAMES:
            assert same_bits(summed[k], again[k]), k
            # (three problems: by WORKGROUPS every workgroup row holds one, and the split pass adds them in order)
            assert same_bits(summed[k], gd.ordered_sum(per[k])), k
        # mixed masks: A, B, x0 summed with the rest per problem, and the reverse
        abx = ndlqr.GRADD_A | ndlqr.GRADD_B | ndlqr.GRADD_x0
        for mask in (abx, ALL & ~abx):
            mixed = bs.gradients_dense(mask)
            for i, k in enumerate(gd.NAMES):
                assert same_bits(mixed[k], summed[k] if mask & (1 << i) else per[k]), (mask, k)
        bs.close()


def test_batch_sum_over_rows_and_splits(ndlqr):
    """The smallest shape at a batch where a workgroup row sums more than one problem AND the split pass runs: at (6,3,16)
    a sum runs in ceil(16 / CHUNK) = 2 chunks, so the batch is split into at most WORKGROUPS / 2 = 1024 rows; 1536 problems
    make 768 rows of two problems each."""
    n, m, N = 6, 3, 16
    nchunks = -(-N // gd.CHUNK)
    rows_max = gd.WORKGROUPS // nchunks
    batch = rows_max + rows_max // 2
    ppb = -(-batch // rows_max)
    assert ppb == 2 and -(-batch // ppb) > 1
    consts = (C.c_int * 2)()
    assert ndlqr.lib().ndlqr_hip_gradients_dense_constants(consts) == 0 and list(consts) == [gd.WORKGROUPS, gd.CHUNK]
    # the three problems of the family, each with right-hand sides and g of its own per copy
    fam = cs.family(n, m, N, "moderate")
    rng = np.random.default_rng([n, m, N, batch])
    arrs = [np.ascontiguousarray(np.tile(a, (batch // cs.BATCH,) + (1,) * (a.ndim - 1))) for a in cs.flat(fam["probs"])]
    for a in arrs[5:]:
        a += 0.5 * rng.standard_normal(a.shape)
    g = rng.standard_normal((batch, (2 * n + m) * N - m))
    for flags in (ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT, ndlqr.FLAG_KEEP_RECORDS):
        bs = ndlqr.BatchSolver(n, m, N, batch, flags=flags)
        bs.initialize_flat_dense(*arrs)
        assert bs.solve() == 0 and bs.solve_adjoint(g) == 0
        per = bs.gradients_dense()
        summed = bs.gradients_dense(ALL)
        again = bs.gradients_dense(ALL)
        if flags & ndlqr.FLAG_STRICT_FP:
            ref = gd.restate(bs.solutions(), bs.adjoint(), n, m, N)
            for k in gd.NAMES:
                assert same_bits(per[k], ref[k]), k
        check_sums(per, summed, batch, ("rows and splits", flags))
        for k in gd.NAMES:
            assert same_bits(summed[k], again[k]), k
            # the device's own order: pairs in order, then the pairs in order
            pairs = np.stack([gd.ordered_sum(per[k][i:i + ppb]) for i in range(0, batch, ppb)])
            assert same_bits(summed[k], gd.ordered_sum(pairs)), k
        mixed = bs.gradients_dense(ndlqr.GRADD_A | ndlqr.GRADD_q)
        for i, k in enumerate(gd.NAMES):
            assert same_bits(mixed[k], summed[k] if k in ("A", "q") else per[k]), k
        bs.close()


# ---------------------------------------------------------------------------- 5: destinations
class Sub:
    """a range of a DeviceArray as a destination"""

    def __init__(self, dev, start, size):
        self.ptr, self.size = dev.ptr + 8 * start, size


@pytest.mark.parametrize("n,m,N", [(7, 9, 5), (12, 4, 16)])
def test_destinations(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solved(ndlqr, fam["probs"], fast_flags(ndlqr, N), fam["g"])
    mask = ndlqr.GRADD_B | ndlqr.GRADD_Q | ndlqr.GRADD_d
    ref = bs.gradients_dense(mask)
    shapes = {k: bs.dense_gradient_shape(k, bool(mask & (1 << i))) for i, k in enumerate(gd.NAMES)}
    pinned = {k: ndlqr.pinned_empty(shapes[k]) for k in gd.NAMES}
    for a in pinned.values():
        a[...] = np.nan
    bs.gradients_dense(mask, pinned)
    dev = {k: ndlqr.DeviceArray(shapes[k]).set(np.full(shapes[k], np.nan)) for k in gd.NAMES}
    bs.gradients_dense(mask, dev)
    for k in gd.NAMES:
        assert same_bits(pinned[k], ref[k]) and same_bits(dev[k].get(), ref[k]), k
    # a subset of the names, as ranges of one NaN-filled device array with a guard between them: only those are written
    guard = 64
    off, at = {}, guard
    for k in gd.NAMES:
        off[k] = at
        at += int(np.prod(shapes[k])) + guard
    whole = ndlqr.DeviceArray((at,)).set(np.full(at, np.nan))
    subset = ("B", "R", "q", "x0")
    bs.gradients_dense(mask, {k: Sub(whole, off[k], int(np.prod(shapes[k]))) for k in subset})
    back = whole.get()
    written = np.zeros(at, dtype=bool)
    for k in subset:
        size = int(np.prod(shapes[k]))
        assert same_bits(back[off[k]:off[k] + size].reshape(shapes[k]), ref[k]), k
        written[off[k]:off[k] + size] = True
    assert np.isnan(back[~written]).all()
    host = {k: np.full(shapes[k], np.nan) for k in ("A", "H")}
    bs.gradients_dense(mask, host)
    for k in host:
        assert same_bits(host[k], ref[k]), k
    with pytest.raises(ValueError):
        bs.gradients_dense(0, dict(C=np.zeros(3)))
    with pytest.raises(ValueError):
        bs.gradients_dense(0, dict(A=np.zeros(3)))
    bs.close()


# ---------------------------------------------------------------------------- 6: constrained mode
@pytest.mark.parametrize("n,m,N", LIN_CASES)
def test_constrained_mode(ndlqr, n, m, N):
    cases = lg.case(n, m, N)
    for flags in (0, ndlqr.FLAG_STRICT_FP):
        bs, fstatus, status = lin_solved(ndlqr, cases, flags)
        got = bs.gradients_dense()
        check_against_restatement(bs, got, bool(flags & ndlqr.FLAG_STRICT_FP), "constrained %s flags %d" % ((n, m, N), flags),
                                  skipped=status == 3)
        summed = bs.gradients_dense(ALL)
        check_sums(got, summed, len(cases), ("constrained", n, m, N, flags))
        for k in gd.NAMES:
            assert same_bits(summed[k], bs.gradients_dense(ALL)[k]), k
        bs.close()


def test_constrained_after_a_plain_solve_gives_the_unconstrained_answers(ndlqr):
    n, m, N = 12, 4, 8
    cases = lg.case(n, m, N)
    probs = [c["p"] for c in cases]
    G = np.stack([c["g"] for c in cases])
    flags = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT
    bs = ndlqr.BatchSolver(n, m, N, len(cases), flags=flags)
    bs.initialize_flat_constrained(*cs.flat(probs), *ls.flat_rows(cases))
    assert bs.solve() == 0 and bs.solve_adjoint(G) == 0
    got = bs.gradients_dense()
    check_against_restatement(bs, got, True, "constrained mode, plain solve")
    bs.close()
    plain = dense_solved(ndlqr, probs, flags, G)
    ref = plain.gradients_dense()
    plain.close()
    for k in gd.NAMES:
        assert same_bits(got[k], ref[k]), k


def test_constrained_with_a_member_that_is_not_finite(ndlqr):
    """The batch of test_gpu_lin_gradients.test_a_forward_that_is_not_finite: problem 1 ends its forward as 3 and is not
    iterated by the adjoint -- exact zeros in its outputs, and the sums are those of the other members."""
    n, m, N = 6, 3, 8
    cases = lg.case(n, m, N)
    bad = [dict(c) for c in cases]
    bad[1] = dict(bad[1], p=dict(bad[1]["p"], q=bad[1]["p"]["q"].copy()))
    bad[1]["p"]["q"][3, 2] = np.nan
    for flags in (0, ndlqr.FLAG_STRICT_FP):
        good, _, _ = lin_solved(ndlqr, cases, flags)
        ref = good.gradients_dense()
        good.close()
        bs, fstatus, status = lin_solved(ndlqr, bad, flags)
        assert fstatus[1] == 3 and status[1] == 3 and list(status[[0, 2]]) == [1, 1]
        got, summed = bs.gradients_dense(), bs.gradients_dense(ALL)
        bs.close()
        for k in gd.NAMES:
            assert same_bits(got[k][1], np.zeros_like(got[k][1])), k
            for i in (0, 2):  # the others bit for bit as without it
                assert same_bits(got[k][i], ref[k][i]), (k, i)
            assert same_bits(summed[k], gd.ordered_sum(got[k][[0, 2]])), k


# ---------------------------------------------------------------------------- 7: nothing moves
def test_nothing_moves_dense(ndlqr):
    n, m, N = 12, 4, 16
    fam = cs.family(n, m, N, "moderate")
    for flags in (ndlqr.FLAG_KEEP_RECORDS, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT):
        a = dense_solved(ndlqr, fam["probs"], flags, fam["g"])
        b = dense_solved(ndlqr, fam["probs"], flags, fam["g"])
        before = (a.solutions(), a.adjoint(), a.factor_count())
        a.gradients_dense(); a.gradients_dense(ALL); a.gradients_dense(ndlqr.GRADD_A, dict(A=np.zeros((N, n * n))))
        assert same_bits(a.solutions(), before[0]) and same_bits(a.adjoint(), before[1]) and a.factor_count() == before[2]
        assert same_bits(before[0], b.solutions()) and same_bits(before[1], b.adjoint())
        for bs in (a, b):
            assert bs.solve_rhs_only() == 0
        assert same_bits(a.solutions(), b.solutions()) and a.factor_count() == b.factor_count()
        a.close(); b.close()


def test_nothing_moves_constrained(ndlqr):
    n, m, N = 12, 4, 8
    cases = lg.case(n, m, N)
    C, D, lo, hi = ls.flat_rows(cases)
    for flags in (0, ndlqr.FLAG_STRICT_FP):
        a, _, _ = lin_solved(ndlqr, cases, flags)
        b, _, _ = lin_solved(ndlqr, cases, flags)
        state = lambda bs: (bs.solutions(), bs.adjoint(), bs.constraint_multipliers(), bs.constraint_residuals(),
                            bs.constraint_adjoint_multipliers())
        before, count = state(a), a.factor_count()
        a.gradients_dense(); a.gradients_dense(ALL)
        after = state(a)
        assert a.factor_count() == count
        for x, y in zip(before, after):
            assert same_bits(x, y)
        # the row gradients and a warm-started forward behind it equal those of a solver that never made the call
        ga, gb = a.constraint_gradients(), b.constraint_gradients()
        for k in ga:
            assert same_bits(ga[k], gb[k]), k
        for bs in (a, b):
            bs.set_constraint_bounds(1.05 * lo, 1.05 * hi)
        ra = a.solve_constrained(warm_start=True, **LIN_SET)
        rb = b.solve_constrained(warm_start=True, **LIN_SET)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        assert same_bits(a.solutions(), b.solutions()) and a.factor_count() == b.factor_count()
        a.close(); b.close()


# ---------------------------------------------------------------------------- 8: refusals by name
def refused(bs, *args, **kw):
    with pytest.raises(RuntimeError, match="ndlqr_BatchGradientsDense failed: -1"):
        bs.gradients_dense(*args, **kw)
    msg = bs.L.ndlqr_hip_last_error().decode()
    assert msg.startswith(WHO), msg
    return msg


def test_refusals_by_name(ndlqr):
    n, m, N = 6, 3, 5
    cases = lg.case(n, m, N)
    probs = [c["p"] for c in cases]
    G = np.stack([c["g"] for c in cases])
    C, D, lo, hi = ls.flat_rows(cases)
    flags = ndlqr.FLAG_KEEP_RECORDS
    # diagonal mode
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH, flags=flags)
    gen = [ndlqr.generate_synthetic(n, m, N, 60 + i) for i in range(cs.BATCH)]
    bs.initialize_flat(*[np.stack([g[k] for g in gen]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")])
    assert bs.solve() == 0 and bs.solve_adjoint(G) == 0
    assert "ndlqr_BatchGradients" in refused(bs) and "dense-cost" in bs.L.ndlqr_hip_last_error().decode()
    bs.gradients()  # (the diagonal gradients are there)
    # dense mode: no adjoint yet; after a new solve; after a re-solve; after a new right-hand side
    bs.initialize_flat_dense(*cs.flat(probs))
    assert bs.solve() == 0
    assert "no adjoint of the resident solution" in refused(bs)
    assert bs.solve_adjoint(G) == 0
    bs.gradients_dense()
    refused(bs, 1 << 9)
    assert "sum_mask" in refused(bs, (1 << 9) | 1)
    assert bs.solve() == 0
    assert "no adjoint of the resident solution" in refused(bs)
    assert bs.solve_adjoint(G) == 0 and bs.solve_rhs_only() == 0
    assert "no adjoint of the resident solution" in refused(bs)
    assert bs.solve_adjoint(G) == 0
    q, r, d, x0 = cs.flat(probs, ("q", "r", "d", "x0"))
    bs.set_rhs_flat(q, r, d, x0)
    assert "right-hand side" in refused(bs)
    assert bs.solve_rhs_only() == 0 and bs.solve_adjoint(G) == 0
    bs.gradients_dense()
    bs.close()
    # constrained mode
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH, flags=flags)
    bs.initialize_flat_constrained(*cs.flat(probs), C, D, lo, hi)
    assert bs.solve() == 0 and bs.solve_adjoint(G) == 0
    bs.gradients_dense()
    # ... a plain adjoint's gradients after a constrained solve, with no constrained adjoint
    bs.solve_constrained(**LIN_SET)
    assert "no constrained adjoint" in refused(bs)
    bs.solve_constrained_adjoint(G, **ADJ_SET)
    bs.gradients_dense()
    bs.set_rhs_flat(q, r, d, x0)
    assert "no constrained adjoint" in refused(bs)
    bs.solve_constrained(**LIN_SET)
    bs.solve_constrained_adjoint(G, **ADJ_SET)
    bs.gradients_dense()
    bs.set_constraint_bounds(lo, hi)
    assert "no constrained adjoint" in refused(bs)
    bs.solve_constrained(**LIN_SET)
    assert "no constrained adjoint" in refused(bs)
    # memory of another device: needs a second GPU; on a box with one MI355X this refusal is NOT exercised (the
    # CallerArrays path it takes is the one ndlqr_hip_gradients' refusal shares)
    if ndlqr.device_count() > 1:
        import torch

        class Foreign:
            def __init__(self, shape):
                self.t = torch.zeros(shape, dtype=torch.float64, device="cuda:1")
                self.ptr, self.size = self.t.data_ptr(), self.t.numel()
        bs.solve_constrained_adjoint(G, **ADJ_SET)
        assert "an output lies in the memory of another device" in refused(bs, 0, dict(q=Foreign((cs.BATCH, N, n))))
    bs.close()


# ---------------------------------------------------------------------------- 9: lqr_solve_dense, shared arguments
# torch runs in a child process (test_gpu_gradients.py has the reason: torch's own HIP runtime must start first)
def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_grad_dense as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _case_shared_arguments(ndlqr, n, m, N):
    import torch
    from rslqr_amd.autograd import lqr_solve_dense
    fam = cs.family(n, m, N, "moderate")
    sh = ("A", "q")
    probs = [dict(p, A=fam["probs"][0]["A"], q=fam["probs"][0]["q"]) for p in fam["probs"]]
    g = torch.tensor(fam["g"], device="cuda")

    def leaves(need):
        out = {}
        for k in cs.NAMES:
            a = probs[0][k] if k in sh else np.stack([p[k] for p in probs])
            out[k] = torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=k in need)
        return out

    refs = []
    for i, p in enumerate(probs):
        K, b = cs.dense_kkt(p)
        refs.append(cs.gradient_reference(p, cs.refined_solve(K, b), cs.refined_solve(K, fam["g"][i])))
    # every gradient: the shared ones against the summed references, the others per problem
    t = leaves(cs.NAMES)
    z = lqr_solve_dense(*[t[k] for k in cs.NAMES])
    (z * g).sum().backward()
    for k in cs.NAMES:
        assert t[k].grad.shape == t[k].shape, k
        want = sum(r[k] for r in refs) if k in sh else np.stack([r[k] for r in refs])
        err = rel(t[k].grad.cpu().numpy(), want)
        print("shared", (n, m, N), k, "%.3e" % err)
        assert err <= GRAD_TOL, (k, err)
    for k in ("Q", "R"):
        got = t[k].grad.cpu().numpy()
        assert np.array_equal(got, got.transpose(0, 1, 3, 2)), k
    # only the shared A needs a gradient: the backward must not materialise a per-problem gA [b, N, n, n] (four copies of
    # the batch, so that the summed gA [N, n, n] and dL/dz are small against it)
    copies = 4
    t = leaves(("A",))
    for k in cs.NAMES:
        if k not in sh:
            t[k] = t[k].detach().repeat(copies, *[1] * (t[k].dim() - 1))
    z = lqr_solve_dense(*[t[k] for k in cs.NAMES])
    loss = (z * g.repeat(copies, 1)).sum()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    per_problem = copies * cs.BATCH * N * n * n * 8
    print("backward of the shared A alone: max_memory_allocated delta %d bytes, one [b, N, n, n] tensor %d" % (delta, per_problem))
    assert delta < per_problem, (delta, per_problem)
    assert all(t[k].grad is None for k in cs.NAMES if k != "A")
    assert rel(t["A"].grad.cpu().numpy(), copies * sum(r["A"] for r in refs)) <= GRAD_TOL


@pytest.mark.parametrize("n,m,N", [(12, 4, 8)])
def test_lqr_solve_dense_sums_shared_arguments_on_the_device(n, m, N):
    _run_case("_case_shared_arguments", n, m, N)
