"""The references of tests/test_gpu_box_update.py, the CPU side (no GPU): the new getters are exported and refuse a NULL
solver; the per-iteration restatement of box_update_support.py is the existing one (box_support.admm_reference,
box_grad_support.adjoint_admm_reference) at its last iteration, bit for bit; the conditions on the seeds that the GPU
cases rely on; the launch table their shapes were chosen by; and the premises of the planted cases."""
import ctypes as C

import numpy as np
import pytest

from box_adaptive_support import admm_adaptive_reference
from box_grad_support import active_codes, adjoint_admm_reference, full_bounds
from box_support import admm_reference
from box_update_support import (ALPHA, PLANT_RHO, RHO, addressable, adjoint_trace, classes, entry_class, forward_trace,
                                loose_bounds, mixed_bounds, oracle_solve, padded_offset, pinned_entry, planted,
                                planted_positions, update_launch)
from test_box_host import synth
from test_gpu_box_update import (ADAPT_SEEDS, ADJOINT_SHAPES, COUNT_SHAPES, SEEDS, SHAPES, TERMINATION, TERMINATION_SHAPES, WARM_SHAPES,
                                 delivered, packed)


# ------------------------------------------------------------------------------------------------ 1. symbols and layout

def test_the_new_getters_are_exported_and_refuse_a_null_solver(ndlqr):
    L = ndlqr.lib()
    buf = np.zeros(4)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    for name in ("ndlqr_CopyBatchBoxResiduals", "ndlqr_CopyBatchBoxAdjointResiduals", "ndlqr_hip_download_box_residuals",
                 "ndlqr_hip_download_box_adjoint_residuals"):
        assert name in ndlqr.exported_symbols()
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        # (no device here, so no solver: every call is refused; test_gpu_box_update.py sends them to a real one)
        assert fn(None, dp) == ndlqr.api.ERR_INVALID, name
    assert (buf == 0).all()
    # a row is four doubles: what BatchSolver.box_residuals() allocates for a batch of 3, and asks of a destination
    import types
    bs = ndlqr.api.BatchSolver.__new__(ndlqr.api.BatchSolver)
    bs.batch, bs.h, bs.L = 3, None, types.SimpleNamespace(ndlqr_CopyBatchBoxResiduals=lambda h, p: 0)
    given = np.zeros(4 * 3)
    assert bs.box_residuals().shape == (3, 4) and bs.box_residuals(given) is given
    for bad in (np.zeros(4 * 3 - 1), np.zeros(4 * 3 + 1)):
        with pytest.raises(ValueError, match="expected a C-contiguous float64 array of 12 doubles"):
            bs.box_residuals(bad)


# ------------------------------------------------------------------------------------------------ 2. the restatement is the old one

@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (7, 9, 16), (6, 3, 4)])
def test_the_trace_is_the_existing_reference_at_its_last_iteration(ndlqr, oracle, n, m, N):
    solve = oracle_solve(oracle)
    prob = synth(ndlqr, n, m, N, 80)
    b = mixed_bounds(oracle, prob)
    M = full_bounds(n, m, N, *b)[2]
    for iters, eps in ((1, 1e-300), (3, 1e-300), (400, 1e-4)):
        ref = admm_reference(prob, solve, *b, RHO, ALPHA, eps, eps, iters)
        tr = forward_trace(prob, solve, b, iters, eps=eps)
        assert len(tr.its) == ref[5] == tr.iters and tr.status == ref[6]
        assert [s["it"] for s in tr.its] == list(range(1, ref[5] + 1))
        assert all(not s["conv"] for s in tr.its[:-1]) and tr.its[-1]["conv"] == (ref[6] == 1)
        got = delivered(tr, ref[5], M, RHO)
        for a, r in zip(got, ref[:5]):
            assert a.tobytes() == r.tobytes()
        # every earlier iteration is the reference stopped there
        if iters == 3:
            for k in (1, 2):
                rk = admm_reference(prob, solve, *b, RHO, ALPHA, eps, eps, k)
                for a, r in zip(delivered(tr, k, M, RHO), rk[:5]):
                    assert a.tobytes() == r.tobytes()
    # a start from the state of two iterations continues the cold run
    two = forward_trace(prob, solve, b, 2)
    more = forward_trace(prob, solve, b, 2, start=two.state())
    four = forward_trace(prob, solve, b, 4)
    assert more.x.tobytes() == four.x.tobytes() and more.mu_u.tobytes() == four.mu_u.tobytes()
    assert more.resid.tobytes() == four.resid.tobytes()
    # the box adjoint
    codes = active_codes(prob, packed(prob, forward_trace(prob, solve, b, 3)), *b)
    g = np.random.default_rng(7).standard_normal(prob.nvars)
    for iters in (1, 3):
        ref = adjoint_admm_reference(prob, solve, codes, g, RHO, ALPHA, 1e-300, 1e-300, iters)
        at = adjoint_trace(prob, solve, codes, g, iters)
        assert at.w.tobytes() == ref[0].tobytes() and at.nu.tobytes() == ref[1].tobytes() and (at.iters, at.status) == ref[2:]
        assert len(at.its) == iters


def test_the_four_numbers_are_those_of_the_definition(ndlqr, oracle):
    """r_prim | r_dual | sp | sd recomputed from the trace's own z, v, y with plain np.max over the bounded entries"""
    n, m, N = 7, 9, 16
    prob = synth(ndlqr, n, m, N, 81)
    b = mixed_bounds(oracle, prob)
    M = full_bounds(n, m, N, *b)[2]
    tr = forward_trace(prob, oracle_solve(oracle), b, 3)
    v_prev = np.zeros((N, n + m))
    for s in tr.its:
        z = s["Z"][:, n:]
        want = (np.max(np.abs(z - s["v"])[M]), RHO * np.max(np.abs(s["v"] - v_prev)[M]),
                max(np.max(np.abs(z)[M]), np.max(np.abs(s["v"])[M])), RHO * np.max(np.abs(s["y"])[M]))
        assert s["resid"] == want
        v_prev = s["v"]


# ------------------------------------------------------------------------------------------------ 3. conditions on the seeds

def test_the_mixed_pattern_is_the_one_described(ndlqr, oracle):
    n, m, N = 12, 4, 16
    prob = synth(ndlqr, n, m, N, 80)
    xlo, xhi, ulo, uhi = mixed_bounds(oracle, prob)
    lo, hi = np.concatenate([xlo, ulo], axis=1), np.concatenate([xhi, uhi], axis=1)
    c = entry_class(n, m, N)
    assert (np.isinf(lo) == ((c == 1) | (c == 3))).all() and (np.isinf(hi) == ((c == 2) | (c == 3))).all()
    k, j = pinned_entry(n, m, N)
    assert c[k, j] == 0 and j >= n and addressable(n, m, N)[k, j] and lo[k, j] == hi[k, j] > 0
    assert ((lo == hi).sum() == 1) and (lo[c == 0] <= hi[c == 0]).all()
    both = (c == 0) & ~(lo == hi)
    assert (lo[both] == -hi[both]).all()
    # scaling keeps the pattern, releasing changes it in every knot
    s = mixed_bounds(oracle, prob, scale=0.9)
    assert all((np.isfinite(a) == np.isfinite(b_)).all() for a, b_ in zip(s, (xlo, xhi, ulo, uhi)))
    assert np.array_equal(s[1][np.isfinite(xhi)], 0.9 * xhi[np.isfinite(xhi)])
    r = mixed_bounds(oracle, prob, scale=0.9, release=True)
    gone = np.concatenate([np.isfinite(xhi) & ~np.isfinite(r[1]), np.isfinite(uhi) & ~np.isfinite(r[3])], axis=1)
    gone &= addressable(n, m, N)
    # (one per knot, except where the pinned entry is the knot's only two-sided one)
    assert (gone.sum(axis=1) <= 1).all() and gone.sum() >= N - 2 and (c[gone] == 0).all() and not gone[k, j]


def _all_cases():
    shapes = list(dict.fromkeys(SHAPES + WARM_SHAPES + ADJOINT_SHAPES))
    return [(shape, seed) for shape in shapes for seed in SEEDS.get(shape, (80, 81))]


def test_every_seed_populates_every_class_of_entry(ndlqr, oracle):
    """after each of the first three iterations of the restatement: bounded entries on lo, on hi and strictly inside
    (those with lo < hi), unbounded addressable entries, and the lo == hi entry at its value; and the entry that carries
    r_prim is not the same at all three iterations for at least half of the shapes"""
    solve = oracle_solve(oracle)
    moved = {}
    for (n, m, N), seed in _all_cases():
        prob = synth(ndlqr, n, m, N, seed)
        b = mixed_bounds(oracle, prob)
        M = full_bounds(n, m, N, *b)[2]
        tr = forward_trace(prob, solve, b, 3)
        for s in tr.its:
            cl = classes(prob, b, s["v"])
            assert min(cl) > 0 and cl[4] == 1, ((n, m, N), seed, s["it"], cl)
        # the codes of the box adjoint after three iterations: all four occur
        codes = active_codes(prob, packed(prob, tr), *b)
        assert set(np.unique(codes)) == {0, 1, 2, 3}, ((n, m, N), seed)
        if seed == 80:
            moved[(n, m, N)] = len({tr.argmax_r_prim(M, it) for it in (1, 2, 3)}) > 1
    print("arg-max of r_prim moves:", moved)
    assert 2 * sum(moved.values()) >= len(moved), moved


# iterations of (seed 80, seed 81) at eps 1e-4 on the restatement, with the lo == hi entry and without it (the counts
# the pattern was first tried with, before the pinned entry joined it: they pin the rest of the pattern)
TERMINATION_ITERS = {(12, 4, 16): ((273, 18), (193, 18)),
                     (7, 9, 16): ((61, 60), (61, 60)),
                     (5, 2, 32): ((83, 89), (83, 89)),
                     (1, 1, 8): ((256, 110), (266, 113))}


def test_every_termination_seed_converges_before_max_iter(ndlqr, oracle):
    assert set(TERMINATION_SHAPES) == set(TERMINATION_ITERS)
    solve = oracle_solve(oracle)
    for (n, m, N), (with_pin, without) in TERMINATION_ITERS.items():
        for p, seed in enumerate((80, 81)):
            prob = synth(ndlqr, n, m, N, seed)
            for pin, want in ((True, with_pin[p]), (False, without[p])):
                tr = forward_trace(prob, solve, mixed_bounds(oracle, prob, pin=pin), TERMINATION["max_iter"], eps=TERMINATION["eps"])
                assert tr.status == 1 and 1 < tr.iters < TERMINATION["max_iter"], ((n, m, N), seed, pin, tr.iters)
                assert tr.iters == want, ((n, m, N), seed, pin, tr.iters)
        assert with_pin[0] != with_pin[1]  # (the two problems of a pair stop at iteration counts of their own)


def test_the_adaptive_case_changes_a_penalty(ndlqr, oracle):
    """the (12,4,16) case with adapt_every = 2 and three iterations: the first problem keeps its penalty at iteration 2,
    the other two halve it, so both exits of box_update's decision run in one launch, the second pass rescales y, and
    iteration 3 reads what it wrote"""
    n, m, N = 12, 4, 16
    solve = oracle_solve(oracle)
    moved = []
    for seed in ADAPT_SEEDS:
        prob = synth(ndlqr, n, m, N, seed)
        its = []
        ref = admm_adaptive_reference(prob, solve, *mixed_bounds(oracle, prob), RHO, ALPHA, 1e-300, 1e-300, 3, 2, trace=its)
        assert [s["rho"] for s in its] == [RHO, RHO, ref[7]] and ref[8] == (ref[7] != RHO), (seed, ref[7:])
        moved.append(ref[7] != RHO)
    assert moved == [False, True, True]


# ------------------------------------------------------------------------------------------------ 4. the launch table

# shape -> (padded (n, m), N * w, passes of the 256-thread entry loop of box_update / box_adjoint_update, passes of the
# 64-thread per-knot row loop of box_start / box_finish): what each shape of test_gpu_box_update.py was chosen for. A
# change of the padding rules or of the instance list (csrc/small_instances.def) that moves a case shows here first.
LAUNCHES = {(6, 3, 4): ((6, 3), 36, 1, 1),         # idle threads
            (1, 1, 8): ((6, 3), 72, 1, 1),         # most entries are pad entries that must never count
            (12, 4, 16): ((12, 4), 256, 1, 1),     # one exact pass
            (5, 2, 32): ((5, 2), 224, 1, 1),       # an instance of its own, not padded: one pass, 32 idle threads
            (5, 3, 32): ((6, 3), 288, 2, 1),       # a padded instance with a short tail (32 entries in the second pass)
            (7, 9, 16): ((8, 16), 384, 2, 1),      # pad columns in the middle of a knot
            (20, 6, 16): ((20, 6), 416, 2, 1),     # runtime-sized strict path
            (12, 4, 256): ((12, 4), 4096, 16, 1),  # many passes
            (130, 5, 4): ((144, 8), 608, 3, 5),    # per-knot loops of five passes, padding beyond 128 states
            (12, 4, 64): ((12, 4), 1024, 4, 1)}    # compact records in fast mode


def test_launch_table_of_the_update_cases():
    assert set(SHAPES) | set(COUNT_SHAPES) | set(WARM_SHAPES) | set(ADJOINT_SHAPES) | set(TERMINATION_SHAPES) <= set(LAUNCHES)
    for shape, want in LAUNCHES.items():
        assert update_launch(*shape) == want, (shape, update_launch(*shape))
    # the planted positions reach both sides of the first pass boundary and the last pass wherever there is one
    for shape in COUNT_SHAPES:
        n, m, N = shape
        offs = sorted(padded_offset(n, m, N, k, j) for k, j in planted_positions(n, m, N))
        passes = LAUNCHES[shape][2]
        assert len(offs) >= (6 if shape == (1, 1, 8) else 12) and offs[0] < 256  # ((1, 1, 8): one column per block)
        if passes > 1:
            assert any(o < 256 for o in offs) and any(o >= 256 for o in offs) and any(o >= 256 * (passes - 1) for o in offs)
            assert min(abs(o - 255) for o in offs) <= LAUNCHES[shape][0][0] + LAUNCHES[shape][0][1], (shape, offs)
        for k, j in planted_positions(n, m, N):
            assert addressable(n, m, N)[k, j]


# ------------------------------------------------------------------------------------------------ 5. the planted cases

@pytest.mark.parametrize("n,m,N", COUNT_SHAPES)
def test_planted_case_premises(ndlqr, oracle, n, m, N):
    """on the oracle's z of the shifted problem: every loose entry has |z| < |c| < B for every planted c = z_e + D, D is a
    power of two >= 16 max |z|, and the problem is small enough for the derivation of the 1e-7 bound (nvars <= 5000)"""
    for seed in (80, 81, 82):
        prob = synth(ndlqr, n, m, N, seed)
        assert prob.nvars <= 5000
        z, D, B = planted(oracle, prob)
        assert np.log2(D) == int(np.log2(D)) and D >= 16 * np.abs(z).max() and B == 4 * D
        A = addressable(n, m, N)
        c = np.abs(z[A] + D)
        assert (c > np.abs(z).max()).all() and (c < B).all() and (c >= 15 * np.abs(z).max()).all()
        lo = loose_bounds(prob, B)
        assert all(np.isfinite(a).all() for a in lo)
        # 1e-9 relative l2 error of a fast solve is below 5e-9 D at the planted entry
        assert 1e-9 * np.linalg.norm(z) <= 5e-9 * D
    assert PLANT_RHO == 0.25
