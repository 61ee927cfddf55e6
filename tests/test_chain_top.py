"""The top tree levels of the separator-only schedule as one block-tridiagonal chain per problem (reduced_chain_top,
rslqr_amd/csrc/kernels_chain_top.hpp; NDLQR_TOP_CHAIN): the separators of level >= max(3, K - 5)
eliminated by block Cholesky along the chain, four problems per wavefront, eaten from both ends by the two wavefronts of
a workgroup. The chain reorders the arithmetic of the tree, so its solutions are held to the project's bars (REL_TOL
against the oracle, the KKT bar of test_resolve_on_compact_records on the hard families) and to the knob off within
REL_TOL -- not to bit-equality; what IS bit-equal is a member next to a failed one, and every repetition of a solve.
All cases run the level-per-launch schedules (NDLQR_TREE=0) with the chain requested (NDLQR_TOP_CHAIN=1)."""
import functools

import numpy as np
import pytest

from failure_support import NOT_SPD, count_bound
from horizon_support import pad_problem
from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9  # the bar of test_batch_fast_within_tolerance
HARD_FAMILIES = [(1.15, 1.0, 1.0), (1.0, 1e-4, 1.0), (1.3, 1e-3, 1.0), (1.0, 1.0, 1e-4)]  # those of tests/test_gpu_parity.py
KEYS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def problem(ndlqr, n, m, N, seed, a_scale=1.0, q_scale=1.0, r_scale=1.0):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    g["A"] = g["A"] * a_scale
    g["Q"] = g["Q"] * q_scale
    g["R"] = g["R"] * r_scale
    return g


def as_problem(n, m, N, g):
    return Problem(n, m, N, *[g[k] for k in KEYS])


def stack(gs):
    return [np.stack([g[k] for g in gs]) for k in KEYS]


def rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def solver(ndlqr, monkeypatch, n, m, N, batch, chain=True, **kw):
    monkeypatch.setenv("NDLQR_TREE", "0")
    monkeypatch.setenv("NDLQR_TOP_CHAIN", "1" if chain else "0")
    return ndlqr.BatchSolver(n, m, N, batch, **kw)


def fused(n, m):
    """(12,4) and what is padded into it run level 2 inside the bottom launch"""
    return (n, m) in ((12, 4), (11, 3))


def check_against_oracle(ndlqr, oracle, monkeypatch, n, m, N, batch, members, family=(1.0, 1.0, 1.0)):
    gs = [problem(ndlqr, n, m, N, 4100 + p, *family) for p in range(batch)]
    bs = solver(ndlqr, monkeypatch, n, m, N, batch)
    bs.initialize_flat(*stack(gs))
    assert bs.solve() == 0
    assert ndlqr.top_chain(bs) is True
    assert bs.schedule() == ("reduced-fused2" if fused(n, m) else "reduced"), bs.schedule()
    sol = bs.solutions()
    assert np.isfinite(sol).all()
    res, bn = bs.kkt_residuals()
    worst = 0.0
    for p in members:
        prob = as_problem(n, m, N, gs[p])
        padded = pad_problem(prob)  # (the oracle takes powers of two: tests/horizon_support.py; prob itself when N is one)
        full = oracle.solve(padded, 8 if family != (1.0, 1.0, 1.0) else 1)[0][: padded.nvars]
        ref = full[: prob.nvars]
        err = float(rel(sol[p], ref))
        worst = max(worst, err)
        print("(%d,%d,%d) x %d member %d: error against the oracle %.3e" % (n, m, N, batch, p, err))
        assert err <= REL_TOL, (p, err)
        ores, obn = oracle.kkt_residual(padded, full)
        print("   device KKT residual %.3e, the oracle's own %.3e" % (res[p] / max(1.0, bn[p]), ores / max(1.0, obn)))
        assert res[p] / max(1.0, bn[p]) <= 10.0 * ores / max(1.0, obn) + 1e-11
    bs.close()
    return worst


@pytest.mark.parametrize("N,batch", [(16, 5), (32, 3), (64, 40), (256, 5), (512, 3), (1024, 1), (13, 5), (100, 3)])
def test_chain_lengths(ndlqr, oracle, monkeypatch, N, batch):
    """(12,4): one block (N = 16: the middle block alone, nothing for the second wavefront), 3, 7 and 31 blocks, level
    launches below a 31-block chain with the sweep over their records behind it (N = 512, 1024), padded horizons; batches
    that are no multiple of four (clamped rows)."""
    check_against_oracle(ndlqr, oracle, monkeypatch, 12, 4, N, batch, sorted({0, batch // 2, batch - 1}))


@pytest.mark.parametrize("n,m", [(6, 3), (8, 4), (9, 3), (10, 4), (13, 4), (15, 2), (11, 3), (7, 9)])
def test_instances(ndlqr, oracle, monkeypatch, n, m):
    """rb_bottom below the chain (6,3), (8,4); the unfused schedule, whose level-2 launch stays (9,3), (10,4); [A | B]
    wider than a DPP row (13,4), (15,2) -- the latter with the rhs column of the panel in the last lane of a row --; the
    padded (11,3) and (7,9)."""
    check_against_oracle(ndlqr, oracle, monkeypatch, n, m, 64, 6, (0, 3, 5))


@pytest.mark.parametrize("family", HARD_FAMILIES)
@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 256, 5), (12, 4, 64, 3), (6, 3, 64, 5)])
def test_hard_families(ndlqr, oracle, monkeypatch, n, m, N, batch, family):
    """hard_problem of tests/test_gpu_parity.py: solutions within REL_TOL of the oracle, device KKT residual at most ten
    times the oracle's own + 1e-11 (the bar of test_resolve_on_compact_records)."""
    check_against_oracle(ndlqr, oracle, monkeypatch, n, m, N, batch, (0, batch - 1), family)


@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 5), (12, 4, 256, 40), (12, 4, 1024, 3), (10, 4, 64, 5), (6, 3, 32, 3)])
def test_knob_on_against_knob_off(ndlqr, monkeypatch, n, m, N, batch):
    """Every member within REL_TOL of the tree's solution; the chain is reported, the schedule name is the same."""
    gs = [problem(ndlqr, n, m, N, 4300 + p) for p in range(batch)]
    out = {}
    for chain in (True, False):
        bs = solver(ndlqr, monkeypatch, n, m, N, batch, chain)
        bs.initialize_flat(*stack(gs))
        assert bs.solve() == 0
        out[chain] = (bs.solutions(), bs.schedule(), ndlqr.top_chain(bs))
        bs.close()
    assert out[True][2] is True and out[False][2] is False
    assert out[True][1] == out[False][1] == ("reduced-fused2" if fused(n, m) else "reduced")
    err = rel(out[True][0], out[False][0])
    print("chain against tree, per member:", err)
    assert (err <= REL_TOL).all(), err


def test_requests_that_keep_the_tree(ndlqr, monkeypatch):
    """KEEP_RECORDS (the chain's scratch lies in the record slots) and an instance whose panel does not fit a DPP row
    keep reduced_top_mc and say so."""
    for n, m, flags in ((12, 4, ndlqr.FLAG_KEEP_RECORDS), (16, 8, 0)):
        bs = solver(ndlqr, monkeypatch, n, m, 64, 5, flags=flags)
        bs.initialize_synthetic(7)
        assert bs.solve() == 0
        assert ndlqr.top_chain(bs) is False, (n, m, flags, bs.schedule())
        bs.close()


@functools.lru_cache(maxsize=None)
def _isolation_inputs(n, m, N, batch):
    import rslqr_amd
    return tuple(problem(rslqr_amd, n, m, N, 4500 + p) for p in range(batch))


@pytest.mark.parametrize("tile", ["left of the middle", "right of the middle", "first"])
def test_member_isolation(ndlqr, monkeypatch, tile):
    """Batch 8, N = 64 (seven blocks, the middle one separator 31): a NaN in A_k of member 5 for every k of an eight-knot
    tile. The other seven members are bit-equal to a clean run, the solve returns NDLQR_ERR_NOT_SPD, and member 5's
    word grows by at least count_bound of every k."""
    n, m, N, batch, bad = 12, 4, 64, 8, 5
    knots = {"left of the middle": range(24, 32), "right of the middle": range(32, 40), "first": range(0, 8)}[tile]
    gs = _isolation_inputs(n, m, N, batch)
    bs = solver(ndlqr, monkeypatch, n, m, N, batch)
    bs.initialize_flat(*stack(gs))
    assert bs.solve() == 0 and ndlqr.top_chain(bs) is True
    clean = bs.solutions()
    schedule = bs.schedule()
    for k in knots:
        poisoned = [{f: v.copy() for f, v in g.items()} for g in gs]
        poisoned[bad]["A"][k][n - 1] = np.nan
        before = bs.cholesky_failure_counts().astype(np.int64)
        bs.initialize_flat(*stack(poisoned))
        rc = bs.solve()
        grow = bs.cholesky_failure_counts().astype(np.int64) - before
        sol = bs.solutions()
        assert rc == NOT_SPD, (k, rc)
        assert bs.cholesky_failures() == int(grow.sum())
        for p in range(batch):
            if p != bad:
                assert grow[p] == 0 and np.array_equal(sol[p], clean[p]), (k, p)
        assert grow[bad] >= count_bound(schedule, k, N), (k, grow[bad], count_bound(schedule, k, N))
    bs.initialize_flat(*stack(gs))
    assert bs.solve() == 0 and np.array_equal(bs.solutions(), clean)
    bs.close()


@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 256, 40), (12, 4, 512, 5), (6, 3, 64, 5)])
def test_solves_in_flight_and_replays(ndlqr, monkeypatch, n, m, N, batch):
    """Two solves in flight on the two buffer sets (each chain keeps its scratch in its set's records) and ten replays of
    the captured launch sequence: every solution is bit-equal to the first."""
    bs = solver(ndlqr, monkeypatch, n, m, N, batch)
    bs.initialize_synthetic(123)
    assert bs.solve() == 0 and ndlqr.top_chain(bs) is True
    first = bs.solutions()
    for rep in range(5):
        assert bs.solve_async() == 0 and bs.solve_async() == 0
        assert bs.synchronize_previous() == 0
        assert np.array_equal(bs.solutions(), first), rep
        assert bs.synchronize() == 0
        assert np.array_equal(bs.solutions(), first), rep
    res, bn = bs.kkt_residuals()
    assert (res <= 1e-9 * np.maximum(1.0, bn)).all()
    bs.close()


def test_step_that_computes_knot_zero_alone(ndlqr, monkeypatch):
    """An MPC step with NDLQR_SOLN_ONLY delivers u of knot 0 equal to that of the resident solution, bit for bit (what
    bench.py reports as equals_resident_solution)."""
    n, m, N, batch = 12, 4, 256, 40
    bs = solver(ndlqr, monkeypatch, n, m, N, batch)
    bs.initialize_synthetic(91)
    assert bs.solve() == 0 and ndlqr.top_chain(bs) is True
    sol = bs.solutions()
    x0 = np.stack([ndlqr.generate_synthetic(n, m, N, 91 + p)["x0"] for p in range(batch)])
    x = ndlqr.pinned_empty(x0.shape)
    x[...] = x0
    u0 = [ndlqr.pinned_empty((batch, 1, m)) for _ in range(2)]
    for blocks in (ndlqr.SOLN_INPUT, ndlqr.SOLN_INPUT | ndlqr.SOLN_ONLY):
        bs.set_step_selection(0, 1, blocks)
        for i in range(4):
            assert bs.step_async(None, None, None, x, u0[i & 1]) == 0
            if i >= 1:
                assert bs.synchronize_previous() == 0
        assert bs.synchronize() == 0
        assert ndlqr.top_chain(bs) is True
        assert np.array_equal(u0[1][:, 0, :], sol[:, 2 * n:2 * n + m])
        assert np.array_equal(u0[0][:, 0, :], sol[:, 2 * n:2 * n + m])
    bs.close()
