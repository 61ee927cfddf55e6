"""The eight-knot back-substitution (rb_backsub) in every size-specialised instance and every way it is launched.

Instances with nstates + ninputs <= 16 have two bodies: the LDS-staged one (NDLQR_BACKSUB_COLS=0)
and the one that keeps [A | B] in registers (NDLQR_BACKSUB_COLS=1: one 16-lane row per knot, block 128); with the
variable unset an instance runs the one that measured faster for it (launch_small.hpp). The other instances have the
staged body alone and ignore the variable. Both serve the plain solve, the re-solve on kept records, the solves
with several right-hand sides and the steps that compute a knot range alone. Every instance of small_instances.def at
N = 8, 16, 256 in those four modes under both settings, each against the oracle at the suite's tolerance (relative l2
error <= 1e-9, test_gpu_parity.py). NDLQR_TREE=0 selects the level-per-launch schedule -- the one that ends in
rb_backsub -- at the small batch used here, and every case asserts that it ran: at N >= 16 the instances with
matrix-core products (all but (4,2), (5,2), (4,1), (2,1)) must report `reduced` / `reduced-fused2`, with kept records
`reduced-compact-records`. The enumerated others (N = 8 and those four instances) take whatever the library runs for
them and meet the same bound; several right-hand sides need the compact records, so there -- and only there -- the call
has to be refused, as documented in include/ndlqr.h.

Plus the weak-input-cost family of test_harder_families_* (R scaled by 1e-4: the reciprocals of [Q | R] and of the
diagonal of L are Newton-refined hardware estimates in the register body) at (12,4,256) and (8,4,256), same bounds as
there, under both settings.
"""
import os
import re

import numpy as np
import pytest

from support import Problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
BATCH = 3

_DEF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rslqr_amd", "csrc", "small_instances.def")
INSTANCES = [(int(a), int(b)) for a, b in re.findall(r"^NDLQR_SMALL_INSTANCE\((\d+),\s*(\d+)\)", open(_DEF).read(), flags=re.M)]
HORIZONS = [8, 16, 256]
KEYS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


@pytest.fixture(params=["staged", "cols"], autouse=True)
def body(request, monkeypatch):
    monkeypatch.setenv("NDLQR_BACKSUB_COLS", "1" if request.param == "cols" else "0")
    return request.param


NO_MATRIX_CORES = [(4, 2), (5, 2), (4, 1), (2, 1)]  # knot-lean schedule: rb_backsub never runs


def _reaches_rb_backsub(n, m, N):
    return N >= 16 and (n, m) not in NO_MATRIX_CORES


def _check_schedule(bs, n, m, N, records):
    """The level-per-launch schedule that ends in rb_backsub, wherever the shape and horizon have it."""
    if _reaches_rb_backsub(n, m, N):
        want = "reduced-compact-records" if records else ("reduced-fused2" if (n, m) == (12, 4) else "reduced")
        assert bs.schedule() == want, bs.schedule()


def _problem(n, m, N, g, **over):
    f = dict(g); f.update(over)
    return Problem(n, m, N, *[f[k] for k in KEYS])


def _rel(oracle, prob, sol):
    ref = oracle.solve(prob, 1)[0][: prob.nvars]
    return np.linalg.norm(sol - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("n,m", INSTANCES)
def test_plain_solve(ndlqr, oracle, monkeypatch, n, m, N):
    monkeypatch.setenv("NDLQR_TREE", "0")
    gens = [ndlqr.generate_synthetic(n, m, N, 8100 + p) for p in range(BATCH)]
    bs = ndlqr.BatchSolver(n, m, N, BATCH)
    bs.initialize_flat(*[np.stack([g[k] for g in gens]) for k in KEYS])
    assert bs.solve() == 0
    _check_schedule(bs, n, m, N, False)
    sol = bs.solutions()
    for p, g in enumerate(gens):
        rel = _rel(oracle, _problem(n, m, N, g), sol[p])
        print("plain", (n, m, N), bs.schedule(), p, rel)
        assert rel <= REL_TOL, (p, rel)
    bs.close()


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("n,m", INSTANCES)
def test_resolve_on_kept_records(ndlqr, oracle, monkeypatch, n, m, N):
    monkeypatch.setenv("NDLQR_TREE", "0")
    gens = [ndlqr.generate_synthetic(n, m, N, 8200 + p) for p in range(BATCH)]
    other = [ndlqr.generate_synthetic(n, m, N, 8250 + p) for p in range(BATCH)]
    bs = ndlqr.BatchSolver(n, m, N, BATCH, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*[np.stack([g[k] for g in gens]) for k in KEYS])
    assert bs.solve() == 0
    _check_schedule(bs, n, m, N, True)
    bs.set_rhs_flat(*[np.stack([o[k] for o in other]) for k in ("q", "r", "d", "x0")])
    assert bs.solve_rhs_only() == 0
    sol = bs.solutions()
    for p, (g, o) in enumerate(zip(gens, other)):
        rel = _rel(oracle, _problem(n, m, N, g, q=o["q"], r=o["r"], d=o["d"], x0=o["x0"]), sol[p])
        print("re-solve", (n, m, N), bs.schedule(), p, rel)
        assert rel <= REL_TOL, (p, rel)
    bs.close()


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("n,m", INSTANCES)
def test_three_right_hand_sides(ndlqr, oracle, monkeypatch, n, m, N):
    monkeypatch.setenv("NDLQR_TREE", "0")
    nrhs = 3
    gens = [ndlqr.generate_synthetic(n, m, N, 8300 + p) for p in range(BATCH)]
    bs = ndlqr.BatchSolver(n, m, N, BATCH, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*[np.stack([g[k] for g in gens]) for k in KEYS])
    assert bs.solve() == 0
    _check_schedule(bs, n, m, N, True)
    rng = np.random.default_rng(17)
    q = rng.standard_normal((nrhs, BATCH, N, n))
    r = rng.standard_normal((nrhs, BATCH, N, m))
    d = 0.1 * rng.standard_normal((nrhs, BATCH, N, n))
    x0 = rng.standard_normal((nrhs, BATCH, n))
    if not _reaches_rb_backsub(n, m, N):
        assert bs.schedule() != "reduced-compact-records", bs.schedule()
        with pytest.raises(RuntimeError):  # (no compact records at this shape and horizon: refused, never wrong)
            bs.solve_multi_rhs(q, r, d, x0)
        bs.close()
        return
    sol = bs.solve_multi_rhs(q, r, d, x0)
    for j in range(nrhs):
        for p, g in enumerate(gens):
            rel = _rel(oracle, _problem(n, m, N, g, q=q[j, p], r=r[j, p], d=d[j, p], x0=x0[j, p]), sol[j, p])
            print("multi-rhs", (n, m, N), j, p, rel)
            assert rel <= REL_TOL, (j, p, rel)
    bs.close()


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("n,m", INSTANCES)
def test_first_and_last_eight_knots_alone(ndlqr, oracle, monkeypatch, n, m, N):
    monkeypatch.setenv("NDLQR_TREE", "0")
    bs = ndlqr.BatchSolver(n, m, N, BATCH)
    bs.initialize_synthetic(8400)
    gens = [ndlqr.generate_synthetic(n, m, N, 8400 + p) for p in range(BATCH)]
    x0 = np.stack([g["x0"] for g in gens])
    zb = 2 * n + m
    for k0 in sorted(set([0, N - 8])):
        bs.set_step_selection(k0, 8, 7 | ndlqr.SOLN_ONLY)
        x = ndlqr.pinned_empty(x0.shape); x[...] = -0.5 * x0
        out = ndlqr.pinned_empty((BATCH, 8, zb))
        assert bs.step_async(None, None, None, x, out) == 0 and bs.synchronize() == 0
        _check_schedule(bs, n, m, N, False)
        for p, g in enumerate(gens):
            prob = _problem(n, m, N, g, x0=x[p])
            ref = np.zeros(N * zb); ref[: prob.nvars] = oracle.solve(prob, 1)[0][: prob.nvars]
            err = np.linalg.norm(out[p] - ref.reshape(N, zb)[k0:k0 + 8]) / np.linalg.norm(ref)
            print("knots alone", (n, m, N), bs.schedule(), k0, p, err)
            assert err <= REL_TOL, (k0, p, err)
    bs.close()


@pytest.mark.parametrize("n,m,N,batch,want", [(12, 4, 256, 40, "reduced-fused2"), (8, 4, 256, 40, "reduced")])
def test_weak_input_costs(ndlqr, oracle, n, m, N, batch, want):
    """R scaled by 1e-4 (HARD_FAMILIES of test_gpu_parity.py), full solve and re-solve on kept records: <= 1e-9 relative
    against the oracle and a KKT residual within ten times the oracle's own."""
    gens = []
    for p in range(batch):
        g = ndlqr.generate_synthetic(n, m, N, 11 + p)
        g["R"] = g["R"] * 1e-4
        gens.append(g)
    flat = [np.stack([g[k] for g in gens]) for k in KEYS]
    sample = sorted(set([0, batch // 2, batch - 1]))
    for flags, schedule in ((0, want), (ndlqr.FLAG_KEEP_RECORDS, "reduced-compact-records")):
        bs = ndlqr.BatchSolver(n, m, N, batch, flags=flags)
        bs.initialize_flat(*flat)
        assert bs.solve() == 0
        assert bs.schedule() == schedule, bs.schedule()
        if flags:
            assert bs.solve_rhs_only() == 0
        sol = bs.solutions()
        kres, kbn = bs.kkt_residuals()
        worst_o = 0.0
        for p in sample:
            prob = _problem(n, m, N, gens[p])
            ref = oracle.solve(prob, 8)[0][: prob.nvars]
            ores, obn = oracle.kkt_residual(prob, ref)
            worst_o = max(worst_o, ores / max(1.0, obn))
            rel = np.linalg.norm(sol[p] - ref) / np.linalg.norm(ref)
            res, bn = oracle.kkt_residual(prob, sol[p])
            print("weak R", (n, m, N), bs.schedule(), p, rel, res / max(1.0, bn), ores / max(1.0, obn))
            assert rel <= REL_TOL, (p, rel)
            assert res / max(1.0, bn) <= 10.0 * ores / max(1.0, obn) + 1e-12, (p, res, bn, ores, obn)
        assert float((kres / np.maximum(1.0, kbn)).max()) <= 10.0 * worst_o + 1e-11
        bs.close()
