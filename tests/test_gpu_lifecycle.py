"""Allocation, growth and teardown of the device context's buffers in one supported call sequence.

One solver of shape (6,3), N = 16, batch 2 in fast mode with FLAG_KEEP_RECORDS (NDLQR_TREE=0: the level-per-launch schedule,
whose compact records the multiple right-hand sides need) takes every optional feature into use in turn, so that every
first-use buffer is allocated and every growable one grows at least once:

1. solve;
2. solve_adjoint (stages g: batch * nvars = 474 doubles, the first grad_stage) and gradients of q and x0 (108 doubles);
3. set_bounds, solve_box, bound_multipliers (288 doubles), solve_box_adjoint, bound_gradients per problem
   (2 * batch * N * (n + m) = 576 doubles: grad_stage grows);
4. a plain solve, then refine;
5. solve_multi_rhs with 1 right-hand side (buffers for 2 sets), then with 5 (10 sets: every multi-rhs buffer grows);
6. solutions() into a pageable array;
7. close.

Each of the five multi-rhs solutions must equal set_rhs_flat + solve_rhs_only of the same right-hand side bit for bit.
The same sequence runs on a solver of the padded shape (7,3) (pad_stage in use) before anything else -- the fresh state
-- and again after the (6,3) solver has been closed, on whatever memory that one gave back: everything the second run
returns must equal the first bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, BATCH = 16, 2
KEYS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
RHS = ("q", "r", "d", "x0")


def _lifecycle(ndlqr, n, m, seed):
    """Steps 1 to 7 on a new solver; everything the calls returned, as a dict of arrays."""
    gens = [ndlqr.generate_synthetic(n, m, N, seed + p) for p in range(BATCH)]
    rng = np.random.default_rng(seed)
    out = {}
    bs = ndlqr.BatchSolver(n, m, N, BATCH, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*[np.stack([g[k] for g in gens]) for k in KEYS])
    # 1.
    assert bs.solve() == 0
    assert bs.schedule() == "reduced-compact-records", bs.schedule()
    out["z"] = bs.solutions()
    # 2.
    g = rng.standard_normal((BATCH, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    out["w"] = bs.adjoint()
    grads = bs.gradients(out={"q": np.zeros(bs.gradient_shape("q")), "x0": np.zeros(bs.gradient_shape("x0"))})
    out["gq"], out["gx0"] = grads["q"], grads["x0"]
    # 3.
    bs.set_bounds(None, None, -0.1 * np.ones(m), 0.1 * np.ones(m))
    out["box_iters"], out["box_status"] = bs.solve_box(max_iter=50, check_every=10)
    out["box_z"] = bs.solutions()
    out["mu_x"], out["mu_u"] = bs.bound_multipliers()
    out["abox_iters"], out["abox_status"] = bs.solve_box_adjoint(g, max_iter=20, check_every=10)
    for k, v in bs.bound_gradients(summed=False).items():
        out["g" + k] = v
    # 4.
    assert bs.solve() == 0
    out["steps"], out["eta_before"], out["eta_after"] = bs.refine(2)
    out["z_refined"] = bs.solutions()
    # 5.
    nrhs = 5
    q = rng.standard_normal((nrhs, BATCH, N, n))
    r = rng.standard_normal((nrhs, BATCH, N, m))
    d = rng.standard_normal((nrhs, BATCH, N, n))
    x0 = rng.standard_normal((nrhs, BATCH, n))
    out["multi1"] = bs.solve_multi_rhs(q[:1], r[:1], d[:1], x0[:1])
    out["multi5"] = bs.solve_multi_rhs(q, r, d, x0)
    assert np.array_equal(out["multi5"][:1], out["multi1"])
    for j in range(nrhs):
        bs.set_rhs_flat(q[j], r[j], d[j], x0[j])
        assert bs.solve_rhs_only() == 0
        one = bs.solutions()
        assert np.array_equal(out["multi5"][j], one), (j, np.abs(out["multi5"][j] - one).max())
    # 6.
    pageable = np.full((BATCH, bs.nvars), np.nan)
    assert bs.solutions(out=pageable) is pageable
    out["z_last"] = pageable
    assert np.array_equal(pageable, out["multi5"][nrhs - 1])
    # 7.
    bs.close()
    for k, v in out.items():
        if v.dtype.kind == "f":
            assert np.all(np.isfinite(v)), k
    return out


def test_allocate_grow_teardown(ndlqr, monkeypatch):
    monkeypatch.setenv("NDLQR_TREE", "0")
    fresh = _lifecycle(ndlqr, 7, 3, 9300)
    _lifecycle(ndlqr, 6, 3, 9200)
    again = _lifecycle(ndlqr, 7, 3, 9300)
    assert sorted(again) == sorted(fresh)
    for k in fresh:
        assert np.array_equal(again[k], fresh[k]), (k, np.abs(again[k] - fresh[k]).max())
