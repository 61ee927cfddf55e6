"""Feedback gains and cost-to-go matrices on the device (ndlqr_BatchFeedbackGains, BatchSolver.feedback_gains; DESIGN.md
section 3.22) against gain_support.py. Shapes (6,3), (12,4), (7,9) (m > n, zero-padded inside an instance), (20,5)
(runtime-sized kernels), (32,8), and (64,16) x N = 4 once (the LDS map without the second buffer); horizons 2 (one
dynamics knot), 5 (padded), 8, 16, 33; batch 3; diagonal costs (generate_synthetic) and dense costs (cost_support's
moderate family).

Bars. Per entry of K, k, P, p against the longdouble restatement: max(8 x the float64 restatement's own largest error on
the same problems, 16 eps x the array's largest entry) -- the bar of test_gpu_cost.test_reduction_per_entry; the margin
covers another operation order and FMA contraction. Consistency with the solver and the MPC use: 1e-9 of the field, the
parity contract the solutions themselves are held to. Everything else: bit for bit."""
import numpy as np
import pytest

import cost_support as cs
import gain_support as gs
from test_gpu_cost import flag_modes

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
KINDS = ("diagonal", "dense")
CASES = [(n, m, N) for (n, m) in gs.SHAPES for N in gs.HORIZONS]
FLAT = dict(K=lambda a: a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1), k=lambda a: a,
            P=lambda a: a.transpose(0, 1, 3, 2).reshape(a.shape[0], a.shape[1], -1), p=lambda a: a)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a if k in b)


def check_per_entry(got, ref, label, names=gs.NAMES):
    """test 1's bar for the arrays `names` of `got` (math convention, the whole horizon); returns the ratios to the bar"""
    ratios = {}
    for k in names:
        limit, own = gs.bar(ref["exact"], ref["f64"], k)
        err = float(np.abs(got[k] - ref["exact"][k]).max())
        ratios[k] = err / limit
        print("gains", label, k, "device %.3e numpy %.3e ratio to bar %.3f" % (err, own, ratios[k]))
        assert got[k].shape == ref["exact"][k].shape and np.isfinite(got[k]).all()
        assert err <= limit, (label, k, err, limit)
    return ratios


# ---------------------------------------------------------------------------- 1: per entry against the longdouble reference
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", CASES + [(64, 16, 4)])
def test_per_entry(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    got = bs.feedback_gains()
    bs.close()
    assert not got["failures"].any()
    check_per_entry(got, ref, "%s %s" % ((n, m, N), kind))


@pytest.mark.parametrize("kind", KINDS)
def test_flag_modes_give_the_same_bits(ndlqr, kind):
    ref = gs.reference(12, 4, 8, kind)
    outs = []
    for flags in flag_modes(ndlqr):
        bs = gs.solver(ndlqr, ref, kind, flags)
        outs.append(bs.feedback_gains())
        bs.close()
    check_per_entry(outs[0], ref, "flag modes " + kind)
    for o in outs[1:]:
        assert same(outs[0], o)


# ---------------------------------------------------------------------------- 2: consistency with the solver
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", CASES)
def test_consistency_with_the_solver(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    assert bs.solve() == 0
    Z = bs.solutions()
    got = bs.feedback_gains()
    bs.close()
    for i in range(gs.BATCH):
        eu, el = gs.closed_loop_errors({k: got[k][i] for k in gs.NAMES}, Z[i], n, m, N)
        print("closed loop", (n, m, N), kind, i, "u %.2e lambda %.2e" % (eu, el))
        assert eu <= REL_TOL and el <= REL_TOL, (i, eu, el)


# ---------------------------------------------------------------------------- 3: the MPC use
@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (6, 3, 8)])
def test_mpc_first_gain_predicts_the_next_input(ndlqr, n, m, N):
    ref = gs.reference(n, m, N, "diagonal")
    bs = gs.solver(ndlqr, ref, "diagonal")
    K0 = bs.feedback_gains(0, 1, want=("K",))["K"][:, 0]
    assert K0.shape == (gs.BATCH, m, n)
    x0 = np.stack([p["x0"] for p in ref["probs"]])
    delta = 0.1 * np.random.default_rng([n, m, N]).standard_normal(x0.shape)
    pin = lambda a: (lambda b: (b.__setitem__(Ellipsis, a), b)[1])(ndlqr.pinned_empty(a.shape))
    ins = [pin(x0), pin(x0 + delta)]
    outs = [ndlqr.pinned_empty((gs.BATCH, bs.nvars)) for _ in range(2)]
    for a, o in zip(ins, outs):
        assert bs.step_async(None, None, None, a, o) == 0
    assert bs.synchronize() == 0
    bs.close()
    u = [o[:, 2 * n:2 * n + m] for o in outs]
    for i in range(gs.BATCH):
        du = u[1][i] - u[0][i]
        err = float(np.abs(du - K0[i] @ delta[i]).max()) / float(np.abs(du).max())
        print("mpc", (n, m, N), i, "%.2e" % err)
        assert err <= REL_TOL, (i, err)


# ---------------------------------------------------------------------------- 4: ranges, memories, determinism
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8), (7, 9, 16), (20, 5, 33), (32, 8, 5)])
def test_ranges_memories_determinism(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    full = bs.feedback_gains()
    assert same(full, bs.feedback_gains())  # two calls: the same bits
    assert np.array_equal(full["P"], full["P"].transpose(0, 1, 3, 2))
    # knot N-1: K, k exact zeros; P, p the last knot's cost
    assert not full["K"][:, N - 1].any() and not full["k"][:, N - 1].any()
    QN = np.stack([p["Q"][N - 1] for p in ref["probs"]])
    qN = np.stack([p["q"][N - 1] for p in ref["probs"]])
    if kind == "diagonal":
        assert np.array_equal(full["P"][:, N - 1], QN) and np.array_equal(full["p"][:, N - 1], qN)
    else:  # (Q as L L' of its factor, q as L (L^-1 q): test 1's bar holds them)
        assert np.abs(full["P"][:, N - 1] - QN).max() <= gs.bar(ref["exact"], ref["f64"], "P")[0]
        assert np.abs(full["p"][:, N - 1] - qN).max() <= gs.bar(ref["exact"], ref["f64"], "p")[0]
    # any range is that slice of the whole read-out
    for k0, nk in {(0, 1), (N - 1, 1), ((N - 1) // 2, min(2, N - (N - 1) // 2)), (0, N)}:
        part = bs.feedback_gains(k0, nk)
        for k in gs.NAMES:
            assert np.array_equal(part[k], full[k][:, k0:k0 + nk]), (k0, nk, k)
    # an omitted output changes no other
    for want in (("K",), ("k", "p"), ("P",), ("K", "k", "P")):
        part = bs.feedback_gains(want=want)
        assert set(part) == set(want) | {"failures"} and same(part, full)
    # pinned and device outputs, flat column-major shapes
    flat = {k: np.ascontiguousarray(FLAT[k](full[k])) for k in gs.NAMES}
    pinned = {k: ndlqr.pinned_empty(flat[k].shape) for k in gs.NAMES}
    assert bs.feedback_gains(out=pinned)["K"] is pinned["K"]
    dev = {k: ndlqr.DeviceArray(flat[k].shape) for k in gs.NAMES}
    bs.feedback_gains(out=dev)
    for k in gs.NAMES:
        assert np.array_equal(pinned[k], flat[k]) and np.array_equal(dev[k].get(), flat[k]), k
    mixed = dict(K=ndlqr.DeviceArray(flat["K"][:, 1:].shape), p=ndlqr.pinned_empty(flat["p"][:, 1:].shape))
    bs.feedback_gains(1, N - 1, out=mixed)
    assert np.array_equal(mixed["K"].get(), flat["K"][:, 1:]) and np.array_equal(mixed["p"], flat["p"][:, 1:])
    bs.close()
    # a problem's outputs do not depend on its place in the batch
    perm = [2, 0, 1]
    bs = gs.solver(ndlqr, ref, kind, probs=[ref["probs"][i] for i in perm])
    moved = bs.feedback_gains()
    bs.close()
    for k in gs.NAMES:
        assert np.array_equal(moved[k], full[k][perm]), k


# ---------------------------------------------------------------------------- 5: nothing else moves
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", [(12, 4, 8), (7, 9, 5), (20, 5, 16)])
def test_nothing_else_moves(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind, ndlqr.FLAG_KEEP_RECORDS)
    assert bs.solve() == 0
    Z = bs.solutions()
    assert bs.solve_rhs_only() == 0
    Z2 = bs.solutions()
    counts = bs.cholesky_failure_counts()
    assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z)
    gains = bs.feedback_gains()
    assert np.array_equal(bs.solutions(), Z)
    assert bs.solve_rhs_only() == 0 and np.array_equal(bs.solutions(), Z2)
    assert np.array_equal(bs.cholesky_failure_counts(), counts)
    if kind == "diagonal":  # the box solve shifts QR and restores it
        bs.set_bounds(ulo=-0.5 * np.ones(m), uhi=0.5 * np.ones(m))
        bs.solve_box(max_iter=20)
        assert same(gains, bs.feedback_gains())
    bs.close()


# ---------------------------------------------------------------------------- 6: the latest right-hand side
def new_rhs(ref, seed):
    rng = np.random.default_rng(seed)
    probs = [dict(p, q=p["q"] + rng.standard_normal(p["q"].shape), r=p["r"] + rng.standard_normal(p["r"].shape),
                  d=p["d"] + 0.3 * rng.standard_normal(p["d"].shape), x0=p["x0"] + 1.0) for p in ref["probs"]]
    exact = gs.stack([gs.gains(p, np.longdouble) for p in probs])
    f64 = gs.stack([(gs.gains(p) if np.count_nonzero(p["H"]) == 0 else gs.gains_reduced(p)) for p in probs])
    return probs, dict(exact=exact, f64=f64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (6, 3, 8), (7, 9, 5)])
def test_set_rhs_moves_k_and_p_alone(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    old = bs.feedback_gains()
    probs, ref2 = new_rhs(ref, [n, m, N, 6])
    bs.set_rhs_flat(*cs.flat(probs, ("q", "r", "d", "x0")))
    got = bs.feedback_gains()
    bs.close()
    assert np.array_equal(got["K"], old["K"]) and np.array_equal(got["P"], old["P"])
    check_per_entry(got, ref2, "new rhs %s %s" % ((n, m, N), kind), ("k", "p"))


@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (6, 3, 8)])
def test_steps_leave_the_latest_rhs_on_either_buffer_set(ndlqr, n, m, N):
    ref = gs.reference(n, m, N, "diagonal")
    bs = gs.solver(ndlqr, ref, "diagonal")
    old = bs.feedback_gains()
    pin = lambda a: (lambda b: (b.__setitem__(Ellipsis, a), b)[1])(ndlqr.pinned_empty(a.shape))
    outs = [ndlqr.pinned_empty((gs.BATCH, bs.nvars)) for _ in range(6)]
    names = ("q", "r", "d", "x0")
    step, probs, ref2 = 0, None, None
    for s in range(3):  # full steps on the sets A, B, A, each with its own right-hand side
        probs, ref2 = new_rhs(ref, [n, m, N, 60 + s])
        parts = [pin(a) for a in cs.flat(probs, names)]
        assert bs.step_async(*parts, outs[step]) == 0
        step += 1
    for count in (1, 2):  # x0-only steps: the current set is B, then A; q, r, d are those of the last full step
        for s in range(count):
            probs = [dict(p, x0=p["x0"] + 0.5) for p in probs]
            assert bs.step_async(None, None, None, pin(cs.flat(probs, ("x0",))[0]), outs[step]) == 0
            step += 1
        assert bs.synchronize() == 0
        got = bs.feedback_gains()
        assert np.array_equal(got["K"], old["K"]) and np.array_equal(got["P"], old["P"])
        # (x0 enters no gain: k, p are those of the last full step's q, r, d)
        check_per_entry(got, ref2, "steps %s x0-only %d" % ((n, m, N), count), ("k", "p"))
    bs.close()


# ---------------------------------------------------------------------------- 7: padded horizon, last knot never loaded
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", [(12, 4, 5), (7, 9, 8), (20, 5, 5), (6, 3, 8)])
def test_last_knot_is_never_loaded(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    clean = bs.feedback_gains()
    bs.close()
    bad = []
    for p in ref["probs"]:
        p = {k: v.copy() for k, v in p.items()}
        for k in ("A", "B", "R", "r", "d") + (("H",) if kind == "dense" else ()):
            p[k][N - 1] = np.nan
        bad.append(p)
    if kind == "diagonal":  # (np.diag of a NaN matrix: the diagonal is NaN, which is what initialize_flat gets)
        assert all(np.isnan(np.diag(p["R"][N - 1])).all() for p in bad)
    bs = gs.solver(ndlqr, ref, kind, probs=bad)
    got = bs.feedback_gains()
    bs.close()
    for k in gs.NAMES:
        assert np.isfinite(got[k]).all() and np.array_equal(got[k], clean[k]), k
    assert not got["failures"].any()


# ---------------------------------------------------------------------------- 8: failure reporting
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,N", [(12, 4, 8), (7, 9, 5), (32, 8, 16)])
def test_failure_reporting(ndlqr, n, m, N, kind):
    ref = gs.reference(n, m, N, kind)
    bs = gs.solver(ndlqr, ref, kind)
    healthy = bs.feedback_gains()
    bs.close()
    probs = [{k: v.copy() for k, v in p.items()} for p in ref["probs"]]
    probs[1]["R"][(N - 1) // 2] = -1e6 * np.eye(m)
    bs = gs.solver(ndlqr, ref, kind, probs=probs)
    before = bs.cholesky_failure_counts()
    flat = {k: np.zeros(s) for k, s in dict(K=(gs.BATCH, N, m * n), k=(gs.BATCH, N, m), P=(gs.BATCH, N, n * n),
                                            p=(gs.BATCH, N, n)).items()}
    fails = np.zeros(gs.BATCH, dtype=np.int32)
    import ctypes as C
    err = bs.L.ndlqr_BatchFeedbackGains(bs.h, 0, N, *[flat[k].ctypes.data_as(C.POINTER(C.c_double)) for k in gs.NAMES],
                                        fails.ctypes.data_as(C.POINTER(C.c_int)))
    got = bs.feedback_gains()  # (documented: no exception, the dict with failures set)
    assert np.array_equal(got["failures"], fails)
    assert fails[0] == 0 and fails[2] == 0, fails
    if kind == "diagonal":
        assert err == ndlqr.api.ERR_NOT_SPD and fails[1] > 0, (err, fails)
    else:  # cost_factor took the pivots of R as 1 and counted them at the initialiser: only what this call adds is asserted
        assert before[1] > 0 and err == (ndlqr.api.ERR_NOT_SPD if fails[1] else 0), (err, before, fails)
    assert np.array_equal(bs.cholesky_failure_counts(), before)
    # Finite input gives finite output. In dense-cost mode the sweep's input is the resident reduced problem: where
    # cost_factor's pivot rule on the indefinite Q - H R^-1 H' has already overflowed (it does at (32,8)), problem 1 has no
    # finite input and nothing of it is asserted; the other problems' outputs are, always.
    finite_in = kind == "diagonal" or all(np.isfinite(a[1]).all() for a in bs.cost_reduction().values())
    print("failures", (n, m, N), kind, "code", err, "counts", fails, "finite input of the bad problem", finite_in)
    bs.close()
    for k in gs.NAMES:
        assert np.isfinite(got[k][[0, 2]]).all() and (not finite_in or np.isfinite(got[k][1]).all()), k
        assert np.array_equal(FLAT[k](got[k]), flat[k], equal_nan=True), k
        assert np.array_equal(got[k][[0, 2]], healthy[k][[0, 2]]), k


# ---------------------------------------------------------------------------- 9: refusals by name
def refused(bs, call):
    with pytest.raises(RuntimeError) as e:
        call()
    msg = bs.L.ndlqr_hip_last_error().decode()
    assert msg.startswith("ndlqr_hip_feedback_gains:") and msg in str(e.value), msg
    return msg


def test_refusals_by_name(ndlqr):
    n, m, N = 12, 4, 8
    ref = gs.reference(n, m, N, "diagonal")
    bs = gs.solver(ndlqr, ref, "diagonal")
    assert bs.solve() == 0
    Z = bs.solutions()
    for call in (lambda: bs.feedback_gains(N - 1, 2), lambda: bs.feedback_gains(0, N + 1), lambda: bs.feedback_gains(3, 0),
                 lambda: bs.feedback_gains(2, -1), lambda: bs.feedback_gains(-1, 2), lambda: bs.feedback_gains(N, 1)):
        assert "knots" in refused(bs, call)
        assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z)
    assert "no output" in refused(bs, lambda: bs.feedback_gains(want=()))
    assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z)
    with pytest.raises(ValueError):
        bs.feedback_gains(want=("K", "Q"))
    bs.close()


def test_constrained_mode_is_refused_by_name(ndlqr):
    n, m, N = 6, 3, 5
    fam = cs.family(n, m, N, "moderate")
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    p = 2
    rng = np.random.default_rng(9)
    Cx, Du = rng.standard_normal((cs.BATCH, N, p * n)), rng.standard_normal((cs.BATCH, N, p * m))
    bs.initialize_flat_constrained(*cs.flat(fam["probs"]), Cx, Du, -np.ones((cs.BATCH, N, p)), np.ones((cs.BATCH, N, p)))
    assert bs.is_constrained() and bs.solve() == 0
    Z = bs.solutions()
    msg = refused(bs, lambda: bs.feedback_gains())
    assert "constrained" in msg and "rho-shifted" in msg
    assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z)
    # a dense initialiser leaves the mode: the gains are there again
    bs.initialize_flat_dense(*cs.flat(fam["probs"]))
    assert not bs.feedback_gains()["failures"].any()
    bs.close()


def test_block_size_beyond_the_lds_is_refused_by_name(ndlqr):
    limit = 160 * 1024
    assert ndlqr.feedback_gains_lds(64, 16) <= limit < ndlqr.feedback_gains_lds(64, 16, second=True)
    n, m, N = 64, 16, 2
    while ndlqr.feedback_gains_lds(n, m) <= limit:  # the first block size of this aspect whose single-buffer map is too large
        n += 8
    assert ndlqr.feedback_gains_lds(n - 8, m) <= limit
    bs = ndlqr.BatchSolver(n, m, N, 1)
    bs.initialize_synthetic(5)
    assert bs.solve() == 0
    Z = bs.solutions()
    msg = refused(bs, lambda: bs.feedback_gains())
    assert "gain_sweep needs %d bytes" % ndlqr.feedback_gains_lds(n, m) in msg
    assert bs.solve() == 0 and np.array_equal(bs.solutions(), Z)
    bs.close()
