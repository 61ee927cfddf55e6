"""The asynchronous MPC step and the solution slices of dense-cost mode (ndlqr_BatchStepAsyncDense,
ndlqr_SolveBatchSlicesAsyncDense, ndlqr_CopyBatchSolutionSlicesDense; DESIGN.md section 3.16, "The asynchronous step"),
against cost_support.py's refined solutions of the dense KKT system and against the same library's synchronous path.
Family: moderate (cond(Q'), cond(R) = 1e3), batch 3, cost_support's shapes and horizons: (7,9) is m > n with a padded
block size, N = 5 a padded horizon, N = 2 has only the first and the last knot, (32,8) runs the runtime-sized family,
(12,4,16) keeps compact records (the re-solve branch of a step).

Bars. The device right-hand side a step leaves, and every slice against the same solver's solutions(): bit for bit --
the two kernels of the step (cost_pack_rhs, cost_deliver_slice) share the per-knot bodies of cost_apply_t / cost_apply.
Solutions per field (max-abs difference over max-abs of the field): 1e-9, the bar of test_gpu_cost.py for this family.
K_0 dx0 against the difference of two x0-only steps: 1e-9, the bar of test_gpu_gains.py for that check."""
import ctypes as C
import types

import numpy as np
import pytest

import cost_support as cs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
CASES = [(n, m, N) for (n, m) in cs.SHAPES for N in cs.HORIZONS]
RHS = ("q", "r", "d", "x0")
# what a step of each kind replaces (x0 always; q and r together)
KINDS = dict(F=RHS, QR=("q", "r", "x0"), D=("d", "x0"), X=("x0",))


def dense_solver(ndlqr, probs, flags=0):
    n, m, N = cs.dims(probs[0])
    bs = ndlqr.BatchSolver(n, m, N, len(probs), flags=flags)
    bs.initialize_flat_dense(*cs.flat(probs))
    assert bs.cost_is_dense()
    return bs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def pin(ndlqr, a):
    b = ndlqr.pinned_empty(a.shape)
    b[...] = a
    return b


def base_rhs(probs):
    return {k: a.copy() for k, a in zip(RHS, cs.flat(probs, RHS))}


def draw(rng, like):
    return {k: rng.standard_normal(a.shape) for k, a in like.items()}


def merge(merged, new, kind):
    """the logical right-hand side after a step of `kind` with the arrays `new`"""
    out = dict(merged)
    for k in KINDS[kind]:
        out[k] = new[k]
    return out


def step(ndlqr, bs, new, kind, out, selection=None, poison=False):
    """one dense step of `kind` from pinned copies of `new`; poison: NaN in r, d of the caller's last knot"""
    args = []
    for k in RHS:
        if k not in KINDS[kind]:
            args.append(None)
            continue
        a = new[k].copy()
        if poison and k in ("r", "d"):
            a[:, -1] = np.nan
        args.append(pin(ndlqr, a))
    return bs.step_dense_async(*args, out, selection=selection)


def references(probs, rhs):
    """refined solutions [batch, nvars] of the problems with the right-hand side `rhs`"""
    return np.stack([cs.refined_solve(*cs.dense_kkt(dict(p, **{k: rhs[k][i] for k in RHS}))) for i, p in enumerate(probs)])


def errors(Z, ref, n, m, N):
    return np.max([cs.field_errors(z, zr, n, m, N) for z, zr in zip(Z, ref)], axis=0)


def cut(Z, n, m, N, k0, nk, blocks):
    """the slice [batch, nk, width] of packed solutions Z [batch, nvars] (u of the last knot: +0)"""
    full = np.zeros((Z.shape[0], N * (2 * n + m)))
    full[:, : Z.shape[1]] = Z
    full = full.reshape(Z.shape[0], N, 2 * n + m)[:, k0:k0 + nk]
    cols = ([np.arange(n)] if blocks & 1 else []) + ([n + np.arange(n)] if blocks & 2 else []) + \
           ([2 * n + np.arange(m)] if blocks & 4 else [])
    return np.ascontiguousarray(full[:, :, np.concatenate(cols)])


def ranges(N):
    return [(0, 1), (N - 1, 1), (0, N)] + ([(1, 2)] if N >= 4 else [])


# ---------------------------------------------------------------------------- 1: the right-hand side, entry by entry
# full, (q, r) + x0, d + x0, x0-only -- ordered so that, with consecutive steps alternating between the two buffer sets,
# each set takes every kind
ORDER = ["F", "QR", "D", "X", "F", "F", "QR", "D", "X"]


@pytest.mark.parametrize("n,m,N", CASES)
def test_rhs_per_entry(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    A, B = dense_solver(ndlqr, fam["probs"]), dense_solver(ndlqr, fam["probs"])
    merged = base_rhs(fam["probs"])
    prev = A.rhs_raw()
    assert same_bits(prev, B.rhs_raw())
    rng = np.random.default_rng([n, m, N, 1])
    out = ndlqr.pinned_empty((cs.BATCH, A.nvars))
    for i, kind in enumerate(ORDER):
        new = draw(rng, merged)
        assert step(ndlqr, A, new, kind, out, poison=True) == 0
        assert A.synchronize() == 0
        merged = merge(merged, new, kind)
        B.set_rhs_flat(*[merged[k] for k in RHS])
        ra, rb = A.rhs_raw(), B.rhs_raw()
        assert np.isfinite(ra).all() and np.isfinite(out).all(), (i, kind)
        assert not same_bits(ra, prev), (i, kind)  # (the step wrote something)
        diff = np.flatnonzero(ra.view(np.uint64).reshape(-1) != rb.view(np.uint64).reshape(-1))
        assert diff.size == 0, (i, kind, diff[:8], ra.reshape(-1)[diff[:8]], rb.reshape(-1)[diff[:8]])
        prev = ra
    A.close()
    B.close()


# ---------------------------------------------------------------------------- 2: solutions per field, flags, memories
def out_memory(ndlqr, which, count):
    """(what the step gets, read() -> the `count` doubles and the sentinel behind them) in pinned | pageable | device memory"""
    if which == 2:
        dev = ndlqr.DeviceArray(count + 1).set(np.full(count + 1, 7.0))
        view = types.SimpleNamespace(ptr=dev.ptr, size=count, keep=dev)
        return view, lambda: (dev.get()[:count], dev.get()[count])
    buf = ndlqr.pinned_empty(count + 1) if which == 0 else np.empty(count + 1)
    buf[...] = 7.0
    return buf[:count], lambda: (buf[:count].copy(), buf[count])


def run_steps(ndlqr, n, m, N, modes, resolve=False):
    """Three whole-vector steps (full, x0-only, d + x0) per flag mode of `modes`, the outputs rotating through pinned,
    pageable and device memory; resolve: the second and third must be re-solves on kept records."""
    fam = cs.family(n, m, N, "moderate")
    rng = np.random.default_rng([n, m, N, 2])
    plan, rhs, news = ["F", "X", "D"], [], []
    merged = base_rhs(fam["probs"])
    for kind in plan:
        news.append(draw(rng, merged))
        merged = merge(merged, news[-1], kind)
        rhs.append(merged)
    refs = [references(fam["probs"], r) for r in rhs]
    for f, flags in enumerate(modes):
        A = dense_solver(ndlqr, fam["probs"], flags)
        B = dense_solver(ndlqr, fam["probs"], flags) if flags == ndlqr.FLAG_STRICT_FP else None
        for i, kind in enumerate(plan):
            dest, read = out_memory(ndlqr, (i + f) % 3, cs.BATCH * A.nvars)
            assert step(ndlqr, A, news[i], kind, dest) == 0
            assert A.synchronize() == 0 and A.cholesky_failures() == 0
            got, sentinel = read()
            got = got.reshape(cs.BATCH, A.nvars)
            err = errors(got, refs[i], n, m, N)
            print("dense step", (n, m, N), "flags", flags, kind, "memory", (i + f) % 3, err, A.schedule())
            assert sentinel == 7.0, (flags, kind)
            assert (err <= REL_TOL).all(), (flags, kind, err)
            assert same_bits(A.solutions(), got), (flags, kind)
            assert ("re-solve" in A.schedule()) == (resolve and i > 0), (flags, kind, A.schedule())
            if B is not None:  # strict mode: the bits of the synchronous path
                B.set_rhs_flat(*[rhs[i][k] for k in RHS])
                assert B.solve() == 0
                assert same_bits(got, B.solutions()), (flags, kind)
        A.close()
        if B is not None:
            B.close()


@pytest.mark.parametrize("n,m,N", CASES)
def test_solutions_per_field(ndlqr, n, m, N):
    run_steps(ndlqr, n, m, N, [0, ndlqr.FLAG_STRICT_FP, ndlqr.FLAG_KEEP_FACT, ndlqr.FLAG_KEEP_RECORDS])


@pytest.mark.parametrize("n,m,N", [(12, 4, 16), (7, 9, 16)])
def test_keep_records_steps_are_resolves(ndlqr, monkeypatch, n, m, N):
    """The level-per-launch schedule (NDLQR_TREE=0; a batch this small runs the tree schedule otherwise, which keeps
    factoring) leaves compact records under KEEP_RECORDS: the first step factors, every further one is the re-solve."""
    monkeypatch.setenv("NDLQR_TREE", "0")
    run_steps(ndlqr, n, m, N, [ndlqr.FLAG_KEEP_RECORDS], resolve=True)


# ---------------------------------------------------------------------------- 3: slices against solutions(), bit for bit
def masks(ndlqr):
    return [ndlqr.SOLN_INPUT, ndlqr.SOLN_STATE | ndlqr.SOLN_INPUT, ndlqr.SOLN_LAMBDA, 7]


@pytest.mark.parametrize("n,m,N", CASES)
def test_slices_bit_for_bit(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    A = dense_solver(ndlqr, fam["probs"])
    rng = np.random.default_rng([n, m, N, 3])
    like = base_rhs(fam["probs"])
    count = 0
    for k0, nk in ranges(N):
        for blocks in masks(ndlqr):
            out = ndlqr.pinned_empty((cs.BATCH, nk, A.slice_width(blocks)))
            out[...] = 7.0
            kind = "F" if count % 3 == 0 else "X"
            count += 1
            assert step(ndlqr, A, draw(rng, like), kind, out, selection=(k0, nk, blocks)) == 0
            assert A.synchronize() == 0
            Z = A.solutions()
            assert same_bits(out, cut(Z, n, m, N, k0, nk, blocks)), (k0, nk, blocks)
            if k0 + nk == N and blocks & ndlqr.SOLN_INPUT:  # u of knot N-1: exact zero
                assert not out[:, -1, -m:].view(np.uint64).any()
    # the slices of a plain solve: synchronously, and computed alone
    assert A.solve() == 0
    Z = A.solutions()
    for k0, nk in ranges(N):
        for blocks in masks(ndlqr):
            assert same_bits(A.solution_slices_dense(k0, nk, blocks), cut(Z, n, m, N, k0, nk, blocks)), (k0, nk, blocks)
    for k0, nk in ranges(N):
        for blocks in masks(ndlqr):
            out = ndlqr.pinned_empty((cs.BATCH, nk, A.slice_width(blocks)))
            assert A.solve_slices_dense_async(k0, nk, blocks, out) == 0
            assert A.synchronize() == 0
            assert same_bits(out, cut(Z, n, m, N, k0, nk, blocks)), (k0, nk, blocks)
            assert same_bits(A.solution_slices_dense(k0, nk, blocks), out)  # (inside what the slice solve computed)
    A.close()


# ---------------------------------------------------------------------------- 4: SOLN_ONLY
@pytest.mark.parametrize("tree", [None, "0"])
@pytest.mark.parametrize("n,m,N", [(7, 9, 2), (6, 3, 5), (32, 8, 8), (12, 4, 16)])
def test_soln_only(ndlqr, monkeypatch, n, m, N, tree):
    """u of knot 0 alone: right at REL_TOL, and the bits of the same step without SOLN_ONLY (the diagonal-cost step has
    that property: the restricted back-substitution runs the same workgroups on the same data). Under KEEP_RECORDS a
    first step factors, so that both steps compared are re-solves (tree "0": the level-per-launch schedule, whose compact
    records have the re-solve and the restricted back-substitution)."""
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    fam = cs.family(n, m, N, "moderate")
    rng = np.random.default_rng([n, m, N, 4])
    merged = base_rhs(fam["probs"])
    new = draw(rng, merged)
    ref = references(fam["probs"], merge(merged, new, "X"))
    u0 = ref[:, 2 * n:2 * n + m]
    inp = ndlqr.SOLN_INPUT
    for flags in (0, ndlqr.FLAG_KEEP_RECORDS):
        A = dense_solver(ndlqr, fam["probs"], flags)
        whole = ndlqr.pinned_empty((cs.BATCH, A.nvars))
        assert step(ndlqr, A, merged, "X", whole) == 0
        outs = [ndlqr.pinned_empty((cs.BATCH, 1, m)) for _ in range(2)]
        assert step(ndlqr, A, new, "X", outs[0], selection=(0, 1, inp)) == 0
        assert step(ndlqr, A, new, "X", outs[1], selection=(0, 1, inp | ndlqr.SOLN_ONLY)) == 0
        assert A.synchronize() == 0
        for o in outs:
            err = float(np.abs(o[:, 0] - u0).max() / np.abs(u0).max())
            print("soln only", (n, m, N), flags, err)
            assert err <= REL_TOL, (flags, err)
        assert same_bits(outs[0], outs[1]), flags
        # the solver holds that slice alone ...
        with pytest.raises(RuntimeError):
            A.solutions()
        assert same_bits(A.solution_slices_dense(0, 1, inp), outs[1])
        # ... until the next complete step
        assert step(ndlqr, A, new, "X", whole) == 0
        assert A.synchronize() == 0
        assert same_bits(A.solutions(), whole)
        assert (errors(whole, ref, n, m, N) <= REL_TOL).all()
        A.close()


# ---------------------------------------------------------------------------- 5: the MPC loop
@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 16)])
def test_mpc_loop_two_in_flight(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    rng = np.random.default_rng([n, m, N, 5])
    merged = base_rhs(fam["probs"])
    A = dense_solver(ndlqr, fam["probs"])
    news, refs = [], []
    for i in range(6):
        kind = "F" if i % 2 == 0 else "X"
        news.append(draw(rng, merged))
        merged = merge(merged, news[-1], kind)
        refs.append(references(fam["probs"], merged)[:, 2 * n:2 * n + m])
    outs = [ndlqr.pinned_empty((cs.BATCH, 1, m)) for _ in range(6)]

    def check(i):
        err = float(np.abs(outs[i][:, 0] - refs[i]).max() / np.abs(refs[i]).max())
        print("mpc step", (n, m, N), i, err)
        assert err <= REL_TOL, (i, err)

    for i in range(6):
        assert step(ndlqr, A, news[i], "F" if i % 2 == 0 else "X", outs[i], selection=(0, 1, ndlqr.SOLN_INPUT)) == 0
        if i >= 1:
            assert A.synchronize_previous() == 0
            check(i - 1)
    assert A.synchronize() == 0
    check(5)
    # the first gain predicts the next input: K_0 dx0 = u_0(x0 + dx0) - u_0(x0)
    K0 = A.feedback_gains(0, 1, want=("K",))["K"][:, 0]
    x0 = merged["x0"]
    delta = 0.1 * rng.standard_normal(x0.shape)
    us = [ndlqr.pinned_empty((cs.BATCH, 1, m)) for _ in range(2)]
    for x, u in zip((x0, x0 + delta), us):
        assert step(ndlqr, A, dict(x0=x), "X", u, selection=(0, 1, ndlqr.SOLN_INPUT)) == 0
    assert A.synchronize() == 0
    A.close()
    for i in range(cs.BATCH):
        du = us[1][i, 0] - us[0][i, 0]
        err = float(np.abs(du - K0[i] @ delta[i]).max()) / float(np.abs(du).max())
        print("mpc gain", (n, m, N), i, "%.2e" % err)
        assert err <= REL_TOL, (i, err)


# ---------------------------------------------------------------------------- 6: state rules and refusals
def outcome(bs, call):
    """(refused, message): refused = the call returned a negative code or raised"""
    try:
        ret = call()
    except (RuntimeError, ValueError):
        return True, bs.L.ndlqr_hip_last_error().decode()
    if isinstance(ret, int) and ret < 0:
        return True, bs.L.ndlqr_hip_last_error().decode()
    return False, ""


def dense_calls(ndlqr, bs, selection=(0, 1, 7)):
    """(the name that opens a refusal, a call) for the three new entry points"""
    n, m, N, b = bs.n, bs.m, bs.N, bs.batch
    z = lambda *s: np.zeros(s)
    k0, nk, blocks = selection
    w = bs.slice_width(blocks)
    return [
        ("ndlqr_hip_step_dense_async",
         lambda: bs.step_dense_async(z(b, N, n), z(b, N, m), z(b, N, n), z(b, n), z(b, max(nk, 0), w), selection=selection)),
        ("ndlqr_hip_solve_slices_dense_async", lambda: bs.solve_slices_dense_async(k0, nk, blocks, z(b, max(nk, 0), w))),
        ("ndlqr_hip_download_selection_dense", lambda: bs.solution_slices_dense(k0, nk, blocks)),
    ]


def test_refusals(ndlqr):
    n, m, N = 12, 4, 8
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solver(ndlqr, fam["probs"])
    assert bs.solve() == 0
    z = lambda *s: np.zeros(s)
    b = cs.BATCH
    # the four plain entry points keep refusing in dense-cost mode, word for word
    plain = [
        ("ndlqr_hip_step_async", lambda: bs.step_async(z(b, N, n), z(b, N, m), z(b, N, n), z(b, n), z(b, bs.nvars))),
        ("ndlqr_hip_set_step_selection", lambda: bs.set_step_selection(0, 1, 7)),
        ("ndlqr_hip_solve_slices_async", lambda: bs.solve_slices_async(0, 1, 7, ndlqr.pinned_empty((b, 1, 2 * n + m)))),
        ("ndlqr_hip_download_selection", lambda: bs.solution_slices(0, 1, 7)),
    ]
    for who, call in plain:
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":") and "dense-cost" in msg, (who, refused, msg)
    # ... and the new ones work there
    for who, call in dense_calls(ndlqr, bs):
        refused, msg = outcome(bs, call)
        assert not refused, (who, msg)
        assert bs.synchronize() == 0
    # q without r: the wrapper, and the library by name
    with pytest.raises(ValueError):
        bs.step_dense_async(z(b, N, n), None, None, z(b, n), z(b, bs.nvars))
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    q, x0, out = z(b, N, n), z(b, n), z(b, bs.nvars)
    assert bs.L.ndlqr_BatchStepAsyncDense(bs.h, ptr(q), None, None, ptr(x0), 0, 0, 7, ptr(out)) == -1
    assert bs.L.ndlqr_hip_last_error().decode().startswith("ndlqr_hip_step_dense_async:")
    assert bs.L.ndlqr_BatchStepAsyncDense(bs.h, None, ptr(z(b, N, m)), None, ptr(x0), 0, 0, 7, ptr(out)) == -1
    assert bs.L.ndlqr_hip_last_error().decode().startswith("ndlqr_hip_step_dense_async:")
    # a slice past the caller's horizon
    for who, call in dense_calls(ndlqr, bs, selection=(N - 1, 2, 7)):
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":"), (who, refused, msg)
    # the solver still works (the step above left a zero right-hand side)
    bs.set_rhs_flat(*cs.flat(fam["probs"], RHS))
    assert bs.solve() == 0
    assert (errors(bs.solutions(), fam["z"], n, m, N) <= REL_TOL).all()
    # constrained mode: the step there is a follow-up
    A_, B_, Q_, H_, R_, q_, r_, d_, x0_ = cs.flat(fam["probs"])
    bs.initialize_flat_constrained(A_, B_, Q_, H_, R_, q_, r_, d_, x0_, z(b, N, n), z(b, N, m), np.array([-np.inf]),
                                   np.array([np.inf]))
    assert bs.cost_is_dense()
    for who, call in dense_calls(ndlqr, bs):
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":") and "constrained" in msg, (who, refused, msg)
    # diagonal mode
    gen = [ndlqr.generate_synthetic(n, m, N, 60 + i) for i in range(b)]
    bs.initialize_flat(*[np.stack([g[k] for g in gen]) for k in ("A", "B", "Q", "R", "q", "r", "d", "x0")])
    assert not bs.cost_is_dense() and bs.solve() == 0
    for who, call in dense_calls(ndlqr, bs):
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":") and "dense-cost" in msg, (who, refused, msg)
    assert bs.rhs_raw().shape[0] == b  # (the read-out works in every mode)
    bs.close()


def test_slice_past_a_padded_horizon_is_refused(ndlqr):
    """horizon 5 runs as 8 device knots: the caller's horizon bounds a slice, not the device's"""
    n, m, N = 6, 3, 5
    fam = cs.family(n, m, N, "moderate")
    bs = dense_solver(ndlqr, fam["probs"])
    assert bs.solve() == 0
    for who, call in dense_calls(ndlqr, bs, selection=(N - 1, 2, 7)):
        refused, msg = outcome(bs, call)
        assert refused and msg.startswith(who + ":"), (who, refused, msg)
    last = bs.solution_slices_dense(N - 1, 1, 7)
    assert same_bits(last, cut(bs.solutions(), n, m, N, N - 1, 1, 7))
    bs.close()


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 16)])
def test_state_after_steps_matches_set_rhs(ndlqr, n, m, N):
    """after dense steps, solve(), solve_adjoint() and feedback_gains() are those of set_rhs_flat with the same data"""
    fam = cs.family(n, m, N, "moderate")
    flags = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT
    A, B = dense_solver(ndlqr, fam["probs"], flags), dense_solver(ndlqr, fam["probs"], flags)
    rng = np.random.default_rng([n, m, N, 6])
    merged = base_rhs(fam["probs"])
    out = ndlqr.pinned_empty((cs.BATCH, A.nvars))
    for kind in ("F", "X", "QR"):
        new = draw(rng, merged)
        assert step(ndlqr, A, new, kind, out) == 0
        merged = merge(merged, new, kind)
    assert A.synchronize() == 0
    B.set_rhs_flat(*[merged[k] for k in RHS])
    assert B.solve() == 0
    assert same_bits(out, B.solutions())
    ga, gb = A.feedback_gains(), B.feedback_gains()
    for k in ("K", "k", "P", "p"):
        assert same_bits(ga[k], gb[k]), k
    assert A.solve_adjoint(fam["g"].copy()) == 0 and B.solve_adjoint(fam["g"].copy()) == 0
    assert same_bits(A.adjoint(), B.adjoint())
    assert A.solve() == 0
    assert same_bits(A.solutions(), B.solutions())
    # set_rhs_flat behind steps: the whole right-hand side again
    base = base_rhs(fam["probs"])
    A.set_rhs_flat(*[base[k] for k in RHS])
    assert A.solve() == 0
    assert (errors(A.solutions(), fam["z"], n, m, N) <= REL_TOL).all()
    A.close()
    B.close()


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 16)])
def test_nan_x0_stays_in_its_problem(ndlqr, n, m, N):
    fam = cs.family(n, m, N, "moderate")
    rng = np.random.default_rng([n, m, N, 7])
    new = draw(rng, base_rhs(fam["probs"]))
    outs = []
    for bad in (False, True):
        A = dense_solver(ndlqr, fam["probs"])
        arrs = {k: a.copy() for k, a in new.items()}
        if bad:
            arrs["x0"][1] = np.nan
        out = ndlqr.pinned_empty((cs.BATCH, A.nvars))
        assert step(ndlqr, A, arrs, "F", out) == 0
        A.synchronize()
        u0 = ndlqr.pinned_empty((cs.BATCH, 1, m))
        assert step(ndlqr, A, arrs, "X", u0, selection=(0, 1, ndlqr.SOLN_INPUT | ndlqr.SOLN_ONLY)) == 0
        A.synchronize()
        A.close()
        outs.append((out.copy(), u0.copy()))
    for i in (0, 2):
        assert np.isfinite(outs[1][0][i]).all()
        assert same_bits(outs[0][0][i], outs[1][0][i]) and same_bits(outs[0][1][i], outs[1][1][i]), i
    assert np.isnan(outs[1][0][1]).any()
