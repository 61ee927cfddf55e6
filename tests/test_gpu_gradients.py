"""Adjoint solve and parameter gradients (ndlqr_SolveBatchAdjoint, ndlqr_BatchGradients, rslqr_amd.autograd) against the
CPU oracle plus numpy: the adjoint K w = g is the oracle's solve of the adjoint problem (same A, B, Q, R; x0' = -g_lam0,
q'_k = -g_xk, r'_k = -g_uk, d'_k = -g_lam(k+1)), the gradients are the outer-product formulas of kernels_grad.hpp
evaluated by numpy on the oracle's z and w, and central differences of L = g . z through the oracle check the formulas.
Independently of the formulas, every forward schedule and the gradient kernel's edges are checked against the KKT operator
itself: <dL/dtheta, V> = w^T (r(z; theta + V) - r(z; theta)) in extended precision on the refined solution and adjoint
(support.gradient_direction_bar)."""
import numpy as np
import pytest

from support import Problem, gradient_direction_bar, refined_solution

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")


def synth(ndlqr, n, m, N, seed, a_scale=1.0, q_scale=1.0, r_scale=1.0):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    g["A"] = g["A"] * a_scale
    g["Q"] = g["Q"] * q_scale
    g["R"] = g["R"] * r_scale
    return Problem(n, m, N, *[g[k] for k in ARGS])


def stack(probs):
    return [np.stack([getattr(p, k) for p in probs]) for k in ARGS]


def blocks(v, n, m, N):
    out = np.zeros(N * (2 * n + m))
    out[: v.size] = v
    return out.reshape(N, 2 * n + m)


def adjoint_problem(prob, g):
    n, m, N = prob.n, prob.m, prob.N
    G = blocks(g, n, m, N)
    r = -G[:, 2 * n:]
    r[N - 1] = 0.0
    d = np.zeros((N, n))
    d[: N - 1] = -G[1:, :n]
    return Problem(n, m, N, prob.A, prob.B, prob.Q, prob.R, -G[:, n:2 * n], r, d, -G[0, :n])


def grad_formula(prob, z, w):
    """The gradients of kernels_grad.hpp from z and w (strict operation order), flat layout of one problem."""
    n, m, N = prob.n, prob.m, prob.N
    Z, W = blocks(z, n, m, N), blocks(w, n, m, N)
    lz, xz, uz = Z[:, :n], Z[:, n:2 * n], Z[:, 2 * n:]
    lw, xw, uw = W[:, :n], W[:, n:2 * n], W[:, 2 * n:]
    out = {k: np.zeros(getattr(prob, k).shape) for k in ARGS}
    out["x0"] = -lw[0]
    out["q"] = -xw
    out["Q"] = -(xw * xz)
    for k in range(N - 1):
        for name, cz, cw, cols in (("A", xz, xw, n), ("B", uz, uw, m)):
            t1 = lw[k + 1][:, None] * cz[k][None, :]
            t2 = lz[k + 1][:, None] * cw[k][None, :]
            s = t1 + t2
            out[name][k] = (-s).T.reshape(n * cols)  # (i, j) at i + n j
        out["R"][k] = -(uw[k] * uz[k])
        out["r"][k] = -uw[k]
        out["d"][k] = -lw[k + 1]
    return out


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def directions(prob, seed):
    """(argument, label, V): one random direction per argument over all of it, then one confined to knot 0, a middle
    knot, knot N - 2 and the last knot (x0 has no knots: the whole of it once)."""
    rng = np.random.default_rng(seed)
    N = prob.N
    out = []
    for k in ARGS:
        shape = getattr(prob, k).shape
        out.append((k, "all", rng.standard_normal(shape)))
        if k == "x0":
            continue
        for knot in sorted({0, N // 2, N - 2, N - 1}):
            V = np.zeros(shape)
            V[knot] = rng.standard_normal(shape[1:])
            out.append((k, "knot %d" % knot, V))
    return out


def check_directions(prob, grads, z, w, z_true, w_true, seed):
    """<G, V> of the gradients G (one problem, computed from z and w) against the KKT operator applied to the truths, for
    every direction of directions(); the last knot of A, B, R, r, d exactly zero."""
    for k, label, V in directions(prob, seed):
        got = (np.asarray(grads[k], dtype=np.longdouble) * V).sum()
        ref, bar = gradient_direction_bar(prob, k, V, z, w, z_true, w_true)
        assert abs(got - ref) <= bar, (k, label, float(got), float(ref), float(bar))
        if k in ("A", "B", "R", "r", "d"):
            assert not np.any(grads[k][prob.N - 1]), (k, "last knot")


def check_against_truth(oracle, prob, g, z, w, grads, seed):
    """w against the refined adjoint (norm-wise, no worse than 10x the oracle's own error), then every direction."""
    ap = adjoint_problem(prob, g)
    z_true = refined_solution(oracle, prob)
    w_true = refined_solution(oracle, ap)
    w_oracle = oracle.solve(ap, 8)[0][: prob.nvars]
    err_gpu, err_oracle = rel(w, w_true), rel(w_oracle, w_true)
    assert err_gpu <= 10 * err_oracle + 1e-13, (err_gpu, err_oracle)
    check_directions(prob, grads, z, w, z_true, w_true, seed)


def references(oracle, probs, g):
    """(z, w, gradients) of every problem from the oracle."""
    out = []
    for p, prob in enumerate(probs):
        z = oracle.solve(prob, 1)[0][: prob.nvars]
        w = oracle.solve(adjoint_problem(prob, g[p]), 1)[0][: prob.nvars]
        out.append((z, w, grad_formula(prob, z, w)))
    return out


# ------------------------------------------------------------------------------------------------ strict, bit-exact

# (tuples of test_gpu_parity.SHAPES, the padded (7, 9, 16) among them, and one beyond 16 states)
STRICT_SHAPES = [(6, 3, 16), (12, 4, 64), (5, 2, 32), (13, 4, 32), (3, 1, 2), (7, 9, 16), (20, 6, 32)]


@pytest.mark.parametrize("n,m,N", STRICT_SHAPES)
def test_strict_adjoint_and_gradients_bit_exact(ndlqr, oracle, n, m, N):
    batch = 3
    probs = [synth(ndlqr, n, m, N, 300 + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    g = np.random.default_rng(1).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    w = bs.adjoint()
    grads = bs.gradients()
    for p, (zr, wr, gr) in enumerate(references(oracle, probs, g)):
        assert np.array_equal(w[p], wr), (p, rel(w[p], wr))
        for k in ARGS:
            assert np.array_equal(grads[k][p], gr[k]), (p, k, rel(grads[k][p], gr[k]))
    bs.close()


# ------------------------------------------------------------------------------------------------ fast mode, every path

# (n, m, N, batch, flags, NDLQR_TREE, schedule of the solve): compact records of the level-per-launch schedule, the
# tree form at batch 1 (full records), the runtime-sized records, a padded shape, the factor-array sweep
FAST_CASES = [(12, 4, 64, 3, "records", "0", "reduced-compact-records"),
              (12, 4, 256, 1, "records", None, "reduced-tree"),
              (32, 8, 128, 1, "records", None, "generic-reduced-records"),
              (64, 16, 64, 1, "records", None, "generic-reduced-records"),
              (11, 3, 64, 2, "records", "0", "reduced-compact-records"),
              (20, 6, 32, 2, "fact", None, "generic-keep"),
              (12, 4, 64, 2, "fact", None, "knot-keep")]
FAMILIES = [(1.0, 1.0, 1.0), (1.0, 1e-4, 1.0), (1.0, 1.0, 1e-4)]


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", FAST_CASES)
@pytest.mark.parametrize("a_scale,q_scale,r_scale", FAMILIES)
def test_fast_adjoint_and_gradients(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want, a_scale, q_scale,
                                    r_scale):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 400 + p, a_scale, q_scale, r_scale) for p in range(batch)]
    fl = ndlqr.FLAG_KEEP_RECORDS if flags == "records" else ndlqr.FLAG_KEEP_FACT
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=fl)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    assert bs.schedule() == want, bs.schedule()
    g = np.random.default_rng(2).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    w = bs.adjoint()
    grads = bs.gradients()
    for p, (zr, wr, gr) in enumerate(references(oracle, probs, g)):
        assert rel(w[p], wr) <= REL_TOL, (p, rel(w[p], wr))
        for k in ARGS:
            assert rel(grads[k][p], gr[k]) <= REL_TOL, (p, k, rel(grads[k][p], gr[k]))
    bs.close()


# ------------------------------------------------------------------------------------------------ primal state

def test_primal_state_preserved(ndlqr, oracle, monkeypatch):
    monkeypatch.setenv("NDLQR_TREE", "0")
    n, m, N, batch = 12, 4, 64, 4
    probs = [synth(ndlqr, n, m, N, 500 + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    sol0 = bs.solutions().copy()
    res0, bn0 = bs.kkt_residuals()
    g = np.random.default_rng(3).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    bs.gradients()
    assert np.array_equal(bs.solutions(), sol0)
    res1, bn1 = bs.kkt_residuals()
    assert np.array_equal(res0, res1) and np.array_equal(bn0, bn1)
    # an x0-only step and a plain re-solve afterwards: against the oracle on the primal q, r, d with the new x0
    x0 = ndlqr.pinned_empty((batch, n))
    x0[:] = np.random.default_rng(4).standard_normal((batch, n))
    soln = ndlqr.pinned_empty((batch, bs.nvars))
    assert bs.step_async(None, None, None, x0, soln) == 0
    assert bs.synchronize() == 0
    moved = [Problem(n, m, N, p.A, p.B, p.Q, p.R, p.q, p.r, p.d, x0[i].copy()) for i, p in enumerate(probs)]
    refs = [oracle.solve(p, 1)[0][: p.nvars] for p in moved]
    for p in range(batch):
        assert rel(soln[p], refs[p]) <= REL_TOL
    assert bs.solve_rhs_only() == 0
    sol = bs.solutions()
    for p in range(batch):
        assert rel(sol[p], refs[p]) <= REL_TOL
    bs.close()


# ------------------------------------------------------------------------------------------------ batch sums

@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 64, 5), (12, 4, 256, 100), (6, 3, 16, 1), (32, 8, 32, 6)])
def test_batch_sum(ndlqr, n, m, N, batch):
    probs = [synth(ndlqr, n, m, N, 600 + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    g = np.random.default_rng(5).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    per = bs.gradients()
    full = bs.gradients(0xFF)
    again = bs.gradients(0xFF)
    for k in ARGS:
        assert full[k].shape == per[k].shape[1:]
        assert rel(full[k], per[k].sum(axis=0)) <= 1e-12, k
        assert np.array_equal(full[k], again[k]), k
    mixed = bs.gradients(ndlqr.GRAD_A | ndlqr.GRAD_B | ndlqr.GRAD_x0)
    for k in ARGS:
        if k in ("A", "B", "x0"):
            assert np.array_equal(mixed[k], full[k]), k
        else:
            assert np.array_equal(mixed[k], per[k]), k
    bs.close()


# ------------------------------------------------------------------------------------------------ pointer kinds

def test_pointer_kinds(ndlqr):
    n, m, N, batch = 12, 4, 64, 3
    probs = [synth(ndlqr, n, m, N, 700 + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    g = np.random.default_rng(6).standard_normal((batch, bs.nvars))
    gp = ndlqr.pinned_empty(g.shape)
    gp[:] = g
    results = []
    for src in (g, gp, ndlqr.DeviceArray(g.shape).set(g)):
        assert bs.solve_adjoint(src) == 0
        for kind in ("pageable", "pinned", "device"):
            for mask in (0, ndlqr.GRAD_A | ndlqr.GRAD_q):
                out = {}
                for i, k in enumerate(ARGS):
                    shape = bs.gradient_shape(k, bool(mask & (1 << i)))
                    out[k] = np.zeros(shape) if kind == "pageable" else \
                        (ndlqr.pinned_empty(shape) if kind == "pinned" else ndlqr.DeviceArray(shape))
                bs.gradients(mask, out)
                got = {k: (v.get() if kind == "device" else np.array(v)) for k, v in out.items()}
                wd = ndlqr.DeviceArray((batch, bs.nvars)) if kind == "device" else None
                w = bs.adjoint(wd).get() if wd is not None else bs.adjoint(
                    ndlqr.pinned_empty((batch, bs.nvars)) if kind == "pinned" else None).copy()
                results.append((mask, got, w))
    for mask, got, w in results[2:]:
        base = results[0] if mask == 0 else results[1]
        assert np.array_equal(w, base[2])
        for k in ARGS:
            assert np.array_equal(got[k], base[1][k]), (mask, k)
    # NULL outputs: the others come out the same
    some = bs.gradients(0, {"B": np.zeros((batch, N, n * m)), "x0": np.zeros((batch, n))})
    assert set(some) == {"B", "x0"}
    assert np.array_equal(some["B"], results[0][1]["B"]) and np.array_equal(some["x0"], results[0][1]["x0"])
    bs.close()


# ------------------------------------------------------------------------------------------------ refusals

def _grad_code(bs):
    return bs.L.ndlqr_BatchGradients(bs.h, 0, *([None] * 8))


def _check_solves(ndlqr, oracle, bs, probs):
    assert bs.solve() == 0
    sol = bs.solutions()
    for p, prob in enumerate(probs):
        ref = oracle.solve(prob, 1)[0][: prob.nvars]
        assert rel(sol[p], ref) <= REL_TOL


def test_refusals(ndlqr, oracle, monkeypatch):
    monkeypatch.setenv("NDLQR_TREE", "0")
    n, m, N, batch = 12, 4, 64, 2
    probs = [synth(ndlqr, n, m, N, 800 + p) for p in range(batch)]
    g = np.random.default_rng(7).standard_normal((batch, (2 * n + m) * N - m))
    # no kept factorisation
    bs = ndlqr.BatchSolver(n, m, N, batch)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    assert bs.solve_adjoint(g) == -1
    assert _grad_code(bs) == -1  # (gradients with no adjoint)
    _check_solves(ndlqr, oracle, bs, probs)
    bs.close()
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    assert _grad_code(bs) == -1
    # after a step that computed a slice alone
    bs.set_step_selection(0, 8, ndlqr.SOLN_INPUT | ndlqr.SOLN_ONLY)
    x0 = ndlqr.pinned_empty((batch, n))
    x0[:] = np.stack([p.x0 for p in probs])
    out = ndlqr.pinned_empty((batch, 8, m))
    assert bs.step_async(None, None, None, x0, out) == 0
    assert bs.synchronize() == 0
    assert bs.solve_adjoint(g) == -1
    bs.set_step_selection()
    _check_solves(ndlqr, oracle, bs, probs)
    # gradients after a later solve
    assert bs.solve_adjoint(g) == 0
    assert _grad_code(bs) == 0
    assert bs.solve() == 0
    assert _grad_code(bs) == -1
    with pytest.raises(RuntimeError):
        bs.adjoint()
    # after new inputs are uploaded
    assert bs.solve_adjoint(g) == 0
    bs.initialize_flat(*stack(probs))
    assert _grad_code(bs) == -1
    assert bs.solve_adjoint(g) == -1
    _check_solves(ndlqr, oracle, bs, probs)
    assert bs.solve_adjoint(g) == 0 and _grad_code(bs) == 0
    bs.close()


# ------------------------------------------------------------------------------------------------ finite differences

@pytest.mark.parametrize("n,m,N,batch", [(3, 2, 8, 2), (2, 1, 4, 3)])
def test_finite_differences(ndlqr, oracle, n, m, N, batch):
    probs = [synth(ndlqr, n, m, N, 900 + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    g = np.random.default_rng(8).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    grads = bs.gradients()
    for p, prob in enumerate(probs):
        def loss(pr):
            return float(g[p] @ oracle.solve(pr, 1)[0][: pr.nvars])
        for k in ARGS:
            base = getattr(prob, k)
            fd = np.zeros(base.size)
            for e in range(base.size):
                h = 1e-5 * max(1.0, abs(base.flat[e]))
                vals = []
                for sgn in (1.0, -1.0):
                    arr = base.copy()
                    arr.flat[e] += sgn * h
                    kw = {a: getattr(prob, a) for a in ARGS}
                    kw[k] = arr
                    vals.append(loss(Problem(n, m, N, *[kw[a] for a in ARGS])))
                fd[e] = (vals[0] - vals[1]) / (2 * h)
            got = grads[k][p].ravel()
            assert np.linalg.norm(got - fd) <= 1e-6 * max(1.0, np.linalg.norm(fd)), (p, k, got, fd)
    bs.close()


# ------------------------------------------------------------------------------------------------ torch
# Each case runs in a fresh process that initialises torch's device before the library's: torch ships its own HIP
# runtime next to the system one this library links, and the second of the two to start in a process may find no device
# (test_gpu_parity.test_device_side_packing_matches_host_packing does the same).

def _run_case(name, *args):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_gradients as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("n,m,N,batch,shared", [(6, 3, 16, 3, False), (6, 3, 16, 3, True), (12, 4, 16, 2, False),
                                                (12, 4, 16, 2, True)])
def test_torch_against_dense_reference(n, m, N, batch, shared):
    """lqr_solve's gradients against a dense KKT system assembled in torch and solved by torch.linalg.solve with
    autograd, per-problem inputs and a shared A, B (batch-sum gradients)."""
    _run_case("_case_dense_reference", n, m, N, batch, shared)


def test_torch_backwards_in_reverse_order():
    """Two forwards on one cached solver, then their backwards in reverse order: each redoes its own factorisation."""
    _run_case("_case_backwards_in_reverse_order")


def test_torch_gradcheck():
    _run_case("_case_gradcheck")


def test_torch_refuses_bad_arguments():
    """The wrong dtype, CPU tensors, mixed devices and matrix-shaped Q raise."""
    _run_case("_case_refuses_bad_arguments")


def _torch_problem(ndlqr, n, m, N, batch, seed, shared_AB=False):
    import torch
    probs = [synth(ndlqr, n, m, N, seed + p) for p in range(batch)]
    arrs = stack(probs)
    t = {}
    for k, a in zip(ARGS, arrs):
        if k in ("A", "B"):
            cols = n if k == "A" else m
            a = a.reshape(batch, N, cols, n).transpose(0, 1, 3, 2)  # column-major flat -> row-major matrices
            if shared_AB:
                a = a[0]
        t[k] = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)
    return t


def _dense_solve(t, n, m, N, batch):
    """z [batch, nvars] from the dense KKT system assembled in torch (torch.linalg.solve, differentiable)."""
    import torch
    zb = 2 * n + m
    nv = zb * N - m
    zs = []
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    for p in range(batch):
        get = lambda k: t[k] if t[k].dim() == {"A": 3, "B": 3, "Q": 2, "R": 2, "q": 2, "r": 2, "d": 2, "x0": 1}[k] else t[k][p]
        A, B, Q, R, q, r, d, x0 = [get(k) for k in ARGS]
        K = torch.zeros((nv, nv), dtype=torch.float64, device="cuda")
        b = torch.zeros(nv, dtype=torch.float64, device="cuda")
        K[0:n, n:2 * n] = -eye
        K[n:2 * n, 0:n] = -eye
        b[0:n] = -x0
        for k in range(N):
            lo, xo, uo = k * zb, k * zb + n, k * zb + 2 * n
            K[xo:xo + n, xo:xo + n] = torch.diag(Q[k])
            b[xo:xo + n] = -q[k]
            if k == N - 1:
                break
            l1, x1 = (k + 1) * zb, (k + 1) * zb + n
            K[uo:uo + m, uo:uo + m] = torch.diag(R[k])
            b[uo:uo + m] = -r[k]
            K[l1:l1 + n, xo:xo + n] = A[k]
            K[xo:xo + n, l1:l1 + n] = A[k].T
            K[l1:l1 + n, uo:uo + m] = B[k]
            K[uo:uo + m, l1:l1 + n] = B[k].T
            K[l1:l1 + n, x1:x1 + n] = -eye
            K[x1:x1 + n, l1:l1 + n] = -eye
            b[l1:l1 + n] = -d[k]
        zs.append(torch.linalg.solve(K, b))
    return torch.stack(zs)


def _grads(fn, t, gz):
    for v in t.values():
        v.grad = None
    z = fn()
    (z * gz).sum().backward()
    return z.detach(), {k: v.grad.detach().clone() for k, v in t.items()}


def _case_dense_reference(ndlqr, n, m, N, batch, shared):
    import torch
    from rslqr_amd.autograd import lqr_solve, split_solution
    t = _torch_problem(ndlqr, n, m, N, batch, 1000, shared_AB=shared)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    z, got = _grads(lambda: lqr_solve(*[t[k] for k in ARGS]), t, gz)
    zr, ref = _grads(lambda: _dense_solve(t, n, m, N, batch), t, gz)
    assert rel(z.cpu().numpy(), zr.cpu().numpy()) <= REL_TOL
    for k in ARGS:
        assert got[k].shape == t[k].shape, k
        assert rel(got[k].cpu().numpy(), ref[k].cpu().numpy()) <= 1e-8, k
    lam, x, u = split_solution(z, n, m, N)
    assert lam.shape == (batch, N, n) and x.shape == (batch, N, n) and u.shape == (batch, N - 1, m)
    assert torch.allclose(x[:, 0], t["x0"].detach(), rtol=1e-12, atol=1e-12)  # x_0 = x0


def _case_backwards_in_reverse_order(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve
    n, m, N, batch = 6, 3, 16, 2
    t1 = _torch_problem(ndlqr, n, m, N, batch, 1100)
    t2 = _torch_problem(ndlqr, n, m, N, batch, 1200)
    gz = torch.randn((batch, (2 * n + m) * N - m), dtype=torch.float64, device="cuda")
    _, ref1 = _grads(lambda: _dense_solve(t1, n, m, N, batch), t1, gz)
    _, ref2 = _grads(lambda: _dense_solve(t2, n, m, N, batch), t2, gz)
    for v in list(t1.values()) + list(t2.values()):
        v.grad = None
    z1 = lqr_solve(*[t1[k] for k in ARGS])
    z2 = lqr_solve(*[t2[k] for k in ARGS])  # (same shape: the same cached solver)
    (z2 * gz).sum().backward()
    (z1 * gz).sum().backward()
    for t, ref in ((t1, ref1), (t2, ref2)):
        for k in ARGS:
            assert rel(t[k].grad.cpu().numpy(), ref[k].cpu().numpy()) <= 1e-8, k


def _case_gradcheck(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve
    t = _torch_problem(ndlqr, 3, 2, 8, 2, 1300)
    assert torch.autograd.gradcheck(lqr_solve, tuple(t[k] for k in ARGS), eps=1e-6, atol=1e-6, rtol=1e-5)


def _case_refuses_bad_arguments(ndlqr):
    import torch
    from rslqr_amd.autograd import lqr_solve
    n, m, N, batch = 3, 2, 8, 2
    t = {k: v.detach() for k, v in _torch_problem(ndlqr, n, m, N, batch, 1400).items()}
    with pytest.raises(TypeError):
        lqr_solve(*[t[k].float() if k == "Q" else t[k] for k in ARGS])
    with pytest.raises(ValueError):
        lqr_solve(*[t[k].cpu() for k in ARGS])
    with pytest.raises(ValueError):
        lqr_solve(*[t[k].cpu() if k == "x0" else t[k] for k in ARGS])
    with pytest.raises(ValueError, match="diagonals"):
        lqr_solve(*[torch.diag_embed(t[k]) if k == "Q" else t[k] for k in ARGS])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            lqr_solve(*[t[k].to("cuda:1") if k == "R" else t[k] for k in ARGS])


# ------------------------------------------------------------------------------------------------ every forward schedule
# Each schedule a solve can leave behind for an adjoint, named as ndlqr_hip_schedule reports it, with the checks of
# check_against_truth (formula-free: the KKT operator on the refined solution and adjoint). A schedule not listed here has
# no gradient case. KEEP_RECORDS: reduced-compact-records (level-per-launch, chosen by batch size alone and with
# NDLQR_TREE=0), reduced-tree (full records, batch 1 and batch > 1), generic-reduced-records (runtime-sized records, also
# at N = 2 and 4), generic-keep (records kept as factors beyond 128 states), knot-lean (an instance off the matrix cores,
# (2,1)). KEEP_FACT:
# generic-keep, knot-keep. STRICT_FP | KEEP_FACT: knot-strict, generic-strict. Padded buckets: (7,9), (11,3), (1,1).
# (n, m, N, batch, flags, NDLQR_TREE, schedule, problems checked against the refined truth)
SCHEDULE_CASES = [(12, 4, 64, 160, "records", None, "reduced-compact-records", (0, 159)),
                  (12, 4, 64, 3, "records", "0", "reduced-compact-records", (1,)),
                  (12, 4, 256, 1, "records", None, "reduced-tree", (0,)),
                  (6, 3, 64, 3, "records", None, "reduced-tree", (0, 2)),
                  (32, 8, 128, 1, "records", None, "generic-reduced-records", (0,)),
                  (5, 2, 2, 3, "records", None, "generic-reduced-records", (0, 2)),
                  (6, 3, 4, 2, "records", None, "generic-reduced-records", (1,)),
                  (144, 16, 8, 1, "records", None, "generic-keep", (0,)),
                  (7, 9, 16, 2, "records", "0", "reduced-compact-records", (1,)),
                  (11, 3, 64, 2, "records", "0", "reduced-compact-records", (0,)),
                  (1, 1, 16, 3, "records", None, "reduced-tree", (0, 2)),
                  (2, 1, 64, 3, "records", None, "knot-lean", (1,)),
                  (20, 6, 32, 2, "fact", None, "generic-keep", (1,)),
                  (12, 4, 64, 2, "fact", None, "knot-keep", (0,)),
                  (6, 3, 4, 2, "fact", None, "generic-keep", (0,)),
                  (12, 4, 16, 2, "strict", None, "knot-strict", (1,)),
                  (20, 6, 16, 2, "strict", None, "generic-strict", (0,))]
SCHEDULE_FAMILIES = [(1.0, 1.0, 1.0), (1.3, 1e-3, 1.0), (1.0, 1.0, 1e-4)]
_FLAGS = {"records": "FLAG_KEEP_RECORDS", "fact": "FLAG_KEEP_FACT", "strict": None}


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want,check", SCHEDULE_CASES,
                         ids=["%s-%d.%d.%d.x%d" % (c[6], c[0], c[1], c[2], c[3]) for c in SCHEDULE_CASES])
@pytest.mark.parametrize("a_scale,q_scale,r_scale", SCHEDULE_FAMILIES)
def test_every_schedule_against_the_kkt_operator(ndlqr, oracle, monkeypatch, n, m, N, batch, flags, tree, want, check,
                                                  a_scale, q_scale, r_scale):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    probs = [synth(ndlqr, n, m, N, 1500 + p, a_scale, q_scale, r_scale) for p in range(batch)]
    fl = ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT if flags == "strict" else getattr(ndlqr, _FLAGS[flags])
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=fl)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    assert bs.schedule() == want, bs.schedule()
    z = bs.solutions().copy()
    g = np.random.default_rng(11).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    assert np.array_equal(bs.solutions(), z)
    w = bs.adjoint()
    grads = bs.gradients()
    assert np.array_equal(bs.solutions(), z)
    for p, prob in enumerate(probs):
        wr = oracle.solve(adjoint_problem(prob, g[p]), 8)[0][: prob.nvars]
        assert rel(w[p], wr) <= REL_TOL, (p, rel(w[p], wr))
    for p in check:
        check_against_truth(oracle, probs[p], g[p], z[p], w[p], {k: grads[k][p] for k in ARGS}, 20 + p)
    bs.close()


# ------------------------------------------------------------------------------------------------ gradient kernel edges

def _ld_sum_bar(per):
    """(sum over the batch in longdouble, batch eps sum |terms|) of per-problem outputs [batch, ...]."""
    t = np.asarray(per, dtype=np.longdouble)
    return t.sum(axis=0), per.shape[0] * np.finfo(np.float64).eps * np.abs(t).sum(axis=0)


def _check_sums(full, per, keys):
    for k in keys:
        s, bar = _ld_sum_bar(per[k])
        assert full[k].shape == per[k].shape[1:], k
        assert (np.abs(full[k] - s) <= bar).all(), (k, float(np.abs(full[k] - s).max()))


def _solved(ndlqr, n, m, N, batch, seed, flags=None):
    probs = [synth(ndlqr, n, m, N, seed + p) for p in range(batch)]
    bs = ndlqr.BatchSolver(n, m, N, batch, flags=ndlqr.FLAG_KEEP_RECORDS if flags is None else flags)
    bs.initialize_flat(*stack(probs))
    assert bs.solve() == 0
    g = np.random.default_rng(seed).standard_normal((batch, bs.nvars))
    assert bs.solve_adjoint(g) == 0
    return bs, probs, g


# (n, m, N, batch): beyond 64 KB of dynamic LDS at one knot per workgroup (96,16); one knot's summed gA beyond the LDS of
# a workgroup (144,16), (150,10) padded, (256,32): its entries spread over several workgroups
@pytest.mark.parametrize("n,m,N,batch", [(96, 16, 8, 3), (144, 16, 8, 3), (150, 10, 4, 2), (256, 32, 4, 2)])
def test_batch_sums_of_large_blocks(ndlqr, n, m, N, batch):
    bs, probs, g = _solved(ndlqr, n, m, N, batch, 1600)
    per = bs.gradients()
    full = bs.gradients(0xFF)
    _check_sums(full, per, ARGS)
    again = bs.gradients(0xFF)
    for k in ARGS:
        assert np.array_equal(full[k], again[k]), k
    if n in (144, 256):  # every set of summed outputs with A or B in it; the rest per problem, as before
        for mask in range(256):
            if not mask & 3:
                continue
            got = bs.gradients(mask)
            for i, k in enumerate(ARGS):
                if mask & (1 << i):
                    assert np.array_equal(got[k], full[k]), (mask, k)
                else:
                    assert np.array_equal(got[k], per[k]), (mask, k)
    bs.close()


@pytest.mark.parametrize("n,m,N,batch", [(12, 4, 256, 100), (144, 16, 64, 24), (6, 3, 16, 1)])
def test_batch_sums_split_and_not_adjacent(ndlqr, n, m, N, batch):
    """Batches split over several workgroup rows of several problems each (ppb > 1, nsplit > 1: (12,4,256) x 100 and the
    sliced gA of (144,16,64) x 24), batch 1, and summed outputs that are not neighbours in GradOut order (the output
    search of grad_sum_splits)."""
    bs, probs, g = _solved(ndlqr, n, m, N, batch, 1700)
    if n == 144:  # (gA alone: the per-problem arrays of all eight would be large)
        per = bs.gradients(0, {"A": np.zeros((batch, N, n * n))})
        full = bs.gradients(ndlqr.GRAD_A, {"A": np.zeros((N, n * n))})
        _check_sums(full, per, ["A"])
        again = bs.gradients(ndlqr.GRAD_A, {"A": np.zeros((N, n * n))})
        assert np.array_equal(full["A"], again["A"])
        bs.close()
        return
    per = bs.gradients()
    for mask in (ndlqr.GRAD_B | ndlqr.GRAD_x0, ndlqr.GRAD_Q | ndlqr.GRAD_d, ndlqr.GRAD_A | ndlqr.GRAD_r,
                 ndlqr.GRAD_R | ndlqr.GRAD_x0, ndlqr.GRAD_x0, ndlqr.GRAD_q):
        got = bs.gradients(mask)
        summed = [k for i, k in enumerate(ARGS) if mask & (1 << i)]
        _check_sums(got, per, summed)
        for k in ARGS:
            if k not in summed:
                assert np.array_equal(got[k], per[k]), (mask, k)
        again = bs.gradients(mask)
        for k in ARGS:
            assert np.array_equal(got[k], again[k]), (mask, k)
    bs.close()


def test_strict_bit_exact_beyond_128_states(ndlqr):
    """Strict mode at (144,16): every per-problem output bit for bit what numpy computes from the device's z and w, and
    the batch sums (their entries spread over several workgroups) within the rounding of a sum."""
    n, m, N, batch = 144, 16, 4, 2
    bs, probs, g = _solved(ndlqr, n, m, N, batch, 1800, ndlqr.FLAG_STRICT_FP | ndlqr.FLAG_KEEP_FACT)
    z, w = bs.solutions(), bs.adjoint()
    per = bs.gradients()
    for p, prob in enumerate(probs):
        want = grad_formula(prob, z[p], w[p])
        for k in ARGS:
            assert np.array_equal(per[k][p], want[k]), (p, k)
    _check_sums(bs.gradients(0xFF), per, ARGS)
    bs.close()


# ------------------------------------------------------------------------------------------------ lqr_solve edges

@pytest.mark.parametrize("case", ["shared_alone", "partial_and_layouts", "horizons", "large_shared_A"])
def test_torch_edges(case):
    """lqr_solve against the dense torch reference: each argument shared alone; requires_grad on a subset; expanded
    (stride-0), transposed and sliced A, B; a non-contiguous incoming gradient; batch 1, N = 2, N = 64; a shared A at
    (144,16), whose batch-summed gA spreads over several workgroups."""
    _run_case("_case_edges", case)


def _leaves(ndlqr, n, m, N, batch, seed, shared=()):
    """Leaf tensors of a problem (row-major A, B), the arguments in `shared` without the batch dimension."""
    import torch
    t = _torch_problem(ndlqr, n, m, N, batch, seed)
    return {k: (v.detach()[0].clone() if k in shared else v.detach().clone()).requires_grad_(True) for k, v in t.items()}


def _compare(args, leaves, n, m, N, batch, gz, backward_with=None):
    """z and the leaves' gradients through lqr_solve(args) against the same through _dense_solve(args)."""
    import torch
    from rslqr_amd.autograd import lqr_solve
    res = []
    for fn in (lambda: lqr_solve(*[args[k] for k in ARGS]), lambda: _dense_solve(args, n, m, N, batch)):
        for v in leaves.values():
            v.grad = None
        z = fn()
        z.backward(gz)
        res.append((z.detach(), {k: (None if v.grad is None else v.grad.clone()) for k, v in leaves.items()}))
    (z, got), (zr, ref) = res
    assert rel(z.cpu().numpy(), zr.cpu().numpy()) <= REL_TOL
    for k in leaves:
        if ref[k] is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None and got[k].shape == leaves[k].shape, k
        assert rel(got[k].cpu().numpy(), ref[k].cpu().numpy()) <= 1e-8, k


def _case_edges(ndlqr, case):
    import torch
    from rslqr_amd.autograd import lqr_solve
    nv = lambda n, m, N: (2 * n + m) * N - m
    if case == "shared_alone":
        n, m, N, batch = 6, 3, 16, 3
        gz = torch.randn((batch, nv(n, m, N)), dtype=torch.float64, device="cuda")
        for k in ARGS:
            leaves = _leaves(ndlqr, n, m, N, batch, 1900, shared=(k,))
            _compare(leaves, leaves, n, m, N, batch, gz)
    elif case == "partial_and_layouts":
        n, m, N, batch = 6, 3, 16, 3
        gz = torch.randn((batch, nv(n, m, N)), dtype=torch.float64, device="cuda")
        # requires_grad on a subset: the others come back None
        for subset in (("A",), ("B", "x0"), ("Q", "d", "r"), ("R", "q")):
            leaves = _leaves(ndlqr, n, m, N, batch, 2000)
            for k in ARGS:
                if k not in subset:
                    leaves[k].requires_grad_(False)
            z = lqr_solve(*[leaves[k] for k in ARGS])
            z.backward(gz)
            for k in ARGS:
                assert (leaves[k].grad is None) == (k not in subset), k
            _compare(leaves, leaves, n, m, N, batch, gz)
        # expanded (stride 0) A and B: one leaf each, broadcast by expand
        leaves = _leaves(ndlqr, n, m, N, batch, 2100, shared=("A", "B"))
        args = dict(leaves)
        args["A"] = leaves["A"].expand(batch, N, n, n)
        args["B"] = leaves["B"].expand(batch, N, n, m)
        assert args["A"].stride(0) == 0
        _compare(args, leaves, n, m, N, batch, gz)
        # transposed A (a leaf that holds A^T: the argument is its transpose) and B sliced from a wider tensor
        leaves = _leaves(ndlqr, n, m, N, batch, 2200)
        leaves["AT"] = leaves.pop("A").detach().transpose(-1, -2).contiguous().requires_grad_(True)
        leaves["Bw"] = torch.nn.functional.pad(leaves.pop("B").detach(), (0, 2)).requires_grad_(True)
        args = {k: leaves[k] for k in ARGS if k in leaves}
        args["A"] = leaves["AT"].transpose(-1, -2)
        args["B"] = leaves["Bw"][..., :m]
        assert not args["A"].is_contiguous() and not args["B"].is_contiguous()
        _compare(args, leaves, n, m, N, batch, gz)
        # an incoming gradient that is a column slice of a wider tensor
        leaves = _leaves(ndlqr, n, m, N, batch, 2300)
        wide = torch.randn((batch, nv(n, m, N) + 7), dtype=torch.float64, device="cuda")
        gzs = wide[:, 3:3 + nv(n, m, N)]
        assert not gzs.is_contiguous()
        _compare(leaves, leaves, n, m, N, batch, gzs)
    elif case == "horizons":
        for n, m, N, batch, shared in ((6, 3, 16, 1, ()), (4, 2, 2, 3, ()), (4, 2, 2, 3, ("A", "B")),
                                       (3, 2, 64, 2, ()), (3, 2, 64, 2, ("A", "Q"))):
            gz = torch.randn((batch, nv(n, m, N)), dtype=torch.float64, device="cuda")
            leaves = _leaves(ndlqr, n, m, N, batch, 2400, shared=shared)
            _compare(leaves, leaves, n, m, N, batch, gz)
    elif case == "large_shared_A":
        n, m, N, batch = 144, 16, 4, 2
        gz = torch.randn((batch, nv(n, m, N)), dtype=torch.float64, device="cuda")
        leaves = _leaves(ndlqr, n, m, N, batch, 2500, shared=("A",))
        _compare(leaves, leaves, n, m, N, batch, gz)
    else:
        raise ValueError(case)
