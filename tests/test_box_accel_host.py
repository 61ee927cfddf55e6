"""Host-side checks of the Anderson acceleration of the box-constrained solve (ndlqr_BatchSetBoxAcceleration; DESIGN.md
section 3.15): the entry points exist and refuse bad arguments without a device; the numpy restatement of the rule
(box_accel_support.admm_accel_reference) with the memory off is box_support.admm_reference, and with it on it meets the
references of test_box_host.py in fewer iterations; the sensitivity of the restatement to the order of its sums, which
fixes the tolerance of the device comparison (CPU only)."""
import ctypes as C

import numpy as np
import pytest

from box_accel_support import admm_accel_reference, cholesky_solve
from box_support import active_set_qp, admm_reference, bvls_inputs, certificate, masks, split
from support import Problem

ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
MEM = 5

# The tolerance of the 12-iteration device comparison (tests/test_gpu_box_accel.py): 100 x the largest relative
# difference in [v, mu] between two 12-iteration runs of the restatement at (12,4,16), memory 5, that differ only in the
# order of their dot products (test_sensitivity_to_the_summation_order, which recomputes it and holds it below this).
# Measured: 7.75e-15 (problem seeds 80, 81 of test_gpu_box.py's strict case, per-problem and shared bounds, one
# permutation each); 100 x that, rounded up to one digit:
GPU_TOLERANCE_12 = 8e-13


def synth(ndlqr, n, m, N, seed):
    g = ndlqr.generate_synthetic(n, m, N, seed)
    return Problem(n, m, N, *[g[k] for k in ARGS])


def test_entry_points_refuse_without_a_solver(ndlqr):
    L = ndlqr.lib()
    for name in ("ndlqr_BatchSetBoxAcceleration", "ndlqr_CopyBatchBoxAcceleration", "ndlqr_hip_set_box_acceleration",
                 "ndlqr_hip_download_box_acceleration"):
        assert name in ndlqr.exported_symbols() and hasattr(L, name), name
    INVALID = ndlqr.api.ERR_INVALID
    ints = np.zeros(4, dtype=np.int32)
    ip = ints.ctypes.data_as(C.POINTER(C.c_int))
    assert L.ndlqr_BatchSetBoxAcceleration(None, 5, 0.0, 0.0) == INVALID
    assert L.ndlqr_CopyBatchBoxAcceleration(None, ip, None, None, None) == INVALID
    L.ndlqr_hip_set_box_acceleration.restype = C.c_int
    L.ndlqr_hip_set_box_acceleration.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    L.ndlqr_hip_download_box_acceleration.restype = C.c_int
    L.ndlqr_hip_download_box_acceleration.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    assert L.ndlqr_hip_set_box_acceleration(None, 5, 1.0, 1e-10) == INVALID
    assert L.ndlqr_hip_download_box_acceleration(None, ints.ctypes.data, None, None, None) == INVALID
    assert C.sizeof(ndlqr.NdLqrBoxSettings) == 4 * 8 + 3 * 4 + 4  # (the setting lives on the solver: the struct keeps its size)


def test_cholesky_solve():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 6))
    A = B.T @ B
    b = rng.standard_normal(6)
    x = cholesky_solve(A.tolist(), b.tolist(), 6)
    assert np.abs(np.array(x) - np.linalg.solve(A, b)).max() <= 1e-12 * np.abs(x).max()
    assert cholesky_solve([[0.0]], [1.0], 1) is None                      # dG = 0
    assert cholesky_solve([[1.0, 1.0], [1.0, 1.0]], [1.0, 1.0], 2) is None  # singular: the second pivot is 0
    assert cholesky_solve([[float("nan")]], [1.0], 1) is None


def _family(ndlqr, oracle):
    """the (4,2,16) problem and bounds of test_box_host.py: input bounds at 0.5 of the largest unconstrained |u|, state
    bounds at 0.6 of the largest unconstrained |x|"""
    n, m, N = 4, 2, 16
    prob = synth(ndlqr, n, m, N, 7)
    solve = lambda p: oracle.solve(p, 1)[0][: p.nvars]
    _, x0, u0 = split(solve(prob), n, m, N)
    uhi = np.tile(0.5 * np.abs(u0).max(axis=0), (N, 1))
    xhi = np.tile(0.6 * np.abs(x0[1:]).max(axis=0), (N, 1))
    inf = np.full((N, n), np.inf)
    return prob, solve, {"u": (-inf, inf, -uhi, uhi), "xu": (-xhi, xhi, -uhi, uhi)}


def test_memory_zero_is_the_plain_restatement(ndlqr, oracle):
    prob, solve, bounds = _family(ndlqr, oracle)
    rho = float(prob.R.mean())
    for b, iters in ((bounds["u"], 5000), (bounds["xu"], 40)):
        ref = admm_reference(prob, solve, *b, rho, 1.6, 1e-10, 1e-10, iters)
        got = admm_accel_reference(prob, solve, *b, rho, 1.6, 1e-10, 1e-10, iters, mem=0)
        assert got.accepted == 0 and got.rejected == 0
        for a, r in zip(got.plain, ref):
            assert np.array_equal(a, r)


@pytest.mark.parametrize("which", ["R", "Q"])
def test_accelerated_restatement_meets_the_references_in_fewer_iterations(ndlqr, oracle, which):
    """as test_box_host.py's test of the plain restatement, at its tolerances: bvls for input bounds, the certificate and
    the active-set QP for state and input bounds; the iterations summed over the family are fewer than the plain ones"""
    prob, solve, bounds = _family(ndlqr, oracle)
    n, m, N = prob.n, prob.m, prob.N
    rho = float((prob.R if which == "R" else prob.Q).mean())
    total = {0: 0, MEM: 0}
    for mem in (0, MEM):
        xlo, xhi, ulo, uhi = bounds["u"]
        a = admm_accel_reference(prob, solve, xlo, xhi, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000, mem=mem)
        assert a.status == 1, a.iters
        ub, _ = bvls_inputs(prob, ulo, uhi)
        assert np.linalg.norm(a.u[: N - 1] - ub) <= 1e-6 * np.linalg.norm(ub), a.iters
        assert (a.u[: N - 1] <= uhi[: N - 1]).all() and (a.u[: N - 1] >= ulo[: N - 1]).all()
        total[mem] += a.iters
        xlo, xhi, ulo, uhi = bounds["xu"]
        a = admm_accel_reference(prob, solve, xlo, xhi, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000, mem=mem)
        assert a.status == 1, a.iters
        z = np.concatenate([a.lam, a.x, a.u], axis=1).reshape(-1)[: prob.nvars]
        cert = certificate(prob, z, a.mu_x, a.mu_u, xlo, xhi, ulo, uhi, 1e-7)
        assert cert["stationarity"] <= 1e-7 and cert["bounds"] <= 0 and cert["complementarity"] <= 1e-7, cert
        ua, xa, na = active_set_qp(prob, xlo, xhi, ulo, uhi, a.x, a.u, a.mu_x, a.mu_u, 1e-7)
        assert na > 0
        assert np.linalg.norm(a.u[: N - 1] - ua) <= 1e-6 * np.linalg.norm(ua)
        total[mem] += a.iters
        if mem:
            assert a.accepted > 0
    print("iterations over the family at rho = mean diag %s: plain %d, accelerated %d" % (which, total[0], total[MEM]))
    assert total[MEM] < total[0], total


def sensitivity_cases(ndlqr, oracle):
    """the problems and bounds of the device's 12-iteration comparison: (12,4,16) x 2, per-problem and shared bounds"""
    from test_gpu_box import input_box, state_box
    n, m, N = 12, 4, 16
    probs = [synth(ndlqr, n, m, N, 80 + p) for p in range(2)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    per = [(xlo[p], xhi[p], ulo[p], uhi[p]) for p in range(2)]
    shared = [(xlo[0], xhi[0], ulo[0], uhi[0])] * 2
    return probs, per, shared


def test_sensitivity_to_the_summation_order(ndlqr, oracle):
    """12 iterations at memory 5, natural against permuted order of the dot products: the largest relative difference in
    v and mu, x 100, is the device tolerance recorded above. Above 1e-9 the regularisation would be too weak."""
    probs, per, shared = sensitivity_cases(ndlqr, oracle)
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    rng = np.random.default_rng(12)
    worst = 0.0
    for bounds in (per, shared):
        for prob, b in zip(probs, bounds):
            run = lambda perm: admm_accel_reference(prob, solve, *b, 0.37, 1.6, 1e-300, 1e-300, 12, mem=MEM, perm=perm)
            a = run(None)
            assert a.iters == 12 and a.status == 2 and a.accepted >= 6, (a.iters, a.status, a.accepted)
            va, ma = np.concatenate([a.x, a.u], axis=1), np.concatenate([a.mu_x, a.mu_u], axis=1)
            Mx, Mu = masks(prob.n, prob.m, prob.N, *b)
            count = int(Mx.sum() + Mu.sum())
            p = run(rng.permutation(count))
            assert (p.accepted, p.rejected, p.columns) == (a.accepted, a.rejected, a.columns)
            vp, mp = np.concatenate([p.x, p.u], axis=1), np.concatenate([p.mu_x, p.mu_u], axis=1)
            worst = max(worst, np.abs(vp - va).max() / np.abs(va).max(), np.abs(mp - ma).max() / np.abs(ma).max())
    print("largest relative difference between summation orders: %.3g" % worst)
    assert worst > 0.0  # (the permutation reaches the sums)
    assert 100.0 * worst <= GPU_TOLERANCE_12, worst
    assert GPU_TOLERANCE_12 <= 1e-9
