"""Host-side checks of the infeasibility detection of the box-constrained solve: the
long-double certificate test of box_infeas_support.py on a hand-made certificate, the numpy restatement of the iteration
with the test, driven by the oracle on a double integrator, and the new entry points (CPU only)."""
import ctypes as C

import numpy as np

from box_infeas_support import admm_infeas_reference, barely_feasible_bounds, farkas_check, infeasible_bounds
from support import Problem


def test_farkas_check_accepts_a_hand_made_certificate_and_rejects_a_flipped_sign():
    """x1 = a x0 + b u0 + d with |u0| <= 1 and x1 <= (a x0 + d - |b|) - gap. With dmu_x1 = 1 the rows e = 0 give
    dlam_1 = 1, dlam_0 = a, dmu_u0 = -b, and S = -gap."""
    a, b, d, x0, gap = 0.9, 0.5, 0.3, 2.0, 0.25
    prob = Problem(1, 1, 2, [a, 0.0], [b, 0.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [d, 0.0], [x0])
    xlo, xhi, ulo, uhi = infeasible_bounds(prob, 1.0, 1, gap)
    assert xhi[1][0] == (a * x0 + d - b) - gap
    dlam = np.array([[a], [1.0]])
    dmu_x = np.array([[0.0], [1.0]])
    dmu_u = np.array([[-b], [0.0]])
    c = farkas_check(prob, (xlo, xhi, ulo, uhi), dlam, dmu_x, dmu_u, 1e-4)
    assert c["ok"] and c["e_inf"] <= 1e-15 and abs(c["S"] + gap) <= 1e-15, c
    # any positive multiple is one too; the negative of it is none
    assert farkas_check(prob, (xlo, xhi, ulo, uhi), 7 * dlam, 7 * dmu_x, 7 * dmu_u, 1e-4)["ok"]
    c = farkas_check(prob, (xlo, xhi, ulo, uhi), dlam, -dmu_x, dmu_u, 1e-4)  # one sign flipped: e != 0, and it points to -inf
    assert not c["ok"] and not c["stationary"] and not c["qualified"], c
    c = farkas_check(prob, (xlo, xhi, ulo, uhi), -dlam, -dmu_x, -dmu_u, 1e-4)
    assert not c["ok"] and c["stationary"] and not c["qualified"], c
    # the same differences against the feasible bounds: S = +gap
    c = farkas_check(prob, barely_feasible_bounds(prob, 1.0, 1, gap), dlam, dmu_x, dmu_u, 1e-4)
    assert not c["ok"] and c["stationary"] and not c["negative"] and abs(c["S"] - gap) <= 1e-15, c
    assert not farkas_check(prob, (xlo, xhi, ulo, uhi), 0 * dlam, 0 * dmu_x, 0 * dmu_u, 1e-4)["nonzero"]


def double_integrator(N=8, dt=0.5):
    A = np.array([[1.0, dt], [0.0, 1.0]])
    B = np.array([[0.5 * dt * dt], [dt]])
    tile = lambda a: np.tile(np.asarray(a, dtype=float).T.reshape(-1), (N, 1))  # column-major storage
    return Problem(2, 1, N, tile(A), tile(B), np.ones((N, 2)), np.full((N, 1), 0.1), np.zeros((N, 2)), np.zeros((N, 1)),
                   np.zeros((N, 2)), [1.0, 0.0])


def test_reference_certifies_the_infeasible_double_integrator_and_converges_on_the_feasible_one(oracle):
    prob = double_integrator()
    solve = lambda p: oracle.solve(p, 1)[0][: p.nvars]
    knot, ubar, gap = prob.N - 1, 0.2, 0.1
    bounds = infeasible_bounds(prob, ubar, knot, gap)
    st, it, dlam, dmu_x, dmu_u = admm_infeas_reference(prob, solve, *bounds, 1.0, 1.6, 1e-6, 1e-6, 2000, 10)
    print("infeasible: status %d at iteration %d" % (st, it))
    assert st == 4 and it % 10 == 0, (st, it)
    c = farkas_check(prob, bounds, dlam, dmu_x, dmu_u, 1e-4)
    assert c["ok"], c
    assert dmu_x[knot][0] > 0 and (np.delete(dmu_x.reshape(-1), knot * prob.n) == 0).all()  # the one bounded state, toward hi
    st, it, dlam, dmu_x, dmu_u = admm_infeas_reference(prob, solve, *barely_feasible_bounds(prob, ubar, knot, gap), 1.0, 1.6,
                                                       1e-6, 1e-6, 2000, 10)
    print("barely feasible: status %d at iteration %d" % (st, it))
    assert st == 1 and not dlam.any() and not dmu_x.any() and not dmu_u.any(), (st, it)


def test_new_entry_points_exist_and_refuse_bad_arguments(ndlqr):
    L = ndlqr.lib()
    names = ("ndlqr_BatchSetInfeasibilityDetection", "ndlqr_CopyBatchInfeasibilityCertificate",
             "ndlqr_hip_set_box_infeasibility", "ndlqr_hip_download_infeasibility_certificate")
    for name in names:
        assert name in ndlqr.exported_symbols()
        assert hasattr(L, name)
    INVALID = ndlqr.api.ERR_INVALID
    # (no device here, so no solver: every call is refused; test_gpu_box_infeas.py sends the same arguments to a real one)
    assert L.ndlqr_BatchSetInfeasibilityDetection(None, -1, 0.0) == INVALID
    assert L.ndlqr_BatchSetInfeasibilityDetection(None, 10, float("nan")) == INVALID
    assert L.ndlqr_BatchSetInfeasibilityDetection(None, 10, 1e-4) == INVALID
    buf = np.zeros(4)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.ndlqr_CopyBatchInfeasibilityCertificate(None, dp, dp, dp) == INVALID
    L.ndlqr_hip_set_box_infeasibility.restype = C.c_int
    L.ndlqr_hip_set_box_infeasibility.argtypes = [C.c_void_p, C.c_int, C.c_double]
    assert L.ndlqr_hip_set_box_infeasibility(None, 10, 1e-4) == INVALID
    L.ndlqr_hip_download_infeasibility_certificate.restype = C.c_int
    L.ndlqr_hip_download_infeasibility_certificate.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    assert L.ndlqr_hip_download_infeasibility_certificate(None, dp, dp, dp) == INVALID
    # the settings struct keeps its size: the detection setting lives on the solver
    assert C.sizeof(ndlqr.NdLqrBoxSettingsFull) == 4 * 8 + 4 * 4 + 2 * 8
