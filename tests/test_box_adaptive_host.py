"""Host-side checks of the per-problem adaptive penalty of the box-constrained solve: the new
entry points exist and refuse bad arguments without a device, and the numpy restatement of the rule, driven by the
oracle on the families of test_box_host.py, meets the same references as the fixed-penalty restatement in fewer
iterations (CPU only)."""
import ctypes as C

import numpy as np
import pytest

from box_adaptive_support import admm_adaptive_reference, penalty_step
from box_support import active_set_qp, admm_reference, bvls_inputs, certificate, split
from test_box_host import _input_box, synth

ADAPT_EVERY = 25


def test_new_entry_points_refuse_without_a_solver(ndlqr):
    L = ndlqr.lib()
    for name in ("ndlqr_CopyBatchBoxPenalties", "ndlqr_hip_solve_box_ex", "ndlqr_hip_download_box_penalties"):
        assert name in ndlqr.exported_symbols()
    rho = np.zeros(4)
    dp = rho.ctypes.data_as(C.POINTER(C.c_double))
    assert L.ndlqr_CopyBatchBoxPenalties(None, dp) == ndlqr.api.ERR_INVALID
    L.ndlqr_hip_download_box_penalties.restype = C.c_int
    L.ndlqr_hip_download_box_penalties.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    assert L.ndlqr_hip_download_box_penalties(None, dp) == ndlqr.api.ERR_INVALID
    L.ndlqr_hip_solve_box_ex.restype = C.c_int
    L.ndlqr_hip_solve_box_ex.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p] * 2 + \
        [C.c_int, C.c_double, C.c_double]
    assert L.ndlqr_hip_solve_box_ex(None, 0.1, 1.6, 1e-6, 1e-6, 10, 5, 0, None, None, 5, 1e-6, 1e6) == ndlqr.api.ERR_INVALID


def test_settings_struct_and_invalid_settings(ndlqr):
    S = ndlqr.NdLqrBoxSettingsFull  # the C struct: the seven fields of NdLqrBoxSettings, then the three new ones
    assert [f[0] for f in S._fields_] == [f[0] for f in ndlqr.NdLqrBoxSettings._fields_] + ["adapt_every", "rho_min", "rho_max"]
    assert C.sizeof(S) == 4 * 8 + 4 * 4 + 2 * 8
    assert S.adapt_every.offset == 44 and S.rho_min.offset == 48 and S.rho_max.offset == 56
    assert all(getattr(S, f[0]).offset == getattr(ndlqr.NdLqrBoxSettings, f[0]).offset for f in ndlqr.NdLqrBoxSettings._fields_)
    st = S(0.5, 1.6, 1e-6, 1e-6, 100, 10, 1)  # the positional construction of the seven earlier fields
    assert st.warm_start == 1 and st.adapt_every == 0 and st.rho_min == 0.0 and st.rho_max == 0.0
    # (without a solver every call is refused; test_gpu_box_adaptive.py sends the same settings to a real one)
    L = ndlqr.lib()
    for bad in (S(0.0, 0.0, 0.0, 0.0, 0, 0, 0, -1, 0.0, 0.0), S(0.0, 0.0, 0.0, 0.0, 0, 0, 0, 5, 2.0, 1.0)):
        assert L.ndlqr_SolveBatchBoxConstrained(None, C.byref(bad), None, None) == ndlqr.api.ERR_INVALID
    # the shorter struct never reaches the C side, which reads ten fields
    short = ndlqr.NdLqrBoxSettings(0.5, 1.6, 1e-6, 1e-6, 100, 10, 1)
    with pytest.raises(C.ArgumentError):
        L.ndlqr_SolveBatchBoxConstrained(None, C.byref(short), None, None)


def test_penalty_step_is_a_clamped_power_of_two():
    assert penalty_step(1.0, 1.0, 1.0, 1.0, 1.0) == 1.0
    assert penalty_step(1.0, 3.9, 1.0, 1.0, 1.0) == 1.0          # ratio below 4: nothing moves
    assert penalty_step(1.0, 4.0, 1.0, 1.0, 1.0) == 2.0
    assert penalty_step(1.0, 1.0, 4.0, 1.0, 1.0) == 0.5
    assert penalty_step(1.0, 1.0, 7.9, 1.0, 1.0) == 0.5          # e = -2 -> k = -1
    assert penalty_step(1.0, 1.0, 8.0, 1.0, 1.0) == 0.5          # e = -3 -> k = -1 (toward zero)
    assert penalty_step(3.0, 2.0 ** 40, 1.0, 1.0, 1.0) == 3.0 * 64  # clamp of the step
    assert penalty_step(3.0, 2.0 ** 40, 1.0, 1.0, 1.0, 1e-6, 100.0) == 100.0  # clamp of rho
    assert penalty_step(1.0, 0.0, 1.0, 1.0, 1.0) == 1.0 and penalty_step(1.0, 1.0, 1.0, 1.0, float("inf")) == 1.0


def test_adaptive_restatement_with_the_oracle_meets_the_references_in_fewer_iterations(ndlqr, oracle):
    """The families and tolerances of test_box_host's fixed-penalty restatement, from rho = mean diag R: input bounds reach
    the bvls solution, state and input bounds pass the certificate and match the active-set QP; the iterations over the
    family add up to fewer than the fixed penalty's."""
    n, m, N = 4, 2, 16
    prob = synth(ndlqr, n, m, N, 7)
    solve = lambda p: oracle.solve(p, 1)[0][: p.nvars]
    rho = float(prob.R.mean())
    ulo, uhi, _ = _input_box(oracle, prob, 0.5)
    inf = np.full((N, n), np.inf)
    total, total_fixed = 0, 0
    x, u, mux, muu, lam, it, st, rho_end, changes = admm_adaptive_reference(prob, solve, -inf, inf, ulo, uhi, rho, 1.6, 1e-10,
                                                                           1e-10, 5000, ADAPT_EVERY)
    print("input bounds: adaptive %d iterations, %d changes, rho %g -> %g" % (it, changes, rho, rho_end))
    assert st == 1, it
    total += it
    fixed = admm_reference(prob, solve, -inf, inf, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000)
    print("input bounds: fixed %d iterations" % fixed[5])
    total_fixed += fixed[5]
    ub, _ = bvls_inputs(prob, ulo, uhi)
    assert np.linalg.norm(u[: N - 1] - ub) <= 1e-6 * np.linalg.norm(ub), it
    assert (u[: N - 1] <= uhi[: N - 1]).all() and (u[: N - 1] >= ulo[: N - 1]).all()
    # state bounds as well: clip x at 60 % of its unconstrained range
    z0 = solve(prob)
    x0 = split(z0, n, m, N)[1]
    xhi = np.tile(0.6 * np.abs(x0[1:]).max(axis=0), (N, 1))
    xlo = -xhi
    x, u, mux, muu, lam, it, st, rho_end, changes = admm_adaptive_reference(prob, solve, xlo, xhi, ulo, uhi, rho, 1.6, 1e-10,
                                                                           1e-10, 5000, ADAPT_EVERY)
    print("state + input bounds: adaptive %d iterations, %d changes, rho %g -> %g" % (it, changes, rho, rho_end))
    assert st == 1, it
    total += it
    fixed = admm_reference(prob, solve, xlo, xhi, ulo, uhi, rho, 1.6, 1e-10, 1e-10, 5000)
    print("state + input bounds: fixed %d iterations" % fixed[5])
    total_fixed += fixed[5]
    z = np.concatenate([lam, x, u], axis=1).reshape(-1)[: prob.nvars]
    cert = certificate(prob, z, mux, muu, xlo, xhi, ulo, uhi, 1e-7)
    assert cert["stationarity"] <= 1e-7 and cert["bounds"] <= 0 and cert["complementarity"] <= 1e-7, cert
    ua, xa, na = active_set_qp(prob, xlo, xhi, ulo, uhi, x, u, mux, muu, 1e-7)
    assert na > 0
    assert np.linalg.norm(u[: N - 1] - ua) <= 1e-6 * np.linalg.norm(ua)
    assert total < total_fixed, (total, total_fixed)


def test_period_zero_is_the_fixed_restatement(ndlqr, oracle):
    n, m, N = 4, 2, 16
    prob = synth(ndlqr, n, m, N, 7)
    solve = lambda p: oracle.solve(p, 1)[0][: p.nvars]
    ulo, uhi, _ = _input_box(oracle, prob, 0.5)
    inf = np.full((N, n), np.inf)
    a = admm_adaptive_reference(prob, solve, -inf, inf, ulo, uhi, 0.37, 1.6, 1e-8, 1e-8, 400, 0)
    b = admm_reference(prob, solve, -inf, inf, ulo, uhi, 0.37, 1.6, 1e-8, 1e-8, 400)
    assert all(np.array_equal(p, q) for p, q in zip(a[:7], b)) and a[7] == 0.37 and a[8] == 0
