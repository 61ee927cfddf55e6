"""Host-side checks of the infeasibility detection of the solve with linear inequality constraints (DESIGN.md section
3.20): the long-double certificate test of lin_infeas_support.py on hand-made certificates and against
box_infeas_support.farkas_check on selector rows, the numpy restatement of the iteration with the test on the instances
the GPU tests use, and the new entry points (CPU only)."""
import ctypes as C

import numpy as np
import pytest

import box_infeas_support as bis
import cost_support as cs
import lin_infeas_support as li
import lin_support as ls
import rslqr_amd
from support import Problem

A_CASES = sorted(li.CHOICE_A)
B_CASES = sorted(li.CHOICE_B)


def test_farkas_check_rows_accepts_a_hand_made_certificate_and_rejects_each_sign_flip():
    """Family B at knot 2 of a (4,2,4) problem: a'x <= -1 and a'x >= 1. dlam = 0, dmu = (t, -t) on the two rows: e = a (t - t)
    = 0 and S = (-1) t + (1)(-t) = -2 t."""
    n, m, N, knot, t = 4, 2, 4, 2, 0.75
    p = cs.dense_problem(n, m, N, 1e3, 5)
    C_, D_, lo, hi = li.family_b(p, knot, 2, feasible=False)
    dlam = np.zeros((N, n))
    dmu = np.zeros((N, 2))
    dmu[knot] = (t, -t)
    c = li.farkas_check_rows(p, C_, D_, lo, hi, dlam, dmu, 1e-4)
    assert c["ok"] and c["e_inf"] == 0 and c["inf_max"] == 0 and c["dmu_inf"] == t and abs(c["S"] + 2 * t) <= 1e-18, c
    assert li.farkas_check_rows(p, C_, D_, lo, hi, dlam, 7 * dmu, 1e-4)["ok"]  # (any positive multiple is one too)
    for flip, stationary in (((-t, -t), False), ((t, t), False), ((-t, t), True)):
        bad = dmu.copy()
        bad[knot] = flip
        c = li.farkas_check_rows(p, C_, D_, lo, hi, dlam, bad, 1e-4)
        assert not c["ok"] and c["stationary"] == stationary and not c["qualified"], (flip, c)
    # a lambda difference alone breaks e = 0
    c = li.farkas_check_rows(p, C_, D_, lo, hi, dlam + 1e-3, dmu, 1e-4)
    assert not c["ok"] and not c["stationary"], c
    # the same differences against the feasible twin's band [t0 - 1.5, t0 - 0.5]: S = t (t0 - 0.5) - t (t0 - 1.5) = +t
    K, b = cs.dense_kkt(p)
    C2, D2, lo2, hi2 = li.family_b(p, knot, 2, feasible=True, z_free=cs.refined_solve(K, b))
    c = li.farkas_check_rows(p, C2, D2, lo2, hi2, dlam, dmu, 1e-4)
    assert not c["ok"] and c["stationary"] and not c["negative"] and abs(c["S"] - t) <= 1e-15, c
    assert not li.farkas_check_rows(p, C_, D_, lo, hi, dlam, 0 * dmu, 1e-4)["nonzero"]
    # a NaN anywhere certifies nothing
    for where in ("dlam", "dmu"):
        d1, d2 = dlam.copy(), dmu.copy()
        (d1 if where == "dlam" else d2)[0, 0] = np.nan
        assert not li.farkas_check_rows(p, C_, D_, lo, hi, d1, d2, 1e-4)["ok"]


def test_farkas_check_rows_rejects_a_large_entry_toward_an_infinite_bound():
    """The certificate of the test above plus an entry on a row without bounds (C = 0 there, so e stays 0): stationary,
    negative -- and not qualified, unless the entry is within eps ||dmu||_inf."""
    n, m, N, knot, t = 4, 2, 4, 2, 0.75
    p = cs.dense_problem(n, m, N, 1e3, 5)
    C_, D_, lo, hi = li.family_b(p, knot, 2, feasible=False)
    dlam = np.zeros((N, n))
    dmu = np.zeros((N, 2))
    dmu[knot] = (t, -t)
    dmu[1, 0] = 0.1
    c = li.farkas_check_rows(p, C_, D_, lo, hi, dlam, dmu, 1e-4)
    assert not c["ok"] and c["stationary"] and c["negative"] and c["nonzero"] and not c["qualified"] and c["inf_max"] == np.longdouble(0.1), c
    dmu[1, 0] = 0.5e-4 * t
    c = li.farkas_check_rows(p, C_, D_, lo, hi, dlam, dmu, 1e-4)
    assert c["ok"] and c["inf_max"] == np.longdouble(0.5e-4 * t), c
    # the one-sided rows themselves, each toward its infinite side
    for r, v in ((0, -0.1), (1, 0.1)):
        bad = np.zeros((N, 2))
        bad[knot] = (t, -t)
        bad[knot, r] += v - bad[knot, r]
        assert not li.farkas_check_rows(p, C_, D_, lo, hi, dlam, bad, 1e-4)["qualified"]


@pytest.mark.parametrize("n,m,N,knot", [(3, 2, 4, 2), (6, 3, 5, 4)])
def test_selector_rows_give_the_numbers_of_the_box_check(n, m, N, knot):
    g = rslqr_amd.generate_synthetic(n, m, N, 11)
    prob = Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])
    p, _, _ = cs.diagonal_problem(n, m, N, 11)
    rng = np.random.default_rng([n, m, N])
    for infeasible in (True, False):
        bounds = (bis.infeasible_bounds if infeasible else bis.barely_feasible_bounds)(prob, 0.4, knot, 0.25)
        rows = ls.selector_rows(n, m, N, *bounds)
        for trial in range(4):
            dlam = rng.standard_normal((N, n))
            dmu_x = rng.standard_normal((N, n)) * (rng.random((N, n)) < 0.5)
            dmu_u = rng.standard_normal((N, m)) * 1e-5 ** (trial % 2)  # (small ones pass the qualification)
            dmu_u[N - 1] = 0  # (an entry the box solve never bounds and whose e the row solve does not form)
            if trial >= 2:
                dmu_x[:] = 0
                dmu_x[knot, 0] = 1.0
            want = bis.farkas_check(prob, bounds, dlam, dmu_x, dmu_u, 1e-4)
            got = li.farkas_check_rows(p, *rows, dlam, np.concatenate([dmu_x, dmu_u], axis=1), 1e-4)
            for k in ("nonzero", "stationary", "qualified", "negative", "ok"):
                assert got[k] == want[k], (k, got, want)
            assert float(got["dmu_inf"]) == want["dmu_inf"]
            assert abs(float(got["e_inf"]) - want["e_inf"]) <= 4 * np.finfo(float).eps * float(got["e_scale"])
            assert abs(float(got["S"]) - want["S"]) <= 4 * np.finfo(float).eps * float(got["S_scale"])


@pytest.mark.parametrize("fam,n,m,N", [("A",) + c for c in A_CASES] + [("B",) + c for c in B_CASES])
def test_restatement_certifies_the_infeasible_member_and_converges_on_its_twins(fam, n, m, N):
    inst = li.instance(n, m, N, fam)
    refs = [c["ref"] for c in inst]
    print("family", fam, (n, m, N), (li.CHOICE_A if fam == "A" else li.CHOICE_B)[(n, m, N)], "status", [r["status"] for r in refs],
          "iterations", [r["iters"] for r in refs])
    assert [r["status"] for r in refs] == [1, 4, 1], [(r["status"], r["iters"]) for r in refs]
    r, c = refs[1], inst[1]
    assert r["iters"] % li.EVERY == 0 and r["iters"] <= li.MAX_ITER
    chk = li.farkas_check_rows(c["p"], c["C"], c["D"], c["lo"], c["hi"], r["dlam"], r["dmu"], li.EPS)
    assert chk["ok"], chk
    for t in (refs[0], refs[2]):
        assert not t["dlam"].any() and not t["dmu"].any()
    if fam == "B":  # the local certificate: dmu = (t, -t') on the two rows, each toward its finite side, and no other row
        knot = li.CHOICE_B[(n, m, N)]["knot"]
        d = r["dmu"][knot]
        assert d[0] > 0 and d[1] < 0 and not np.delete(r["dmu"], knot, axis=0).any()
    else:  # the dense row toward its upper bound, and input rows on the way back to x0
        knot = li.CHOICE_A[(n, m, N)]["knot"]
        assert r["dmu"][knot, m] > 0 and np.abs(r["dmu"][:knot, :m]).max() > 0 and np.abs(r["dlam"][0]).max() > 0


def test_new_entry_points_exist_and_refuse_without_a_solver(ndlqr):
    L = ndlqr.lib()
    names = ("ndlqr_BatchSetConstraintInfeasibilityDetection", "ndlqr_CopyBatchConstraintInfeasibilityCertificate",
             "ndlqr_CopyBatchConstraintInfeasibilityMeasures", "ndlqr_hip_set_constraint_infeasibility",
             "ndlqr_hip_download_constraint_infeasibility_certificate", "ndlqr_hip_download_constraint_infeasibility_measures")
    for name in names:
        assert name in ndlqr.exported_symbols()
        assert hasattr(L, name)
    INVALID = ndlqr.api.ERR_INVALID
    # (no device here, so no solver: every call is refused; test_gpu_lin_infeas.py sends the same arguments to a real one)
    assert L.ndlqr_BatchSetConstraintInfeasibilityDetection(None, -1, 0.0) == INVALID
    assert L.ndlqr_BatchSetConstraintInfeasibilityDetection(None, 10, float("nan")) == INVALID
    assert L.ndlqr_BatchSetConstraintInfeasibilityDetection(None, 10, 1e-4) == INVALID
    buf = np.zeros(4)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    ints = np.zeros(4, dtype=np.int32)
    ip = ints.ctypes.data_as(C.POINTER(C.c_int))
    assert L.ndlqr_CopyBatchConstraintInfeasibilityCertificate(None, dp, dp) == INVALID
    assert L.ndlqr_CopyBatchConstraintInfeasibilityMeasures(None, dp, ip) == INVALID
    L.ndlqr_hip_set_constraint_infeasibility.restype = C.c_int
    L.ndlqr_hip_set_constraint_infeasibility.argtypes = [C.c_void_p, C.c_int, C.c_double]
    assert L.ndlqr_hip_set_constraint_infeasibility(None, 10, 1e-4) == INVALID
    L.ndlqr_hip_download_constraint_infeasibility_certificate.restype = C.c_int
    L.ndlqr_hip_download_constraint_infeasibility_certificate.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 2
    assert L.ndlqr_hip_download_constraint_infeasibility_certificate(None, dp, dp) == INVALID
    L.ndlqr_hip_download_constraint_infeasibility_measures.restype = C.c_int
    L.ndlqr_hip_download_constraint_infeasibility_measures.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    assert L.ndlqr_hip_download_constraint_infeasibility_measures(None, dp, ip) == INVALID
