"""Infeasibility detection of the solve with linear inequality constraints on the device
(ndlqr_BatchSetConstraintInfeasibilityDetection, ndlqr_CopyBatchConstraintInfeasibilityCertificate / Measures; DESIGN.md
section 3.20) against lin_infeas_support.py: the long-double certificate test from the problem data alone and the float64
restatement of the iteration with the test. Batch 3 -- problem 1 infeasible, problems 0 and 2 its feasible twins --, the
instances of lin_infeas_support.instance (family A "travelling" on every shape, family B "local" on two), rho = 1,
alpha = 1.6, eps_abs = eps_rel = 1e-6, a check every 10 iterations with eps = 1e-4; default mode everywhere, strict mode
on (6,3,5) and (12,4,8)."""
import numpy as np
import pytest

import cost_support as cs
import lin_grad_support as lg
import lin_infeas_support as li
import lin_support as ls
from test_gpu_lin import REL_TOL, constrained_solver

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
SET = dict(rho=li.RHO, alpha=li.ALPHA, eps_abs=li.EPS_ABS, eps_rel=li.EPS_REL)
STRICT_CASES = [(6, 3, 5), (12, 4, 8)]
CASES = [("A",) + c for c in sorted(li.CHOICE_A)] + [("B",) + c for c in sorted(li.CHOICE_B)]
BAD, TWINS = 1, (0, 2)


def modes(ndlqr, n, m, N):
    return [0, ndlqr.FLAG_STRICT_FP] if (n, m, N) in STRICT_CASES else [0]


def detecting_solver(ndlqr, inst, flags=0, every=li.EVERY, eps=li.EPS):
    bs = constrained_solver(ndlqr, inst, flags)
    bs.set_constraint_infeasibility(every, eps)
    return bs


def state(bs, iters, status):
    return dict(iters=iters, status=status, Z=bs.solutions(), v=bs.constraint_reduction()["v"], mu=bs.constraint_multipliers())


def check_dynamics(c, z):
    """the dynamics rows of a delivered z to the parity contract: 1e-9 of the largest state"""
    p = c["p"]
    n, m, N = cs.dims(p)
    _, x, u = cs.split(z.astype(LD), n, m, N)
    dyn = [np.abs(x[0] - p["x0"]).max()]
    for k in range(N - 1):
        dyn.append(np.abs(x[k + 1] - (p["A"][k] @ x[k] + p["B"][k] @ u[k] + p["d"][k])).max())
    assert float(max(dyn)) <= REL_TOL * float(np.abs(x).max()), (float(max(dyn)), float(np.abs(x).max()))


def check_certificate(c, dlam, dmu, eps=2 * li.EPS):
    chk = li.farkas_check_rows(c["p"], c["C"], c["D"], c["lo"], c["hi"], dlam, dmu, eps)
    assert chk["ok"], chk
    return chk


# ---------------------------------------------------------------------------- 1: the certificate
@pytest.mark.parametrize("fam,n,m,N", CASES)
def test_infeasible_member_is_certified_and_the_batch_stops_early(ndlqr, fam, n, m, N):
    inst = li.instance(n, m, N, fam)
    ref = [c["ref"] for c in inst]
    assert [r["status"] for r in ref] == [1, 4, 1]
    for flags in modes(ndlqr, n, m, N):
        bs = detecting_solver(ndlqr, inst, flags)
        iters, status = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
        on = state(bs, iters, status)
        dlam, dmu = bs.constraint_infeasibility_certificate()
        meas, at = bs.constraint_infeasibility_measures()
        bs.close()
        print("certify", fam, (n, m, N), "flags", flags, "device", list(iters), list(status), "| restatement",
              [r["iters"] for r in ref], [r["status"] for r in ref], "| measures of the certified",
              ["%.3e" % x for x in meas[BAD]], "at", at[BAD])
        assert list(status) == [1, 4, 1], (iters, status)
        assert abs(int(iters[BAD]) - ref[BAD]["iters"]) <= li.EVERY and iters[BAD] % li.EVERY == 0, (iters, ref[BAD]["iters"])
        assert iters.max() < li.MAX_ITER  # (every member frozen: the host stopped at its next look at the count)
        chk = check_certificate(inst[BAD], dlam[BAD], dmu[BAD])
        # the measures are those of the certifying check, and they are the certificate's own numbers
        assert at[BAD] == iters[BAD]
        assert meas[BAD][1] == float(chk["dmu_inf"]) and meas[BAD][2] == float(chk["inf_max"])
        assert abs(meas[BAD][0] - float(chk["e_inf"])) <= (n + dmu.shape[2] + 2) * EPS * float(chk["e_scale"])
        assert abs(LD(meas[BAD][3]) - chk["S"]) <= 4 * EPS * EPS * chk["S_scale"] + EPS * abs(chk["S"])
        for i in TWINS:
            assert not dlam[i].any() and not dmu[i].any()
        check_dynamics(inst[BAD], on["Z"][BAD])
        # without detection the infeasible member holds the batch to max_iter; the twins deliver the same bits
        bs = constrained_solver(ndlqr, inst, flags)
        iters, status = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
        off = state(bs, iters, status)
        bs.close()
        assert list(off["status"]) == [1, 2, 1] and off["iters"][BAD] == li.MAX_ITER
        for i in TWINS:
            assert on["iters"][i] == off["iters"][i]
            for k in ("Z", "v", "mu"):
                assert np.array_equal(on[k][i], off[k][i]), (i, k)


# ---------------------------------------------------------------------------- 2: off is off
def test_off_is_off(ndlqr):
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    for flags in modes(ndlqr, n, m, N):
        fresh = constrained_solver(ndlqr, inst, flags)
        want = state(fresh, *fresh.solve_constrained(max_iter=300, **SET))
        fresh.close()
        bs = detecting_solver(ndlqr, inst, flags)
        _, status = bs.solve_constrained(max_iter=300, **SET)
        assert status[BAD] == 4
        bs.constraint_infeasibility_certificate()
        bs.set_constraint_infeasibility(0)
        got = state(bs, *bs.solve_constrained(max_iter=300, **SET))
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert got["status"][BAD] == 2
        for read in (bs.constraint_infeasibility_certificate, bs.constraint_infeasibility_measures):
            with pytest.raises(RuntimeError, match="ndlqr_hip_download_constraint_infeasibility_.*not that of a constrained solve "
                                                   "with infeasibility detection on"):
                read()
        bs.close()


# ---------------------------------------------------------------------------- 3: a frozen status-4 problem
@pytest.mark.parametrize("fam,n,m,N", [("A", 6, 3, 5), ("B", 7, 9, 16)])
def test_certified_problem_delivers_one_z_however_long_the_batch_goes_on(ndlqr, fam, n, m, N):
    """eps_abs = eps_rel = 1e-300 (0 would mean the default): the twins never converge and the batch runs to max_iter; the infeasible member's trajectory
    does not depend on the tolerances."""
    inst = li.instance(n, m, N, fam)
    for flags in modes(ndlqr, n, m, N):
        out = []
        bs = detecting_solver(ndlqr, inst, flags)
        it0 = int(bs.solve_constrained(max_iter=li.MAX_ITER, **SET)[0][BAD])
        for further in (10, 200):
            iters, status = bs.solve_constrained(max_iter=it0 + further, **dict(SET, eps_abs=1e-300, eps_rel=1e-300))
            assert list(status) == [2, 4, 2] and iters[BAD] == it0, (iters, status)
            out.append((bs.solutions()[BAD], bs.constraint_multipliers()[BAD], bs.constraint_infeasibility_certificate()))
        bs.close()
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        assert np.array_equal(out[0][2][0], out[1][2][0]) and np.array_equal(out[0][2][1], out[1][2][1])
        check_dynamics(inst[BAD], out[0][0])


# ---------------------------------------------------------------------------- 4: with the adaptive penalty
@pytest.mark.parametrize("every,adapt", [(7, 25), (25, 25)])
@pytest.mark.parametrize("fam,n,m,N", [("A", 6, 3, 5), ("A", 12, 4, 8), ("B", 7, 9, 16)])
def test_certificates_pass_with_the_adaptive_penalty(ndlqr, fam, n, m, N, every, adapt):
    """Check period 7 against adapt period 25 (coprime), and 25 against 25: every check is an adapt iteration, and a
    problem may be certified behind the update that moved its penalty. Whatever the penalties did, a problem reported as 4
    carries a certificate that passes the long-double test, its delivered z satisfies the dynamics, and no twin is
    ever reported as 4."""
    inst = li.instance(n, m, N, fam)
    for flags in modes(ndlqr, n, m, N):
        bs = detecting_solver(ndlqr, inst, flags, every=every)
        bs.set_constraint_adaptation(adapt)
        iters, status = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
        Z, rho = bs.solutions(), bs.constraint_penalties()
        dlam, dmu = bs.constraint_infeasibility_certificate()
        meas, at = bs.constraint_infeasibility_measures()
        bs.close()
        print("adaptive", fam, (n, m, N), "flags", flags, "check", every, "adapt", adapt, "device", list(iters), list(status),
              "rho", list(rho), "measures", ["%.3e" % x for x in meas[BAD]], "at", at[BAD])
        assert list(status) == [1, 4, 1], (iters, status)
        assert iters[BAD] % every == 0 and iters.max() < li.MAX_ITER
        check_certificate(inst[BAD], dlam[BAD], dmu[BAD])
        check_dynamics(inst[BAD], Z[BAD])
        for i in TWINS:
            assert not dlam[i].any() and not dmu[i].any()
            check_dynamics(inst[i], Z[i])


def test_batch_that_ends_with_a_certificate_behind_a_move(ndlqr):
    """Tolerance 1e-3: the twins converge early, and the infeasible member is certified behind an update that also moved
    its penalty (checks and adapt iterations coincide) -- the last event of the batch. The move stands: the batch is
    factored for it and re-solved once more, so the delivered z belongs to the records in force, and the remembered
    factorisation serves the adjoint and a warm start afterwards."""
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    kw = dict(SET, eps_abs=1e-3, eps_rel=1e-3)
    G = np.stack([lg.seeded_g(n, m, N, i) for i in range(cs.BATCH)])
    for flags in modes(ndlqr, n, m, N):
        bs = detecting_solver(ndlqr, inst, flags, every=25)
        bs.set_constraint_adaptation(25)
        iters, status = bs.solve_constrained(max_iter=li.MAX_ITER, **kw)
        it0 = int(iters[BAD])
        Z, rho = bs.solutions(), bs.constraint_penalties()
        dlam, dmu = bs.constraint_infeasibility_certificate()
        assert list(status) == [1, 4, 1] and it0 == iters.max() and it0 % 25 == 0, (iters, status)
        check_certificate(inst[BAD], dlam[BAD], dmu[BAD])
        check_dynamics(inst[BAD], Z[BAD])
        # the adjoint takes the remembered factorisation up; the certified member is not iterated
        _, astatus = bs.solve_constrained_adjoint(G, max_iter=2000, alpha=li.ALPHA, eps_abs=1e-8, eps_rel=1e-8)
        assert astatus[BAD] == 3 and not bs.adjoint()[BAD].any()
        # ... and so does a warm start (the infeasible member cold, from the penalty it ended with)
        iters_w, status_w = bs.solve_constrained(max_iter=li.MAX_ITER, warm_start=True, **kw)
        assert status_w[0] == 1 and status_w[2] == 1 and status_w[BAD] in (2, 4), (iters_w, status_w)
        check_dynamics(inst[BAD], bs.solutions()[BAD])
        if status_w[BAD] == 4:
            d2 = bs.constraint_infeasibility_certificate()
            check_certificate(inst[BAD], d2[0][BAD], d2[1][BAD])
        bs.close()
        # stopped at it0 by max_iter, no move is considered at it0 (it < max_iter): the penalty before the move
        bs = detecting_solver(ndlqr, inst, flags, every=25)
        bs.set_constraint_adaptation(25)
        iters_b, status_b = bs.solve_constrained(max_iter=it0, **kw)
        rho_before = bs.constraint_penalties()
        bs.close()
        print("certificate behind a move", "flags", flags, list(iters), list(status), "rho", list(rho), "rho before", list(rho_before))
        assert status_b[BAD] == 4 and iters_b[BAD] == it0 and rho[BAD] != rho_before[BAD], (rho, rho_before)


# ---------------------------------------------------------------------------- 5: the kept lambda
@pytest.mark.parametrize("fam,n,m,N", [("A", 6, 3, 5), ("A", 7, 9, 16)])
def test_kept_lambda_is_the_delivered_one(ndlqr, fam, n, m, N):
    """The differences a check at `it` judges are those of the iterates two cold solves stopped at it - 1 and it deliver
    (solutions(): lambda in the caller's variables; constraint_multipliers(): mu = rho y): the measures' D and
    infinite-side maximum bit for bit, ||e||_inf within (n + p + 2) eps x the largest sum of absolute terms of an entry
    (its fma chain), S within 4 eps^2 sum |terms| + eps |S| (the two-term accumulator, rounded once)."""
    inst = li.instance(n, m, N, fam)
    for flags in modes(ndlqr, n, m, N):
        bs = constrained_solver(ndlqr, inst, flags)
        li.check_kept_lambda(bs, inst, 2 * li.EVERY, li.EVERY, li.EPS, SET, ("kept lambda", (n, m, N), "flags", flags))
        bs.close()


# ---------------------------------------------------------------------------- 6: warm start after status 4
def test_warm_start_after_status_4_starts_cold(ndlqr):
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    for flags in modes(ndlqr, n, m, N):
        bs = detecting_solver(ndlqr, inst, flags)
        cold = state(bs, *bs.solve_constrained(max_iter=li.MAX_ITER, **SET))
        cert = bs.constraint_infeasibility_certificate()
        assert list(cold["status"]) == [1, 4, 1]
        warm = state(bs, *bs.solve_constrained(max_iter=li.MAX_ITER, warm_start=True, **SET))
        cert_w = bs.constraint_infeasibility_certificate()
        bs.close()
        assert list(warm["status"]) == [1, 4, 1] and warm["iters"][BAD] == cold["iters"][BAD]
        assert (warm["iters"][list(TWINS)] < cold["iters"][list(TWINS)]).all()  # (the twins did start warm)
        for k in ("Z", "v", "mu"):
            assert np.array_equal(warm[k][BAD], cold[k][BAD]), k
        assert np.array_equal(cert_w[0], cert[0]) and np.array_equal(cert_w[1], cert[1])


# ---------------------------------------------------------------------------- 7: adjoint and gradients
def test_adjoint_and_gradients_of_a_certified_problem_are_zero(ndlqr):
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    # the same batch with the infeasible member's rows replaced by its feasible twin's: problems 0 and 2 are the same
    rows = li.family_a(inst[BAD]["p"], feasible=True, **li.CHOICE_A[(n, m, N)])
    feasible = [inst[0], dict(inst[BAD], C=rows[0], D=rows[1], lo=rows[2], hi=rows[3]), inst[2]]
    G = np.stack([lg.seeded_g(n, m, N, i) for i in range(cs.BATCH)])
    kw = dict(max_iter=3000, alpha=li.ALPHA, eps_abs=1e-8, eps_rel=1e-8)
    for flags in modes(ndlqr, n, m, N):
        out = []
        for cases in (inst, feasible):
            bs = detecting_solver(ndlqr, cases, flags)
            _, fstatus = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
            iters, status = bs.solve_constrained_adjoint(G, **kw)
            out.append(dict(fstatus=fstatus, iters=iters, status=status, W=bs.adjoint(), nu=bs.constraint_adjoint_multipliers(),
                            g=bs.constraint_gradients(), gs=bs.constraint_gradients(summed=True)))
            bs.close()
        bad, good = out
        assert list(bad["fstatus"]) == [1, 4, 1] and list(good["fstatus"]) == [1, 1, 1]
        assert bad["status"][BAD] == 3 and bad["iters"][BAD] == 0  # (carried like a forward 3: not iterated)
        assert not bad["W"][BAD].any() and not bad["nu"][BAD].any()
        for k in ("C", "D", "lo", "hi"):
            assert not bad["g"][k][BAD].any(), k
            for i in TWINS:
                assert np.array_equal(bad["g"][k][i], good["g"][k][i]), (k, i)
            assert np.abs(bad["gs"][k] - (bad["g"][k][0] + bad["g"][k][2])).max() <= 4 * EPS * np.abs(bad["g"][k]).max()
        for i in TWINS:
            assert bad["status"][i] == good["status"][i] and bad["iters"][i] == good["iters"][i] > 0
            assert np.array_equal(bad["W"][i], good["W"][i]) and np.array_equal(bad["nu"][i], good["nu"][i])


def test_torch_returns_zeros_for_a_certified_problem():
    _run_child("_case_torch")


def _run_child(name, *args):
    """test_gpu_lin_gradients._run_case for a case of this module: torch's HIP runtime has to be the first in its process"""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import rslqr_amd, test_gpu_lin_infeas as T\n"
            "T.%s(rslqr_amd, *json.loads(%r))\n"
            "print('case ok')\n" % (os.path.dirname(here), here, name, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "case ok" in r.stdout, (name, args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _case_torch(ndlqr):
    import torch
    from rslqr_amd.autograd import _lin_cache, lqr_solve_constrained
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    names = cs.NAMES + ("C", "D", "lo", "hi")
    arr = {k: np.stack([c["p"][k] for c in inst]) for k in cs.NAMES}
    arr.update({k: np.stack([c[k] for c in inst]) for k in ("C", "D", "lo", "hi")})
    t = {k: torch.tensor(np.ascontiguousarray(arr[k]), dtype=torch.float64, device="cuda", requires_grad=True) for k in names}
    gz = torch.tensor(np.stack([lg.seeded_g(n, m, N, i) for i in range(cs.BATCH)]), dtype=torch.float64, device="cuda")
    kw = dict(rho=li.RHO, alpha=li.ALPHA, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000)
    with pytest.raises(RuntimeError, match="did not converge"):  # (without detection the infeasible member ends as 2)
        lqr_solve_constrained(*[t[k] for k in names], **kw)
    z = lqr_solve_constrained(*[t[k] for k in names], infeas_every=li.EVERY, infeas_eps=0.0, **kw)
    (z * gz).sum().backward()
    (bs, _), = _lin_cache.values()
    _, at = bs.constraint_infeasibility_measures()
    print("certified at", at[BAD])
    assert at[BAD] > 0 and torch.isfinite(z).all()
    for k in names:
        g = t[k].grad
        assert g is not None and g.shape == t[k].shape, k
        assert not g[BAD].any(), k
        assert torch.isfinite(g).all() and g[0].any() == g[2].any(), k
    assert t["q"].grad[0].any() and t["C"].grad[0].any()
    # infeas_every = 0 on the same cached solver switches it off again
    with pytest.raises(RuntimeError, match="did not converge"):
        lqr_solve_constrained(*[t[k] for k in names], **kw)


# ---------------------------------------------------------------------------- 8: NaN data
def test_nan_data_ends_as_3_never_4(ndlqr):
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    # q of knot 0 reaches lambda_0 alone (x_0 is fixed): the update's maxima never see that NaN, the check does
    for where, at, want in (("q", (3, 2), 3), ("d", (1, 0), 3), ("x0", (0,), 3), ("q", (0, 0), 2)):
        cases = [dict(c) for c in inst]
        p = {k: v.copy() for k, v in cases[BAD]["p"].items()}
        p[where][at] = np.nan
        cases[BAD]["p"] = p
        for flags in modes(ndlqr, n, m, N):
            # (a check at every iteration from the second on: the NaN meets the test as early as it can)
            bs = detecting_solver(ndlqr, cases, flags, every=1)
            iters, status = bs.solve_constrained(max_iter=400, **SET)
            dlam, dmu = bs.constraint_infeasibility_certificate()
            meas, _ = bs.constraint_infeasibility_measures()
            bs.close()
            print("NaN in", where, at, "flags", flags, list(iters), list(status), "measures", list(meas[BAD]))
            assert status[BAD] == want and status[0] == 1 and status[2] == 1, (where, at, iters, status)
            assert not dlam.any() and not dmu.any()
            if want == 2:  # (examined at every check, the NaN stored as it is)
                assert np.isnan(meas[BAD][0])


# ---------------------------------------------------------------------------- 9: the setting, refusals
def test_setting_and_refusals(ndlqr):
    n, m, N = 6, 3, 5
    inst = li.instance(n, m, N, "A")
    bs = ndlqr.BatchSolver(n, m, N, cs.BATCH)
    bs.set_constraint_infeasibility(li.EVERY)  # (allowed in any mode; eps = 0: 1e-4)
    for kw in (dict(every=-1), dict(every=5, eps=-1.0), dict(every=5, eps=np.nan), dict(every=5, eps=np.inf)):
        with pytest.raises(RuntimeError, match="ndlqr_BatchSetConstraintInfeasibilityDetection failed"):
            bs.set_constraint_infeasibility(**kw)
    for read in (bs.constraint_infeasibility_certificate, bs.constraint_infeasibility_measures):
        with pytest.raises(RuntimeError, match="ndlqr_hip_download_constraint_infeasibility_.*: the solver is not in constrained mode"):
            read()
    # the setting is the solver's: the refused calls left it, and the initialiser keeps it
    C, D, lo, hi = ls.flat_rows(inst)
    bs.initialize_flat_constrained(*cs.flat([c["p"] for c in inst]), C, D, lo, hi)
    stale = "ndlqr_hip_download_constraint_infeasibility_.*not that of a constrained solve with infeasibility detection on"
    with pytest.raises(RuntimeError, match=stale):  # (no solve yet)
        bs.constraint_infeasibility_certificate()
    iters, status = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
    assert list(status) == [1, 4, 1] and iters[BAD] % li.EVERY == 0
    dlam, dmu = bs.constraint_infeasibility_certificate()
    check_certificate(inst[BAD], dlam[BAD], dmu[BAD])
    # either output alone; not neither
    L = ndlqr.lib()
    only = np.zeros_like(dmu)
    assert L.ndlqr_CopyBatchConstraintInfeasibilityCertificate(bs.h, None, only.ctypes.data_as(ndlqr.api.dp)) == 0
    assert np.array_equal(only, dmu)
    assert L.ndlqr_CopyBatchConstraintInfeasibilityCertificate(bs.h, None, None) == ndlqr.api.ERR_INVALID
    assert L.ndlqr_CopyBatchConstraintInfeasibilityMeasures(bs.h, None, None) == ndlqr.api.ERR_INVALID
    # device memory of the solver's own device
    dev = ndlqr.DeviceArray(dlam.shape)
    bs.constraint_infeasibility_certificate(dlam=dev)
    assert np.array_equal(dev.get(), dlam)
    # the box solve's switch and read-outs stay refused in this mode
    with pytest.raises(RuntimeError, match="ndlqr_hip_set_box_infeasibility"):
        bs.set_box_infeasibility(10)
    with pytest.raises(RuntimeError, match="ndlqr_hip_download_infeasibility_certificate"):
        bs.infeasibility_certificate()
    # a plain solve in between drops the read-outs
    assert bs.solve() == 0
    for read in (bs.constraint_infeasibility_certificate, bs.constraint_infeasibility_measures):
        with pytest.raises(RuntimeError, match=stale):
            read()
    # another initialiser leaves constrained mode; the setting stays, and a padded horizon (N = 5) never refused it
    bs.initialize_flat_dense(*cs.flat([c["p"] for c in inst]))
    with pytest.raises(RuntimeError, match="the solver is not in constrained mode"):
        bs.constraint_infeasibility_measures()
    bs.initialize_flat_constrained(*cs.flat([c["p"] for c in inst]), C, D, lo, hi)
    _, status = bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
    assert list(status) == [1, 4, 1]
    bs.close()
    # the memory of another device: this one assertion needs a second GPU and is NOT exercised on a box with one MI355X
    if ndlqr.device_count() >= 2:
        import torch

        class Foreign:
            def __init__(self, a):
                self.t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:1")
                self.ptr, self.size = self.t.data_ptr(), self.t.numel()
        bs = detecting_solver(ndlqr, inst)
        bs.solve_constrained(max_iter=li.MAX_ITER, **SET)
        other = Foreign(dlam)
        with pytest.raises(RuntimeError, match="ndlqr_hip_download_constraint_infeasibility_certificate: an output lies in the "
                                               "memory of another device"):
            bs.constraint_infeasibility_certificate(dlam=other)
        bs.close()
