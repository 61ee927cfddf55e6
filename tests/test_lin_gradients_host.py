"""Gradients through the solve with linear inequality constraints, the parts that need no GPU:
the thirteen gradient formulas against central differences in longdouble, the convergence of the restated adjoint
iteration (lin_grad_support.adjoint_admm) to the direct active-set solve on the 44 cases whose forward converges, and
the box special case against box_grad_support.adjoint_admm_reference."""
import numpy as np
import scipy.sparse.linalg as spla

import box_grad_support as bg
import cost_support as cs
import lin_grad_support as lg
import lin_support as ls
from support import Problem

LD = np.longdouble


def test_entry_points_are_exported(ndlqr):
    L = ndlqr.lib()
    for name in ("ndlqr_SolveBatchLinAdjoint", "ndlqr_BatchConstraintGradients", "ndlqr_CopyBatchConstraintAdjointMultipliers",
                 "ndlqr_CopyBatchConstraintAdjointResiduals", "ndlqr_CopyBatchConstraintCodes"):
        assert name in ndlqr.exported_symbols() and hasattr(L, name), name
    # without a solver every one of them is an invalid call
    assert L.ndlqr_SolveBatchLinAdjoint(None, None, None, None, None) == -1
    assert L.ndlqr_BatchConstraintGradients(None, None, None, None, None, 0) == -1
    assert L.ndlqr_CopyBatchConstraintCodes(None, None) == -1


# ---------------------------------------------------------------------------- 1: the formulas by central differences
# Step. The loss g'z*(theta) is rational in theta: the central difference at h has a truncation error c h^2 and a
# rounding error dL / 2h, dL the error of the loss itself -- the longdouble solves leave about 100 eps_longdouble |L| =
# 1e-17 |L|. The bar has two parts. 4 |FD_h - FD_{h/2}| covers the truncation: the difference is 3/4 c h^2 and FD_{h/2}
# is c h^2 / 4 off, a twelfth of the bar, as long as h is small enough for the h^4 term not to matter. The floor, 16 eps
# of the gradient's largest entry, has to cover the rounding wherever the truncation is small or zero (the solution is
# linear in q, r, d, x0, lo, hi): dL / 2h <= 16 eps |G| asks for h >= 1e-17 |L| / (32 eps |G|) = 1.5e-3 |L| / |G|, and
# the loss is up to ten times the largest gradient entry here. h = 2^-6 is that, and still a fiftieth of the smallest
# cost eigenvalue scale of the family (condition 1e3 around 1): the printed ratios of the nonlinear arguments sit at the
# asymptotic 1/12.
H_STEP = 2.0 ** -6


def test_all_thirteen_gradient_formulas_by_central_differences():
    n, m, N = 6, 3, 5
    worst = {}
    for i, c in enumerate(lg.case(n, m, N)):
        assert c["ref"]["status"] == 1
        codes, g = c["codes"], c["g"].astype(LD)
        theta = {k: np.asarray(c["p"][k], dtype=LD).copy() for k in cs.NAMES}
        theta.update(C=c["C"].astype(LD), D=c["D"].astype(LD), lo=c["lo"].astype(LD), hi=c["hi"].astype(LD))

        def forward(t):
            p = {k: t[k] for k in cs.NAMES}
            _, b = ls.kkt_ld(p)
            cA = np.where(codes == 3, t["hi"], np.where(codes == 2, t["lo"], 0)).astype(LD)
            return lg.direct(p, t["C"], t["D"], codes, b, cA, LD)

        z, mu = forward(theta)
        w, nu = lg.direct({k: theta[k] for k in cs.NAMES}, theta["C"], theta["D"], codes, g, None, LD)
        grads = cs.gradient_reference(c["p"], z, w)
        grads.update(lg.constraint_grads(c["p"], codes, z, w, mu, nu))

        def fd(name, idx, h):
            out = []
            for sgn in (1, -1):
                t = dict(theta)
                t[name] = theta[name].copy()
                t[name][idx] += sgn * LD(h)
                out.append(g @ forward(t)[0])
            return (out[0] - out[1]) / (2 * LD(h))

        for name in list(cs.NAMES) + ["C", "D", "lo", "hi"]:
            G = np.asarray(grads[name], dtype=LD)
            floor = 16 * lg.EPS * float(np.abs(G).max())
            for idx in np.ndindex(theta[name].shape):
                if name in ("lo", "hi") and not np.isfinite(theta[name][idx]):
                    continue
                f1, f2 = fd(name, idx, H_STEP), fd(name, idx, H_STEP / 2)
                bar = 4 * float(abs(f1 - f2)) + floor
                err = float(abs(G[idx] - f2))
                worst[name] = max(worst.get(name, 0.0), err / bar if bar > 0 else (np.inf if err > 0 else 0.0))
                assert err <= bar, (i, name, idx, float(G[idx]), float(f2), err, bar)
    print("central differences, largest error / bar per argument:", {k: "%.3g" % v for k, v in worst.items()})


# ---------------------------------------------------------------------------- 2: the restated adjoint converges
def test_restated_adjoint_reaches_the_direct_solve():
    count, its, sv, mus, slack, rel = 0, [], [], [], [], []
    for (n, m, N) in lg.CASES:
        for i, c in enumerate(lg.case(n, m, N)):
            if lg.skipped(n, m, N, i):
                assert c["ref"]["status"] == 2, (n, m, N, i)
                continue
            assert c["ref"]["status"] == 1, (n, m, N, i)
            count += 1
            a = c["adj"]
            assert a["status"] == 1, (n, m, N, i, a["iters"])
            bar = lg.adjoint_bar(c, a["w"], a["resid"])
            err = float(np.abs(a["w"] - c["w_direct"]).max())
            assert err <= bar["w"], (n, m, N, i, err, bar)
            assert c["sv_ratio"] > 0
            its.append(a["iters"]); sv.append(c["sv_ratio"]); rel.append(err / float(np.abs(c["w_direct"]).max()))
            act = c["codes"] >= 2
            w = ls.rows_of(c["p"], c["C"], c["D"], c["ref"]["z"])
            mus.append(float(np.abs(c["ref"]["mu"][act]).min()) if act.any() else np.inf)
            free = c["codes"] == 1
            slack.append(float(np.minimum(w - c["lo"], c["hi"] - w)[free].min()) if free.any() else np.inf)
    print("adjoint restatement: %d cases, iterations %d .. %d, singular value ratio >= %.2e, |mu| on active rows >= %.2e, "
          "slack of inactive rows >= %.2e, |w - w_direct| / |w| <= %.2e" % (count, min(its), max(its), min(sv), min(mus),
                                                                            min(slack), max(rel)))
    assert count == 44
    assert min(sv) >= 1e-5  # (nonsingular active-set systems: measured 1.4e-5)
    assert min(mus) > 1e-6 and min(slack) > 1e-6  # (device and restatement see the same active set)


# ---------------------------------------------------------------------------- 3: the box special case
def test_selector_rows_reproduce_the_box_adjoint_reference():
    n, m, N = 6, 3, 5
    for i in range(cs.BATCH):
        p, Qd, Rd = cs.diagonal_problem(n, m, N, 41 + i)
        K, b = cs.dense_kkt(p)
        _, x, u = cs.split(cs.refined_solve(K, b), n, m, N)
        xhi = 0.9 * np.abs(x).max(axis=0) * np.ones((N, n)); uhi = 0.6 * np.abs(u).max(axis=0) * np.ones((N, m))
        C, D, lo, hi = ls.selector_rows(n, m, N, -xhi, xhi, -uhi, uhi)
        fwd = ls.admm(p, C, D, lo, hi)
        assert fwd["status"] == 1
        codes = lg.codes_of(fwd["v"], lo, hi)
        g = lg.seeded_g(n, m, N, i)
        mine = lg.adjoint_admm(p, C, D, lo, hi, codes, g)
        # the box reference on the diagonal problem
        col = lambda M: M.transpose(0, 2, 1).reshape(N, -1)
        prob = Problem(n, m, N, col(p["A"]), col(p["B"]), Qd, Rd, p["q"], p["r"], p["d"], p["x0"])
        Zf = np.zeros((N, 2 * n + m))
        Zf.reshape(-1)[: fwd["z"].size] = fwd["z"]
        Zf[:, n:] = np.where(codes > 0, fwd["v"], Zf[:, n:])  # (a box solution: x, u are the projected iterate)
        box_codes = bg.active_codes(prob, Zf.reshape(-1)[: fwd["z"].size], -xhi, xhi, -uhi, uhi)
        assert np.array_equal(box_codes, codes)
        solve = lambda pr: spla.spsolve(*bg.kkt_sparse(pr))
        w_box, nu_box, it_box, st_box = bg.adjoint_admm_reference(prob, solve, box_codes, g, ls.RHO, ls.ALPHA, 1e-8, 1e-8, 2000)
        assert st_box == 1 and mine["status"] == 1 and abs(it_box - mine["iters"]) <= 2, (it_box, mine["iters"])
        KK, _, _ = lg.bordered(p, C, D, codes)
        c = dict(p=p, C=C, D=D, inv_norm=float(np.abs(np.linalg.inv(KK)).sum(axis=1).max()))
        bar = lg.adjoint_bar(c, mine["w"], mine["resid"])["w"]
        ew, en = float(np.abs(mine["w"] - w_box).max()), float(np.abs(mine["nu"] - nu_box).max())
        print("selector rows", i, "iterations", mine["iters"], it_box, "|w - w_box| %.3e |nu - nu_box| %.3e bar %.3e" % (ew, en, bar))
        assert ew <= bar and en <= bar, (ew, en, bar)
