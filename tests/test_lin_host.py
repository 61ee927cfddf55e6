"""The restatement of the solve with linear inequality constraints (lin_support.admm) against
what it must satisfy, on the CPU: a converged restatement satisfies the KKT conditions of the constrained QP, and with
rows that select single entries it reproduces the box restatement box_support.admm_reference."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import box_support as bs
import cost_support as cs
import lin_support as ls
import rslqr_amd
from box_grad_support import kkt_sparse
from support import Problem

SHAPES = [(6, 3, 2), (6, 3, 5), (12, 4, 8), (7, 9, 5), (20, 5, 16)]


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_converged_restatement_satisfies_kkt(n, m, N):
    """K z - b + G' mu = 0, feasibility, sign and complementarity of mu, to the bars lin_support.kkt_bar derives from the
    residual row; in float64 and, on the smallest shape, in longdouble."""
    seen = 0
    for c in ls.case(n, m, N):
        runs = [c["ref"]]
        if (n, m, N) == SHAPES[0]:
            runs.append(ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], dtype=np.longdouble))
        for r in runs:
            if r["status"] != 1:
                continue  # (a seed ADMM does not converge at rho = 1: the status tests run those)
            seen += 1
            bar = ls.kkt_bar(c["p"], c["C"], c["D"], r["z"], r["resid"])
            got = ls.kkt_violation(c["p"], c["C"], c["D"], c["lo"], c["hi"], r["z"], r["mu"], bar["tol"])
            print((n, m, N), r["iters"], got, bar)
            assert got["stationarity"] <= bar["stationarity"]
            assert got["feasibility"] <= bar["feasibility"]
            assert got["complementarity"] == 0.0
            active = np.abs(np.asarray(r["mu"], dtype=np.float64)) > 0
            assert active.any(), "no constraint is active: the case checks nothing"
    assert seen > 0


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (12, 4, 8)])
def test_selector_rows_reproduce_the_box_restatement(n, m, N):
    """Rows that select every x and u entry on a diagonal cost: the iterates v, y of the first iterations, the iteration
    count and the solution agree with box_support.admm_reference (same rho, alpha, eps; the same dense solver class).
    Bar: 8 x the float64 restatement's own distance from the longdouble one after three iterations, at least 16 eps of the
    field's largest entry."""
    p, Qd, Rd = cs.diagonal_problem(n, m, N, 41)
    g = rslqr_amd.generate_synthetic(n, m, N, 41)
    prob = Problem(n, m, N, g["A"], g["B"], g["Q"], g["R"], g["q"], g["r"], g["d"], g["x0"])
    K, b = cs.dense_kkt(p)
    _, x, u = cs.split(cs.refined_solve(K, b), n, m, N)
    # (state bounds at 0.6 of the unconstrained range are infeasible on these seeds: inputs at 0.6, states at 0.9)
    xhi = 0.9 * np.abs(x).max(axis=0) * np.ones((N, n)); uhi = 0.6 * np.abs(u).max(axis=0) * np.ones((N, m))
    C, D, lo, hi = ls.selector_rows(n, m, N, -xhi, xhi, -uhi, uhi)

    def solve(q):
        Ks, bq = kkt_sparse(q)
        return spla.splu(Ks.tocsc()).solve(bq)

    rho, alpha, eps = 1.0, 1.6, 1e-8
    tb, tl, tld = [], [], []
    xb, ub, mux, muu, lam, itb, stb = bs.admm_reference(prob, solve, -xhi, xhi, -uhi, uhi, rho, alpha, eps, eps, 2000, trace=tb)
    rl = ls.admm(p, C, D, lo, hi, rho, alpha, eps, eps, 2000, trace=tl)
    ls.admm(p, C, D, lo, hi, rho, alpha, eps, eps, 3, dtype=np.longdouble, trace=tld)
    eps64 = np.finfo(np.float64).eps
    for k in range(3):
        for name in ("v", "y"):
            ref = tld[k][name]
            own = float(np.abs(tl[k][name] - ref).max())
            bar = max(8 * own, 16 * eps64 * float(np.abs(ref).max()))
            err = float(np.abs(tb[k][name] - ref).max())
            print(name, k + 1, err, own, bar)
            assert err <= bar
    assert stb == rl["status"] == 1
    assert abs(itb - rl["iters"]) <= 2
    _, xl, ul = cs.split(np.asarray(rl["z"]), n, m, N)
    M = np.isfinite(lo) | np.isfinite(hi)
    vx, vu = rl["v"][:, :n], rl["v"][:, n:]
    tol = eps * (1 + max(np.abs(xb).max(), np.abs(ub).max())) * 4
    assert np.abs(np.where(M[:, :n], vx, xl) - xb).max() <= tol
    assert np.abs(np.where(M[:, n:], vu, ul)[: N - 1] - ub[: N - 1]).max() <= tol
