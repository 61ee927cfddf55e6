"""The references of the objective read-out against each other, without a GPU: the optimal-value
identity pins the sign conventions, the last-knot rule and the packing; the reduced-variable identity is what lets the
diagonal kernel serve dense-cost mode; the envelope formulas are what lqr_value's backward applies."""
import numpy as np
import pytest

import cost_support as cs
import objective_support as osup
from support import Problem


@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 16), (7, 9, 4), (2, 1, 2)])
def test_optimal_value_identity(ndlqr, oracle, n, m, N):
    """J* = 1/2 [sum (q'x + r'u) + lam_0'x_init + sum lam_(k+1)'d_k] at the oracle's solution, to 1e-9 S"""
    for seed in (3, 4):
        p, Qd, Rd = cs.diagonal_problem(n, m, N, seed)
        col = lambda M: M.transpose(0, 2, 1).reshape(N, -1)
        prob = Problem(n, m, N, col(p["A"]), col(p["B"]), Qd, Rd, p["q"], p["r"], p["d"], p["x0"])
        soln, _, _, fails = oracle.solve(prob, 1)
        assert fails == 0
        z = soln[: prob.nvars]
        ex = osup.exact(p, z)
        lam, x, u = cs.split(z.astype(np.longdouble), n, m, N)
        ld = lambda a: np.asarray(a, dtype=np.longdouble)
        ident = 0.5 * ((ld(p["q"]) * x).sum() + (ld(p["r"][:N - 1]) * u[:N - 1]).sum() + lam[0] @ ld(p["x0"])
                       + (lam[1:] * ld(p["d"][:N - 1])).sum())
        assert abs(float(ident) - ex["J"]) <= 1e-9 * ex["S"], (float(ident), ex["J"], ex["S"])
        # the stage costs add up to J, and the last knot has no input terms
        assert abs(ex["ell"].sum() - ex["J"]) <= 4 * osup.EPS * ex["S"]
        other = {k: v.copy() for k, v in p.items()}
        for k in ("A", "B", "H", "R", "r", "d"):
            other[k][N - 1] = 7.0
        assert np.array_equal(osup.exact(other, z)["ell"], ex["ell"])


@pytest.mark.parametrize("kind", ["dense", "dense-noH"])
@pytest.mark.parametrize("N", [2, 5, 8])
@pytest.mark.parametrize("n,m", [(6, 3), (12, 4), (7, 9)])
def test_reduced_variable_identity(n, m, N, kind):
    """1/2 |xi|^2 + 1/2 |nu|^2 + q~'xi + r~'nu in float64 against the exact stage cost in the caller's variables: within
    max(8 x its own float64 error, 16 eps S). Its own error is measured against the identity evaluated in longdouble on
    the longdouble reduction, which separates an algebraic mismatch (an error of the size of S) from rounding."""
    probs = osup.families(n, m, N, kind)
    ref = cs.family(n, m, N, "moderate")
    for p, z in zip(probs, ref["z"]):
        # (z of the family with H also serves the family without: the identity holds at any point)
        ex = osup.exact(p, z)
        f64 = osup.reduced_f64(p, z)
        red = cs.reduce(p, np.longdouble)
        _, x, u = cs.split(np.asarray(z, dtype=np.longdouble), n, m, N)
        ell_ld = np.zeros(N, dtype=np.longdouble)
        for k in range(N):
            xi = red["L"][k].T @ x[k]
            ell_ld[k] = 0.5 * (xi @ xi) + red["qt"][k] @ xi
            if k < N - 1:
                nu = red["LR"][k].T @ (u[k] + red["G"][k] @ x[k])
                ell_ld[k] += 0.5 * (nu @ nu) + red["rt"][k] @ nu
        # the identity itself, in extended precision: far below the float64 bars
        assert np.all(np.abs(ell_ld.astype(np.float64) - ex["ell"]) <= 1e-12 * ex["S_k"] + 64 * osup.EPS * np.abs(ex["ell"])), (ell_ld, ex["ell"])
        own = np.abs(f64["ell"] - ell_ld.astype(np.float64))
        assert np.all(np.abs(f64["ell"] - ex["ell"]) <= np.maximum(8 * own, 16 * osup.EPS * ex["S_k"])), (f64["ell"], ex["ell"], ex["S_k"])
        ownJ = abs(f64["J"] - float(ell_ld.sum()))
        assert abs(f64["J"] - ex["J"]) <= max(8 * ownJ, 16 * osup.EPS * ex["S"]), (f64["J"], ex["J"], ex["S"])


def _torch_problem(probs, dense):
    import torch
    names = cs.NAMES if dense else ("A", "B", "Q", "R", "q", "r", "d", "x0")
    out = {}
    for k in names:
        a = np.stack([p[k] for p in probs])
        if not dense and k in ("Q", "R"):
            a = np.stack([np.stack([np.diag(M) for M in p[k]]) for p in probs])
        out[k] = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    return out


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n,m,N", [(3, 2, 4), (4, 2, 5)])
def test_envelope_formulas(n, m, N, dense):
    """dJ*/dtheta = the partial derivative of the Lagrangian, against torch double autograd through the dense KKT solve:
    1e-9 x the array's max-abs; the never-read last-knot entries exactly zero; the torch restatement that lqr_value's
    backward applies gives the same as the numpy one"""
    import torch
    from rslqr_amd.autograd import value_gradients
    probs = osup.families(n, m, N, "dense" if dense else "diagonal", 2)
    t = _torch_problem(probs, dense)
    J, z = osup.kkt_value_torch(t, n, m, N, dense)
    names = list(t)
    auto = dict(zip(names, torch.autograd.grad(J.sum(), [t[k] for k in names])))
    vg = dict(zip(names, value_gradients(z.detach(), n, m, N, dense)))
    for b in range(len(probs)):
        env = osup.envelope(z[b].detach().numpy(), n, m, N, dense)
        assert set(env) == set(names)
        for k in names:
            ref = auto[k][b].numpy()
            tol = 1e-9 * np.abs(ref).max()
            assert np.abs(env[k] - ref).max() <= tol, (k, env[k], ref)
            assert np.abs(vg[k][b].numpy() - ref).max() <= tol, (k, vg[k][b], ref)
            if k in ("A", "B", "H", "R", "r", "d"):
                assert not env[k][N - 1].any() and not vg[k][b, N - 1].numpy().any(), k
                assert not ref[N - 1].any(), k
