"""Host checks of the references behind the dense-cost tests (cost_support.py): the restated
reduction is exact algebra, the generators keep what they claim, and the library exports the new entry point."""
import numpy as np
import pytest

import rslqr_amd
import cost_support as cs

SHAPES = [(6, 3, 5), (12, 4, 16), (7, 9, 12), (20, 5, 8)]
EPS = np.finfo(float).eps


def _bar(p):
    """Forward-error bound of the reduction in float64: Q' = Q - W W' is a cancellation, so Q' -- and with it L, the
    scaling of every x and lambda -- carries a relative perturbation of eps |Q_k| |Q'_k^-1| (R_k: eps cond(R_k)); a
    factor 8 for the triangular solves and products behind it."""
    n, m, N = cs.dims(p)
    worst = 1.0
    for k in range(N):
        Qp = p["Q"][k] - (p["H"][k] @ np.linalg.solve(p["R"][k], p["H"][k].T) if k < N - 1 else 0.0)
        worst = max(worst, np.linalg.norm(p["Q"][k], 2) * np.linalg.norm(np.linalg.inv(Qp), 2), np.linalg.cond(p["R"][k]))
    return 8 * EPS * worst


def _reduced_solve(p, g=None):
    """S K~^-1 S' g (g None: the problem's own right-hand side), everything in float64"""
    red = cs.reduce(p)
    Kt, bt = cs.dense_kkt(cs.reduced_problem(red))
    rhs = bt if g is None else cs.apply_St(red, g)
    return cs.apply_S(red, np.linalg.solve(Kt, rhs))


@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", SHAPES)
def test_reduction_reproduces_the_dense_solution(n, m, N, name):
    p = cs.dense_problem(n, m, N, cs.FAMILIES[name], 11)
    K, b = cs.dense_kkt(p)
    err = cs.field_errors(_reduced_solve(p), cs.refined_solve(K, b), n, m, N)
    print("solution", (n, m, N), name, err)
    print("bar", _bar(p))
    assert max(err) <= _bar(p), err


@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m,N", SHAPES)
def test_adjoint_through_the_reduction(n, m, N, name):
    p = cs.dense_problem(n, m, N, cs.FAMILIES[name], 12)
    K, _ = cs.dense_kkt(p)
    g = np.random.default_rng(5).standard_normal(K.shape[0])
    err = cs.field_errors(_reduced_solve(p, g), cs.refined_solve(K, g), n, m, N)
    print("adjoint", (n, m, N), name, err)
    print("bar", _bar(p))
    assert max(err) <= _bar(p), err


def test_reduced_right_hand_side_is_St_b():
    p = cs.dense_problem(6, 3, 5, 1e3, 3)
    red = cs.reduce(p, np.longdouble)
    _, b = cs.dense_kkt(p)
    _, bt = cs.dense_kkt(cs.reduced_problem(red))
    assert np.abs(cs.apply_St(red, b.astype(np.longdouble)) - bt).max() <= 64 * np.finfo(float).eps * np.abs(bt).max()


@pytest.mark.parametrize("name", ["moderate", "hard"])
@pytest.mark.parametrize("n,m", cs.SHAPES)
def test_generators_keep_their_condition_numbers(n, m, name):
    cond = cs.FAMILIES[name]
    p = cs.dense_problem(n, m, 5, cond, 21)
    ld = np.longdouble
    for k in range(5):
        R = p["R"][k]
        assert np.array_equal(R, R.T) and np.array_equal(p["Q"][k], p["Q"][k].T)
        assert abs(np.linalg.cond(R) / cond - 1) <= 1e-6, (k, np.linalg.cond(R))
        if k < 4:
            Qp = (p["Q"][k].astype(ld) - p["H"][k].astype(ld) @ np.linalg.solve(R, p["H"][k].T).astype(ld)).astype(float)
        else:
            Qp = p["Q"][k]
        ev = np.linalg.eigvalsh(0.5 * (Qp + Qp.T))
        # (Q' is formed by a cancellation of relative size |H R^-1 H'| / lambda_min(Q') eps ~ 1e-9 in the hard family)
        assert ev[0] > 0 and abs(ev[-1] / ev[0] / cond - 1) <= 1e-5, (k, ev[-1] / ev[0])


def test_diagonal_problem_is_the_generators():
    p, Qd, Rd = cs.diagonal_problem(6, 3, 5, 2)
    assert np.array_equal(np.stack([np.diag(v) for v in p["Q"]]), Qd) and not p["H"].any()
    assert np.array_equal(np.stack([np.diag(v) for v in p["R"]]), Rd)


def test_dense_entry_points_are_exported():
    names = rslqr_amd.exported_symbols()
    for s in ("ndlqr_InitializeBatchFlatDense", "ndlqr_BatchCostIsDense", "ndlqr_hip_download_cost_reduction"):
        assert s in names, s
        assert hasattr(rslqr_amd.lib(), s), s
