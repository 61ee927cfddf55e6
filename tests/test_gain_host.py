"""The convention of the feedback gains and cost-to-go matrices (ndlqr_BatchFeedbackGains), pinned
without a GPU: the longdouble gains of gain_support.gains() against the refined solution of the dense KKT system
(cost_support.dense_kkt + refined_solve), which knows nothing of a Riccati recursion. On the optimal trajectory
u_k = K_k x_k + k_k and lambda_k = P_k x_k + p_k in the signs of the solution vector [lambda x u]:
max_k |u_k - (K_k x_k + k_k)| / max|u| and max_k |lambda_k - (P_k x_k + p_k)| / max|lambda| are each <= 1e-13 (the refined
solution carries a few eps; the largest value seen over these cases was 9.4e-16)."""
import numpy as np
import pytest

import cost_support as cs
import gain_support as gs

TOL = 1e-13
SEEDS = (0, 1, 2)


def problems(n, m, N, kind):
    if kind == "diagonal":
        return [cs.diagonal_problem(n, m, N, 500 + 13 * s)[0] for s in SEEDS]
    return [cs.dense_problem(n, m, N, 1e3, 700 + 17 * s) for s in SEEDS]


@pytest.mark.parametrize("kind", ["diagonal", "dense"])
@pytest.mark.parametrize("N", gs.HORIZONS)
@pytest.mark.parametrize("n,m", gs.SHAPES)
def test_gains_reproduce_the_kkt_solution(n, m, N, kind):
    for p in problems(n, m, N, kind):
        g = gs.gains(p, np.longdouble)
        z = cs.refined_solve(*cs.dense_kkt(p))
        eu, el = gs.closed_loop_errors(g, z, n, m, N)
        print("closed loop", (n, m, N), kind, "u %.2e lambda %.2e" % (eu, el))
        assert eu <= TOL and el <= TOL, (eu, el)
        assert np.array_equal(g["P"], g["P"].transpose(0, 2, 1))
        assert not g["K"][N - 1].any() and not g["k"][N - 1].any()
        assert np.array_equal(g["P"][N - 1], p["Q"][N - 1].astype(np.longdouble)) and np.array_equal(g["p"][N - 1], p["q"][N - 1])


@pytest.mark.parametrize("n,m,N", [(6, 3, 5), (7, 9, 8), (12, 4, 16)])
def test_the_two_float64_restatements_agree_with_the_longdouble_one(n, m, N):
    """gains() in float64 and the reduce / unit-cost / map-back restatement of dense-cost mode both follow the longdouble
    gains to a small multiple of eps times cond: the yardsticks of the device tests are restatements of the same thing."""
    for p in problems(n, m, N, "dense"):
        exact = gs.gains(p, np.longdouble)
        for f64 in (gs.gains(p, np.float64), gs.gains_reduced(p)):
            for k in gs.NAMES:
                assert f64[k].dtype == np.float64
                err = float(np.abs(f64[k] - exact[k]).max()) / float(np.abs(exact[k]).max())
                assert err <= 1e-10, (k, err)
