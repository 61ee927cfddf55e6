"""The two facts the dense-cost step (ndlqr_BatchStepAsyncDense) rests on, in numpy on
cost_support's restatement of the reduction -- no GPU:

- S is block diagonal over the knots: S restricted to a knot range equals the range of S applied to the whole vector, so a
  slice of the solution needs the z blocks and the records of its own knots alone (cost_deliver_slice);
- the reduced q depends on r, q~_k = L_k^-1 (q_k - G_k' r_k): replacing r alone changes q~, which is why a step replaces q
  and r together or neither (cost_pack_rhs)."""
import numpy as np
import pytest

import cost_support as cs

CASES = [(6, 3, 2), (12, 4, 5), (7, 9, 8), (20, 5, 16)]


def problem(n, m, N):
    return cs.dense_problem(n, m, N, cs.FAMILIES["moderate"], 11)


@pytest.mark.parametrize("n,m,N", CASES)
def test_S_on_a_knot_range_is_the_range_of_S(n, m, N):
    p = problem(n, m, N)
    red = cs.reduce(p)
    zt = np.random.default_rng([n, m, N]).standard_normal((2 * n + m) * N - m)
    lam, x, u = cs.split(cs.apply_S(red, zt), n, m, N)
    lt, xt, ut = cs.split(zt, n, m, N)
    for k0, nk in {(0, 1), (N - 1, 1), (0, N), (N // 2, 1), (max(N // 2 - 1, 0), 2)}:
        for k in range(k0, k0 + nk):  # knot k from its own blocks and its own record: the operations of apply_S
            assert np.array_equal(red["L"][k] @ lt[k], lam[k])
            xk = cs._bwd(red["L"][k], xt[k])
            assert np.array_equal(xk, x[k])
            if k < N - 1:
                assert np.array_equal(cs._bwd(red["LR"][k], ut[k]) - red["G"][k] @ xk, u[k])
            else:
                assert not u[k].any()
    # ... and a change of z~ outside the range leaves the range alone
    k0, nk = 0, 1
    other = zt.copy()
    other[(2 * n + m) * (k0 + nk):] += 1.0
    l2, x2, u2 = cs.split(cs.apply_S(red, other), n, m, N)
    assert np.array_equal(l2[:nk], lam[:nk]) and np.array_equal(x2[:nk], x[:nk]) and np.array_equal(u2[:nk], u[:nk])


@pytest.mark.parametrize("n,m,N", CASES)
def test_replacing_r_alone_changes_the_reduced_q(n, m, N):
    p = problem(n, m, N)
    red = cs.reduce(p)
    r2 = p["r"] + 1.0
    red2 = cs.reduce(dict(p, r=r2))
    # every knot but the last (which has no r): q~ moves by -L^-1 G' (r2 - r), and G is not zero in this family
    for k in range(N - 1):
        assert np.abs(red["G"][k]).max() > 0
        assert not np.array_equal(red2["qt"][k], red["qt"][k])
        shift = cs._fwd(red["L"][k], red["G"][k].T @ (r2[k] - p["r"][k]))
        assert np.allclose(red["qt"][k] - red2["qt"][k], shift, rtol=1e-9, atol=1e-12)
    assert np.array_equal(red2["qt"][N - 1], red["qt"][N - 1])
    # S' says the same on the packed vector: the u rows of g reach the x rows of S' g
    g = np.zeros((2 * n + m) * N - m)
    g[2 * n:2 * n + m] = 1.0  # the u rows of knot 0 alone
    _, xs, _ = cs.split(cs.apply_St(red, g), n, m, N)
    assert xs[0].any() and not xs[1:].any()
    # d and x0 enter the lambda rows alone: replacing them leaves q~ and r~ as they are
    red3 = cs.reduce(dict(p, d=p["d"] + 1.0, x0=p["x0"] - 2.0))
    assert np.array_equal(red3["qt"], red["qt"]) and np.array_equal(red3["rt"], red["rt"])
