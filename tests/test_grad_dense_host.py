"""The numpy restatement of the dense-cost gradients (grad_dense_support.py) against the independent
reference cost_support.gradient_reference, and the C entry point's NULL handle. No GPU."""
import numpy as np
import pytest

import cost_support as cs
import grad_dense_support as gd

CASES = [(6, 3, 2), (7, 9, 5), (12, 4, 8)]


@pytest.mark.parametrize("n,m,N", CASES)
def test_restatement_equals_the_reference(n, m, N):
    """The same algebra in another layout and operation order: 1e-13 relative per output."""
    fam = cs.family(n, m, N, "moderate")
    got = gd.restate(fam["z"], fam["w"], n, m, N)
    for i, p in enumerate(fam["probs"]):
        ref = cs.gradient_reference(p, fam["z"][i], fam["w"][i])
        for k in gd.NAMES:
            a = gd.to_math(k, got[k][i], n, m)
            assert a.shape == ref[k].shape, k
            err = np.linalg.norm(a - ref[k]) / np.linalg.norm(ref[k])
            assert err <= 1e-13, (k, i, err)


@pytest.mark.parametrize("n,m,N", CASES)
def test_symmetry_and_last_knot(n, m, N):
    fam = cs.family(n, m, N, "moderate")
    got, mag = gd.restate(fam["z"], fam["w"], n, m, N, mags=True)
    for k in ("Q", "R"):
        r = gd.rows_of(k, n, m)
        M = got[k].reshape(cs.BATCH, N, r, r)
        assert np.array_equal(M.view(np.uint64), M.transpose(0, 1, 3, 2).view(np.uint64)), k
    for k in ("A", "B", "H", "R", "r", "d"):
        last = got[k][:, N - 1]
        assert np.array_equal(last.view(np.uint64), np.zeros_like(last).view(np.uint64)), k
        assert np.abs(got[k][:, : N - 1]).max() > 0, k
    assert np.abs(got["Q"][:, N - 1]).min() > 0 and np.abs(got["q"][:, N - 1]).min() > 0
    for k in gd.MATRICES:
        assert mag[k].shape == got[k].shape and (np.abs(got[k]) <= mag[k]).all(), k


def test_sums():
    rng = np.random.default_rng(5)
    per = rng.standard_normal((7, 4, 3)) * 10.0 ** rng.integers(-8, 8, (7, 4, 3))
    exact = gd.fsum(per)
    assert exact.shape == (4, 3)
    assert (np.abs(gd.ordered_sum(per) - exact) <= 7 * gd.EPS * np.abs(per).sum(axis=0)).all()
    assert np.array_equal(gd.ordered_sum(per[:1]), per[0])


def test_null_handle(ndlqr):
    assert ndlqr.lib().ndlqr_BatchGradientsDense(None, 0, *[None] * 9) == -1
    assert ndlqr.GRAD_DENSE_NAMES == gd.NAMES
    assert [getattr(ndlqr, "GRADD_" + k) for k in gd.NAMES] == [1 << i for i in range(9)]
