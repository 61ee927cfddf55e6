"""The reference of the padded-horizon tests checked against an independent witness: the oracle on
horizon_support.pad_problem(prob) must solve the N-knot problem, for horizons N that are no power of two.

Witness: support.kkt_residual_ld, the extended-precision residual of the N-knot KKT system (it shares no code with the
oracle or with pad_problem and never sees the padded problem). Bar: the infinity norm of that residual is at most
    64 eps (2n + m) max|z| max(1, max|A|, max|B|, max Q, max R)
-- 64 roundings of relative size eps per row of K of a knot, at the scale of the products in that row (the data the
N-knot problem uses: A, B, R of the last knot excluded). Measured on the shapes below (seeds 700 .. 702): the residual is
between 1.3e-15 and 1.4e-14 at max|z| up to 96, the bar between 2.1e-12 and 4.1e-11 -- two to three orders above it.
The tail of the padded solution is exactly zero and the oracle reports no non-positive pivot, also with A, B, R, r, d of
the caller's last knot set to NaN or to garbage (R = -3 included): the padded problem never contains them."""
import numpy as np
import pytest

import rslqr_amd
from horizon_support import kkt_bar, kkt_inf, next_pow2, pad_problem, poisoned, reference, synth
from support import Problem

SHAPES = [(2, 1, 3), (3, 2, 5), (6, 3, 7), (4, 2, 9), (12, 4, 12), (6, 3, 100), (12, 4, 33)]


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_padded_problem_solves_the_n_knot_problem(oracle, n, m, N):
    for seed in (700, 701, 702):
        prob = synth(rslqr_amd, n, m, N, seed)
        z, tail, fails = reference(oracle, prob)
        assert fails == 0
        assert z.size == prob.nvars and tail.size == (2 * n + m) * next_pow2(N) - prob.nvars
        assert not tail.any(), np.abs(tail).max()  # exactly zero
        res, bar = kkt_inf(prob, z), kkt_bar(prob, z)
        print("(%d,%d,%d) seed %d: residual %.3g, bar %.3g, max|z| %.3g" % (n, m, N, seed, res, bar, np.abs(z).max()))
        assert res <= bar, (res, bar)


@pytest.mark.parametrize("n,m,N", SHAPES)
def test_last_knot_data_never_enters(oracle, n, m, N):
    prob = synth(rslqr_amd, n, m, N, 710)
    z, _, _ = reference(oracle, prob)
    garbage = Problem(n, m, N, *[a.copy() for a in prob.arrays()])
    rng = np.random.default_rng(N)
    for a in (garbage.A, garbage.B, garbage.r, garbage.d):
        a[N - 1] = 1e3 * rng.standard_normal(a.shape[1])
    garbage.R[N - 1] = -3.0
    for other in (garbage, poisoned(prob)):
        z2, tail, fails = reference(oracle, other)
        assert fails == 0 and not tail.any()
        assert np.array_equal(z2, z)
        assert np.isfinite(z2).all()


def test_power_of_two_horizons_are_left_alone(oracle):
    prob = synth(rslqr_amd, 6, 3, 8, 720)
    assert pad_problem(prob) is prob
    assert pad_problem(prob, 16).N == 16
