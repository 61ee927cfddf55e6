"""The references of tests/test_gpu_residuals.py, the CPU side (no GPU): the plain extended-precision KKT rows of
residual_support.kkt_rows_ld against the oracle's KKT residual, and the seeds of the strict-mode termination test of the
box-constrained solve -- on the restatement driven by the oracle every one of them ends by convergence before max_iter."""
import numpy as np
import pytest

from residual_support import (BOX_TERMINATION, BOX_TERMINATION_CASES, box_termination_reference, kkt_rows_ld, mixed_problem,
                              residual_dd_launch)
from test_box_host import synth


@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 16), (5, 2, 2)])
def test_plain_rows_agree_with_the_oracle(ndlqr, oracle, n, m, N):
    """Both norms to 1e-12 relative, on a solution and on that solution against another problem's right-hand side. The
    mixed pair has a residual of the size of the data, and 1e-12 is relative to the residual norm itself. On a solution
    the residual norm is a rounding of zero (1e-15 .. 3e-14 here, where the fp64 oracle and the extended-precision rows
    differ by 1 % .. 12 % of it), so 1e-12 is relative to the norm of the right-hand side there: the two differ by
    1e-17 .. 4e-17 of it."""
    first, other = synth(ndlqr, n, m, N, 40), synth(ndlqr, n, m, N, 90)
    z = oracle.solve(first, 1)[0][: first.nvars]
    res, b, rn, bn = kkt_rows_ld(first, z)
    ores, obn = oracle.kkt_residual(first, z)
    assert res.dtype == np.longdouble and res.shape == b.shape == (first.nvars,)
    assert abs(bn - obn) <= 1e-12 * obn
    assert rn <= 1e-9 * max(1.0, obn) and ores <= 1e-9 * max(1.0, obn)
    assert abs(rn - ores) <= 1e-12 * obn, (float(rn), ores, obn)
    mixed = mixed_problem(first, other)
    res, b, rn, bn = kkt_rows_ld(mixed, z)
    ores, obn = oracle.kkt_residual(mixed, z)
    assert ores > 1e-3
    assert abs(rn - ores) <= 1e-12 * ores, (float(rn), ores)
    assert abs(bn - obn) <= 1e-12 * obn, (float(bn), obn)
    # the right-hand side is the other problem's, entry by entry
    _, b_other, _, _ = kkt_rows_ld(other, z)
    assert np.array_equal(b, b_other)


def test_a_single_entry_moves_a_single_row(ndlqr, oracle):
    """What test_gpu_residuals.py relies on: delta on one right-hand-side entry moves one row of K z - b by delta, and the
    r of the last knot moves none."""
    n, m, N = 5, 2, 4
    prob = synth(ndlqr, n, m, N, 3)
    z = oracle.solve(prob, 1)[0][: prob.nvars]
    base = kkt_rows_ld(prob, z)[0]
    rows = 2 * n + m
    for name, k, i, row in (("x0", None, 1, 1), ("d", 2, 4, 3 * rows + 4), ("q", 3, 0, 3 * rows + n), ("r", 1, 1, rows + 2 * n + 1),
                            ("r", N - 1, 0, None)):
        saved = getattr(prob, name).copy()
        if k is None:
            prob.x0[i] += 0.25
        else:
            getattr(prob, name)[k, i] += 0.25
        moved = np.nonzero(kkt_rows_ld(prob, z)[0] != base)[0]
        getattr(prob, name)[...] = saved
        assert moved.tolist() == ([] if row is None else [row]), (name, k, i, moved)


# shape -> (threads, LDS-staged tile, passes of the task loop in block 0, padded block size): what each case of
# test_gpu_residuals.VECTOR_SHAPES was chosen for. A change of launch_residual_dd, of the padding rules or of the instance
# list that moves a case shows here first (the restatement reads csrc/small_instances.def).
LAUNCHES = {(32, 8, 4): (128, True, 1, (32, 8)),
            (48, 16, 4): (256, True, 1, (48, 16)),
            (96, 16, 2): (256, True, 2, (96, 16)),
            (128, 16, 2): (256, True, 2, (128, 16)),
            (144, 16, 2): (256, False, 2, (144, 16)),
            (144, 16, 4): (256, False, 2, (144, 16)),
            (130, 5, 4): (256, False, 2, (144, 8)),
            (150, 10, 2): (256, False, 2, (160, 12)),
            (256, 32, 2): (256, False, 4, (256, 32)),
            (1, 1, 8): (64, True, 1, (6, 3)),
            # the shapes of test_gpu_refine.RESIDUAL_SHAPES, for comparison: all alike
            (6, 3, 8): (64, True, 1, (6, 3)),
            (16, 4, 8): (64, True, 1, (16, 4)),
            (7, 9, 8): (64, True, 1, (8, 16))}


def test_launch_shapes_of_the_vector_cases():
    from test_gpu_residuals import VECTOR_SHAPES
    assert set(VECTOR_SHAPES) <= set(LAUNCHES)
    for shape, want in LAUNCHES.items():
        assert residual_dd_launch(*shape) == want, (shape, residual_dd_launch(*shape))
    # (128, 16) is the largest staged block: 8 (128 * 145 + 2 * 272) + 64 bytes
    assert 8 * (128 * 145 + 2 * 272) + 64 == 152896 and not residual_dd_launch(144, 16, 2)[1]


@pytest.mark.parametrize("n,m,N,seed", BOX_TERMINATION_CASES)
def test_box_termination_seeds_converge_on_the_restatement(ndlqr, oracle, n, m, N, seed):
    _, _, ref = box_termination_reference(ndlqr, oracle, n, m, N, seed)
    for p, r in enumerate(ref):
        rit, rst = r[5], r[6]
        print((n, m, N), seed + p, "iterations", rit, "status", rst)
        assert rst == 1 and 1 < rit < BOX_TERMINATION["max_iter"], (p, rit, rst)
