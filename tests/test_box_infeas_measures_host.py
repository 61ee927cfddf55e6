"""The references of tests/test_gpu_box_infeas_measures.py, the CPU side (no GPU): the launch classes of box_certify
that its shapes were chosen for, against box_infeas_measures_support.certify_launch, and measures_reference against
box_infeas_support.farkas_check -- two evaluations that share no code -- on a hand-made certificate and on the
differences of two consecutive iterates of the numpy restatement driven by the oracle."""
import numpy as np
import pytest

from box_infeas_measures_support import certify_launch, conditions, measures_reference
from box_infeas_support import farkas_check, infeasible_bounds
from box_support import admm_reference
from support import Problem
from test_box_host import synth

# shape -> (padded block, w, G, knots per pass, largest dlam load nl * n, largest task count nk * w): what each case of
# test_gpu_box_infeas_measures.SHAPES was chosen for. A change of certify_group, of the kernel's loops, of the padding
# rules or of the instance list that moves a case shows here first.
LAUNCHES = {(12, 4, 16): ((12, 4), 16, 16, [16], 192, 256),           # one pass of exactly 256 tasks, no knot behind it
            (12, 4, 32): ((12, 4), 16, 16, [16, 16], 204, 256),      # two full passes, dlam of the knot behind the first
            (13, 4, 16): ((13, 4), 17, 15, [15, 1], 208, 255),       # a tail pass of one knot
            (20, 6, 16): ((20, 6), 26, 9, [9, 7], 200, 234),         # passes of 9 + 7
            (7, 9, 16): ((8, 16), 24, 10, [10, 6], 88, 240),         # small padded block
            (1, 1, 8): ((6, 3), 9, 28, [8], 48, 72),                 # the smallest padded instance
            (64, 16, 8): ((64, 16), 80, 3, [3, 3, 2], 256, 240),     # a load of exactly 256
            (96, 16, 4): ((96, 16), 112, 2, [2, 2], 288, 224),       # strided dlam load
            (144, 16, 4): ((144, 16), 160, 1, [1, 1, 1, 1], 288, 160),  # one knot per pass, strided load
            (130, 5, 4): ((144, 8), 152, 1, [1, 1, 1, 1], 288, 152),    # padding beyond 128 states
            (256, 32, 2): ((256, 32), 288, 1, [1, 1], 512, 288),     # w >= 256: strided task loop, load of 512
            # the shapes of test_gpu_box_infeas.CASES, for comparison: one or two passes, nothing strided
            (6, 3, 8): ((6, 3), 9, 28, [8], 48, 72),
            (5, 2, 2): ((5, 2), 7, 36, [2], 10, 14),
            (16, 4, 8): ((16, 4), 20, 12, [8], 128, 160),
            (2, 1, 16): ((2, 1), 3, 85, [16], 32, 48)}


def test_launch_classes_of_the_measure_cases():
    from test_gpu_box_infeas_measures import ENTRY_SHAPES, SHAPES
    assert set(SHAPES) <= set(LAUNCHES) and set(ENTRY_SHAPES) <= set(SHAPES)
    for shape, want in LAUNCHES.items():
        assert certify_launch(*shape) == want, (shape, certify_launch(*shape))
    got = {s: certify_launch(*s) for s in SHAPES}
    assert any(w >= 256 and tasks > 256 for _, w, _, _, _, tasks in got.values())          # the strided task loop
    assert sum(load > 256 for _, _, _, _, load, _ in got.values()) >= 4                     # the strided dlam load
    assert any(128 < w < 256 and G == 1 for _, w, G, _, _, _ in got.values())              # one knot per pass below 256
    assert any(pad[0] > 128 and pad != s[:2] for s, (pad, _, _, _, _, _) in got.items())   # padded beyond 128 states
    assert any(len(p) >= 2 and p[0] == p[1] == G for _, _, G, p, _, _ in got.values())     # two full passes
    assert any(len(p) >= 2 and p[-1] == 1 and G > 1 for _, _, G, p, _, _ in got.values())  # a tail pass of one knot
    assert any(tasks == 256 for _, _, _, _, _, tasks in got.values()) and any(load == 256 for _, _, _, _, load, _ in got.values())


def _agree(ref, c):
    for key, other in (("E", "e_inf"), ("D", "dmu_inf"), ("S", "S")):
        assert abs(ref[key] - c[other]) <= 1e-15 * abs(c[other]), (key, ref[key], c[other])


def test_measures_reference_on_the_hand_made_certificate():
    """(test_box_infeas_host.py) x1 = a x0 + b u0 + d, |u0| <= 1, x1 <= (a x0 + d - |b|) - gap: E = 0, D = 1, S = -gap, and
    nothing points to an infinite bound; with dmu_x1 flipped it does."""
    a, b, d, x0, gap = 0.9, 0.5, 0.3, 2.0, 0.25
    prob = Problem(1, 1, 2, [a, 0.0], [b, 0.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [d, 0.0], [x0])
    bounds = infeasible_bounds(prob, 1.0, 1, gap)
    dlam = np.array([[a], [1.0]])
    dmu_x = np.array([[0.0], [1.0]])
    dmu_u = np.array([[-b], [0.0]])
    ref = measures_reference(prob, bounds, dlam, dmu_x, dmu_u)
    c = farkas_check(prob, bounds, dlam, dmu_x, dmu_u, 1e-4)
    assert ref["E"] <= 1e-15 and ref["D"] == 1.0 and ref["I"] == 0.0 and abs(ref["S"] + gap) <= 1e-15, ref
    assert abs(ref["E"] - c["e_inf"]) <= 1e-15 and ref["D"] == c["dmu_inf"] and abs(ref["S"] - c["S"]) <= 1e-15 * gap
    assert conditions(ref, 1e-4) and c["ok"]
    assert ref["terms"] == 2 + 2  # two bounded entries, x0 dlam_0 and d_0 dlam_1
    assert ref["tol_E"] > 0 and 0 < ref["tol_S"] <= 1e-15
    flipped = measures_reference(prob, bounds, dlam, -dmu_x, dmu_u)
    assert flipped["I"] == 1.0 and flipped["D"] == 1.0 and not conditions(flipped, 1e-4)
    assert flipped["terms"] == 1 + 2 and flipped["E"] == 2.0


@pytest.mark.parametrize("n,m,N", [(6, 3, 8), (12, 4, 16)])
def test_measures_reference_agrees_with_farkas_check_on_consecutive_iterates(ndlqr, oracle, n, m, N):
    """dlam, dmu between iterations 3 and 4 of box_support.admm_reference (every input and every state of the knots >= 1
    bounded, as the device cases): E, D and S of measures_reference equal e_inf, dmu_inf and S of farkas_check to 1e-15
    relative."""
    from box_support import split
    prob = synth(ndlqr, n, m, N, 2101)
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    _, x, u = split(solve(prob), n, m, N)
    uhi = np.tile(0.5 * np.abs(u).mean(axis=0), (N, 1))
    xhi = np.tile(0.7 * np.abs(x[1:]).max(axis=0), (N, 1))
    bounds = (-xhi, xhi, -uhi, uhi)
    rho = float(prob.Q.mean())
    runs = [admm_reference(prob, solve, *bounds, rho, 1.6, 1e-300, 1e-300, it) for it in (3, 4)]
    assert all(r[6] == 2 for r in runs)
    (_, _, mx3, mu3, lam3, _, _), (_, _, mx4, mu4, lam4, _, _) = runs
    dlam, dmu_x, dmu_u = lam4 - lam3, mx4 - mx3, mu4 - mu3
    ref = measures_reference(prob, bounds, dlam, dmu_x, dmu_u)
    c = farkas_check(prob, bounds, dlam, dmu_x, dmu_u, 1e-4)
    print((n, m, N), ref, c)
    assert ref["D"] > 0 and ref["E"] > 0
    _agree(ref, c)
    assert ref["I"] == 0.0 and c["qualified"]  # (two-sided bounds: nothing points to an infinite one)
    assert conditions(ref, 1e-4) == c["ok"]
    assert ref["tol_E"] <= 1e-12 * ref["E"] and ref["tol_S"] <= 1e-12 * abs(ref["S"]), ref


def test_measures_entry_points_exist_and_refuse_bad_arguments(ndlqr):
    import ctypes as C
    L = ndlqr.lib()
    for name in ("ndlqr_CopyBatchInfeasibilityMeasures", "ndlqr_hip_download_infeasibility_measures"):
        assert name in ndlqr.exported_symbols() and hasattr(L, name)
    INVALID = ndlqr.api.ERR_INVALID
    buf, ints = np.zeros(4), np.zeros(1, dtype=np.int32)
    dp, ip = buf.ctypes.data_as(C.POINTER(C.c_double)), ints.ctypes.data_as(C.POINTER(C.c_int))
    # (no device here, so no solver: every call is refused; test_gpu_box_infeas_measures.py sends them to a real one)
    assert L.ndlqr_CopyBatchInfeasibilityMeasures(None, dp, ip) == INVALID
    L.ndlqr_hip_download_infeasibility_measures.restype = C.c_int
    L.ndlqr_hip_download_infeasibility_measures.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    assert L.ndlqr_hip_download_infeasibility_measures(None, dp, ip) == INVALID
