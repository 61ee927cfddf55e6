"""Non-finite inputs and Cholesky failure reporting in every solve path (the runner and the host model: failure_support.py).

Per case -- one per schedule name of ndlqr_hip_schedule, at the smallest horizon that still selects it, batch 5 with the bad
members 1 and 3 (batch 3 with bad member 1 where the shape is large) -- and per placement:
  * a single NaN / +Inf in the entries (n-1, 0) and (0, last column) of A_k and of B_k, for every separator k (N <= 16;
    failure_support.separators_to_test beyond): the solve returns NDLQR_ERR_NOT_SPD, cholesky_failures() equals the growth of
    the per-problem words, the words of healthy members do not grow, a bad member's word grows by at least
    len(contaminated(k, N)) (failure_support.COUNT_BOUNDS), solutions and device KKT residuals of the healthy members --
    with a KEEP flag also their rhs-only re-solve with a new right-hand side and their adjoint -- equal a solve of the healthy
    batch bit for bit, and re-initialised with the healthy batch the solver returns 0 with no word growing and the same bits;
  * -1, 0, NaN, +Inf in one entry of Q_k (terminal Q included) and of R_k: the same with a count bound of 1;
  * NaN in A, B, R, r, d of the caller's last knot: return 0, no count grows, the same bits;
  * Q_{N-1}[n-1] = 1e-310 (an isolated infinite pivot of S_{N-2}): the member is flagged, or its solution is one.
The schedules that depend on NDLQR_PAIR1 / NDLQR_COMPACT1 run the same runner in the child processes of
tests/test_pair1_bottom.py and tests/test_compact1_records.py.

Which placements reach which flag_failure site (launch_small.hpp, launch_reduced.hpp, launch_generic in ndlqr_hip.hip):
  staging of the weights -- every weight placement of the case's schedule, and nothing else:
    kernels_bottom_reduced.hpp:1065  bottom_group_mc: reduced-fused2, reduced-compact-records, reduced-records, reduced-tree,
                                     reduced at 9 states and more
    kernels_rowbcast.hpp:240         rb_bottom: reduced at (6,3)
    kernels_small.hpp:1208           bottom_small: knot-lean, knot-keep, knot-strict
    kernels_reduced_mfma.hpp:388     separator_reduced_mfma<LEVEL0>: generic-reduced(-records); terminal Q at s == N - 2
    kernels_leaf.hpp:28              leaf_generic: generic-lean, generic-keep, generic-strict
  Cholesky passes -- A_k / B_k placements; "level l" means k of that level and every k below it in the tree:
    kernels_bottom_reduced.hpp:1146  chol_pair_y_mc, level 0, s0 = lane 0 (k = 0 mod 4), s2 = lane 32 (k = 2 mod 4): reduced
                                     (9 states and more), reduced-fused2, reduced-compact-records
    kernels_bottom_reduced.hpp:1186  chol_pair_mc, level 0, the same halves: reduced-records, reduced-tree
    kernels_bottom_reduced.hpp:1233  chol_pair_y_mc on t, level 1: reduced (10,4) (compact level-1 records), reduced-fused2
                                     with NDLQR_PAIR1=0
    kernels_bottom_reduced.hpp:918   chol_pair1_y_mc, level 1, t0 = lane 0 (k = 1 mod 8 and its children 0, 2), t1 = lane 32
                                     (k = 5 mod 8, children 4, 6): reduced-fused2 at (12,4) -- the padded horizon 13 too --,
                                     and with NDLQR_PAIR1=1 at (10,4)
    kernels_bottom_reduced.hpp:1251  chol_wy_mc on t, level 1: reduced (9,3), reduced-compact-records, reduced-records,
                                     reduced-tree, reduced-fused2 with NDLQR_COMPACT1=0
    kernels_bottom_reduced.hpp:797   reduced_eliminate_pass_mc, level 2 (k = 3 mod 8): reduced-fused2
    kernels_bottom_reduced.hpp:733   reduced_separator_mc: level >= 2 of reduced, reduced-records, reduced-compact-records,
                                     reduced-tree; level >= 3 of reduced-fused2 (reduced_level_mc at N = 16, reduced_top_mc at
                                     N = 32)
    kernels_rowbcast.hpp:315, 405    rb_chol_inv of rb_bottom, level 0 (a DPP row per separator) and level 1: reduced at (6,3)
    kernels_small.hpp:1298           separator_core in bottom_small, levels 0 and 1: knot-lean, knot-keep, knot-strict
    kernels_small.hpp:350            separator_wave (level_small), level >= 2: the same
    kernels_reduced_mfma.hpp:201     chol16_inverse_in_place in reduced_cholesky, every level: generic-reduced(-records); the
                                     second diagonal block and the look-ahead at 32 and 64 states
    kernels_mfma.hpp:55              chol16_and_inverse in sep_cholesky (separator_mfma), every level: generic-keep at
                                     (144,16), generic-lean at (144,16)
    kernels_generic.hpp:141          pivot loop of separator_generic, every level: generic-strict, generic-keep at (20,6),
                                     (6,3) and (5,2); at N = 2 the only separator is the last and the top one, so the
                                     isolated infinite pivot has no ancestor to be reported by
    kernels_small.hpp:109            (the pivot test of factor_solve behind :350 and :1298) the isolated infinite pivot at
                                     knot-lean and knot-keep, whose factor panel stays finite: no ancestor reports it
"""
import pytest

import failure_support as fs

pytestmark = pytest.mark.gpu

# (n, m, N, batch, flags, NDLQR_TREE, schedule): shapes of test_gpu_gradients.SCHEDULE_CASES at the smallest horizon that
# still selects the schedule -- N = 16 for the size-specialised instances (two eight-knot workgroups: a first and a last
# tile), N = 8 where only that horizon gives the full-record schedule, N = 2 / 4 for the runtime-sized ones -- plus the flag
# modes none / KEEP_RECORDS / KEEP_FACT / STRICT_FP | KEEP_FACT / GENERIC, one longer horizon per launch that only exists
# there (reduced_top_mc: N = 32; the 64-knot knot-lean case of the gradients), and the padded horizons 5 and 13.
CASES = [(12, 4, 16, 5, "none", "0", "reduced-fused2"),
         (12, 4, 32, 3, "none", "0", "reduced-fused2"),
         (12, 4, 13, 5, "none", "0", "reduced-fused2"),
         (10, 4, 16, 5, "none", "0", "reduced"),
         (9, 3, 16, 5, "none", "0", "reduced"),
         (6, 3, 16, 5, "none", "0", "reduced"),
         (12, 4, 8, 5, "none", "0", "reduced-records"),
         (12, 4, 8, 5, "records", "0", "reduced-records"),
         (12, 4, 16, 5, "records", "0", "reduced-compact-records"),
         (7, 9, 16, 3, "records", "0", "reduced-compact-records"),
         (12, 4, 16, 5, "none", None, "reduced-tree"),
         (1, 1, 16, 3, "records", None, "reduced-tree"),
         (6, 3, 5, 5, "records", None, "reduced-tree"),
         (2, 1, 16, 5, "none", None, "knot-lean"),
         (2, 1, 64, 3, "records", None, "knot-lean"),
         (2, 1, 13, 5, "none", None, "knot-lean"),
         (12, 4, 16, 5, "fact", None, "knot-keep"),
         (12, 4, 16, 5, "strict", None, "knot-strict"),
         (5, 2, 2, 3, "none", None, "generic-reduced"),
         (5, 2, 2, 3, "records", None, "generic-reduced-records"),
         (6, 3, 4, 5, "none", None, "generic-reduced"),
         (6, 3, 4, 5, "records", None, "generic-reduced-records"),
         (20, 6, 16, 5, "none", None, "generic-reduced"),
         (20, 6, 5, 3, "records", None, "generic-reduced-records"),
         (12, 4, 16, 5, "generic", None, "generic-reduced"),
         (32, 8, 4, 3, "none", None, "generic-reduced"),
         (32, 8, 4, 3, "records", None, "generic-reduced-records"),
         (64, 16, 4, 3, "none", None, "generic-reduced"),
         (64, 16, 4, 3, "records", None, "generic-reduced-records"),
         (144, 16, 8, 3, "none", None, "generic-lean"),
         (144, 16, 8, 3, "records", None, "generic-keep"),
         (20, 6, 16, 5, "fact", None, "generic-keep"),
         (20, 6, 32, 3, "fact", None, "generic-keep"),
         (6, 3, 4, 5, "fact", None, "generic-keep"),
         (5, 2, 2, 3, "fact", None, "generic-keep"),     # (one separator: the last and the top one, no ancestor)
         (5, 2, 2, 3, "strict", None, "generic-strict"),
         (20, 6, 16, 5, "strict", None, "generic-strict"),
         (20, 6, 13, 3, "strict", None, "generic-strict")]


def case_id(c):
    return "%s-%d.%d.%d.x%d-%s" % (c[6], c[0], c[1], c[2], c[3], c[4])


@pytest.mark.parametrize("n,m,N,batch,flags,tree,want", CASES, ids=[case_id(c) for c in CASES])
def test_failures_are_reported_per_problem(ndlqr, monkeypatch, n, m, N, batch, flags, tree, want):
    if tree is not None:
        monkeypatch.setenv("NDLQR_TREE", tree)
    out = fs.run_case(ndlqr, n, m, N, batch, flags, want)
    print(case_id((n, m, N, batch, flags, tree, want)), "solves", out["solves"], "isolated infinity", out.get("isolated"))
    assert out["schedule"] == want, out["schedule"]
    assert not out["violations"], "%d violations, the first: %s" % (len(out["violations"]), out["violations"][:6])


def test_every_schedule_name_has_a_case():
    """(the names of ndlqr_hip.h, and reduced-compact-records, which the header leaves out)"""
    assert {c[6] for c in CASES} == set(fs.COUNT_BOUNDS)
