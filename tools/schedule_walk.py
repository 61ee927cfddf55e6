"""Developer tool (GPU box): one tiny solve per row of the schedule table of DESIGN.md section 3, in one process, for
comparing the launches of two builds of the library.

    NDLQR_PIPELINE=1 rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/schedule_walk.py
    python3 tools/schedule_walk.py --list DIR/.../run_kernel_trace.csv > launches.txt

The first form prints the schedule() of every case (each case sets its NDLQR_* switches before it creates its solver;
NDLQR_LIBRARY picks the build, NDLQR_PIPELINE=1 makes stream order trace order). The second prints the ordered list of
kernel name, grid, workgroup and LDS size of such a trace: two builds that decide alike give identical lists.
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("NDLQR_TREE", "NDLQR_FUSE2", "NDLQR_NO_TOP", "NDLQR_ROWBCAST")
RECORDS, FACT, STRICT, GENERIC = "FLAG_KEEP_RECORDS", "FLAG_KEEP_FACT", "FLAG_STRICT_FP", "FLAG_GENERIC"
# (n, m, N, batch, switches, flags, what to run after the solve)
CASES = [
    (12, 4, 16, 3, {}, (), ""),                                                  # tree
    (12, 4, 16, 3, {"NDLQR_TREE": "0"}, (), ""),                                 # fused2
    (12, 4, 16, 3, {"NDLQR_TREE": "0", "NDLQR_FUSE2": "0"}, (), ""),             # not fused
    (12, 4, 16, 3, {"NDLQR_TREE": "0", "NDLQR_NO_TOP": "1"}, (), ""),            # level per launch
    (12, 4, 64, 3, {"NDLQR_TREE": "0"}, (), ""),                                 # ... with reduced_top_mc (K >= 5)
    (12, 4, 64, 3, {"NDLQR_TREE": "0", "NDLQR_NO_TOP": "1"}, (), ""),            # ... and without
    (12, 4, 64, 3, {"NDLQR_TREE": "0", "NDLQR_FUSE2": "0"}, (), ""),
    (6, 3, 32, 3, {"NDLQR_TREE": "0"}, (), ""),                                  # rowbcast
    (6, 3, 32, 3, {"NDLQR_TREE": "0", "NDLQR_ROWBCAST": "0"}, (), ""),
    (12, 4, 16, 3, {}, (RECORDS,), "rhs adjoint"),                               # kept records: full ...
    (12, 4, 16, 3, {"NDLQR_TREE": "0"}, (RECORDS,), "rhs adjoint step"),         # ... and compact, their re-solves
    (12, 4, 64, 3, {"NDLQR_TREE": "0"}, (RECORDS,), "rhs step"),
    (12, 4, 64, 3, {"NDLQR_TREE": "0"}, (), "step"),                             # a step that factors, knot range alone
    (4, 2, 8, 2, {}, (), ""),                                                    # knot schedules
    (4, 2, 8, 2, {}, (STRICT,), ""),
    (4, 2, 8, 2, {}, (FACT,), "rhs"),
    (4, 2, 8, 2, {}, (STRICT, FACT), "rhs"),
    (16, 4, 8, 2, {}, (), ""),                                                   # runtime-sized separator-only
    (16, 4, 8, 2, {}, (RECORDS,), "rhs adjoint"),
    (64, 16, 8, 2, {}, (RECORDS,), "step"),
    (16, 300, 4, 1, {}, (), ""),                                                 # knot-based runtime-sized
    (16, 300, 4, 1, {}, (RECORDS,), "rhs"),
    (144, 16, 4, 1, {}, (), ""),                                                 # ... large blocks
    (144, 16, 4, 1, {}, (STRICT,), ""),
    (12, 4, 16, 3, {}, (GENERIC,), ""),                                          # runtime-sized on a specialised shape
    (12, 4, 16, 3, {}, (GENERIC, STRICT), ""),
]


def walk():
    import numpy as np
    import rslqr_amd as R
    for n, m, N, batch, env, flags, then in CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        fl = 0
        for f in flags:
            fl |= getattr(R, f)
        bs = R.BatchSolver(n, m, N, batch, flags=fl)
        bs.initialize_synthetic(1)
        names = []
        for _ in range(2):  # (captured, then replayed)
            assert bs.solve() == 0
            names.append(bs.schedule())
        for what in then.split():
            if what == "rhs":
                assert bs.solve_rhs_only() == 0
            elif what == "adjoint":
                assert bs.solve_adjoint(np.ones((batch, bs.nvars))) == 0
            elif what == "step":
                bs.set_step_selection(8 if N > 16 else 0, 1, R.SOLN_INPUT | R.SOLN_ONLY)
                out = R.pinned_empty((batch, 1, m))
                x0 = R.pinned_empty((batch, n))
                x0[:] = 0.5
                for _ in range(2):
                    assert bs.step_async(None, None, None, x0, out) == 0
                    assert bs.synchronize() == 0
            names.append(what + ": " + bs.schedule())
        print("(%d,%d,%d)x%d %s %s -> %s" % (n, m, N, batch, " ".join("%s=%s" % kv for kv in sorted(env.items())) or "-",
                                            "|".join(f[5:] for f in flags) or "default", ", ".join(names)), flush=True)
        bs.close()


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].replace("void ndlqr::", "").replace("ndlqr::", "")
        print("%s grid %s,%s,%s wg %s,%s,%s lds %s" % (name, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                                                      r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"],
                                                      r["LDS_Block_Size"]))


if __name__ == "__main__":
    if "--list" in sys.argv:
        launches(sys.argv[sys.argv.index("--list") + 1])
    else:
        walk()
