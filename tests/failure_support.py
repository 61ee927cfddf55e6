"""Host model and runner of the failure-reporting tests (tests/test_gpu_failures.py, and the `nonspd` modes of
tests/pair1_support.py and tests/compact1_support.py, which run the same runner in a child process).

The contract under test (include/ndlqr.h): a member of a batch whose data the factorisation cannot use -- a weight that is
not positive and finite, a non-finite entry of A or B -- makes the solve return NDLQR_ERR_NOT_SPD, is counted in
ndlqr_BatchCholeskyFailures and in ITS word of ndlqr_CopyBatchCholeskyFailureCounts, and leaves every other member's
results untouched, bit for bit. Nothing here asserts a figure for a solve path's accuracy: the checks are return codes,
counts and bit-equality (the one residual, of the isolated-infinity case, only tells a solution from garbage).

Host model (plain numpy / integers; checked against hand-written tables by tests/test_failure_support_host.py):
  level(k)            tree level of separator k: its number of trailing one bits (src/binary_tree.c:9-37)
  device_horizon(N)   the power of two the device pads the time axis to
  contaminated(k, N)  separator k and its ancestors, one per level from level(k) to K - 1, K = log2(device_horizon(N)):
                      the separators whose S-bar holds a NaN once the data of separator k (A_k, B_k) holds one -- k's own
                      by its leaf products, every ancestor's through the Schur contribution of the one below it
  must_flag(...)      whether a problem holds data the contract says is reported

Test infrastructure."""
import numpy as np

KEYS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
NOT_SPD = -3
SEED = 2300
REL_TOL = 1e-9  # the project's bar for a solution; here only: "is this a solution at all" (isolated-infinity case)


# ------------------------------------------------------------------------------------------------------- host model
def trailing_ones(k):
    t = 0
    while k & 1:
        k >>= 1
        t += 1
    return t


def level(k):
    return trailing_ones(k)


def device_horizon(N):
    P = 1
    while P < N:
        P *= 2
    return P


def tree_depth(N):
    return device_horizon(N).bit_length() - 1


def ancestor(k, l):
    """the level-l separator whose subtree holds knot k and k + 1 (l >= level(k); l == level(k): k itself)"""
    return ((k >> (l + 1)) << (l + 1)) + (1 << l) - 1


def contaminated(k, N):
    P = device_horizon(N)
    assert 0 <= k < P - 1, (k, N)
    return [ancestor(k, l) for l in range(level(k), tree_depth(N))]


def must_flag(n, m, N, A, B, Q, R):
    """one problem's arrays ([N, ..]): a weight the solve uses that is non-finite or not positive, or an entry of A or B
    that the solve uses that is non-finite. A, B, R (r, d) of the caller's last knot are not used."""
    A, B, Q, R = (np.asarray(a, dtype=np.float64).reshape(N, -1) for a in (A, B, Q, R))
    bad_w = lambda w: bool((~np.isfinite(w) | ~(w > 0.0)).any())
    return bad_w(Q[:N]) or bad_w(R[: N - 1]) or not np.isfinite(A[: N - 1]).all() or not np.isfinite(B[: N - 1]).all()


def separators_to_test(N):
    """Separators of a caller horizon N that get a placement: all of them (0 .. N - 2) up to a device horizon of 16;
    beyond, those of the first eight-knot tile, of one interior tile and of the last tile, plus one separator of every
    level above 2 (the last one of that level; the top separator P / 2 - 1 is the only one of its level)."""
    P = device_horizon(N)
    if P <= 16:
        return list(range(N - 1))
    tiles = sorted({0, (P // 8) // 2, (N - 2) // 8})
    ks = {k for t in tiles for k in range(8 * t, 8 * t + 8) if k <= N - 2}
    for l in range(3, tree_depth(N)):
        of_level = [k for k in range(N - 1) if level(k) == l]
        if of_level:
            ks.add(of_level[-1])
    return sorted(ks)


# ---------------------------------------------------------------------------------------- lower bounds on the count
# One row per schedule name (ndlqr_hip.h, ndlqr_hip_schedule): what a placement in A_k or B_k must at least add to the
# bad member's word, and the lines that show it. "per-separator": the schedule runs one Cholesky per separator (one pass
# per 16 x 16 diagonal block beyond 16 states -- more flags, never fewer), each with a flag_failure of its own, so every
# separator of contaminated(k, N) flags once: the bound is len(contaminated(k, N)). No schedule folds the Cholesky passes
# of several tree levels into one check -- the launches that hold several levels (the bottom launches, reduced_top_mc, the
# tree launch) run them one after the other, each behind its own test -- so no row states a smaller bound.
PER_SEPARATOR = "per-separator"
COUNT_BOUNDS = {
    # bottom launch: levels 0 and 1 of a four-knot group, one paired pass for s0 | s2 flagged per half
    # (kernels_bottom_reduced.hpp:1145-1146 compact, :1183-1186 full records), one pass for t (:1233 compact level-1
    # records, :1250-1251 full); level >= 2: reduced_level_mc / reduced_top_mc -> reduced_separator_mc (:732-733).
    # rb_bottom (blocks up to 8 states): kernels_rowbcast.hpp:315 (four level-0 separators, a DPP row each), :405 (t).
    "reduced": (PER_SEPARATOR, "kernels_bottom_reduced.hpp:1145,1233,1250,732; kernels_rowbcast.hpp:315,405"),
    # bottom8_reduced_mc: the groups as above (paired level-1 pass: :916-918, flagged per half), level 2 inside the
    # launch (reduced_eliminate_pass_mc, :797), level >= 3 as above
    "reduced-fused2": (PER_SEPARATOR, "kernels_bottom_reduced.hpp:1145,1233,916-918,797,732"),
    "reduced-records": (PER_SEPARATOR, "kernels_bottom_reduced.hpp:1183-1186,1250-1251,732-733"),
    "reduced-compact-records": (PER_SEPARATOR, "kernels_bottom_reduced.hpp:1145-1146,1250-1251,732-733"),
    # bottom_reduced_mc<TREE>: the group, then the wavefront that arrives last at a parent eliminates it
    "reduced-tree": (PER_SEPARATOR, "kernels_bottom_reduced.hpp:1183-1186,1250-1251,732-733"),
    # bottom_small: levels 0, 1 through separator_core (kernels_small.hpp:1295-1298); level_small -> separator_wave (:347-350)
    "knot-lean": (PER_SEPARATOR, "kernels_small.hpp:1295-1298,347-350"),
    "knot-keep": (PER_SEPARATOR, "kernels_small.hpp:1295-1298,347-350"),
    "knot-strict": (PER_SEPARATOR, "kernels_small.hpp:1295-1298,347-350"),
    # one launch of separator_reduced_mfma per level, reduced_cholesky flags per diagonal block
    "generic-reduced": (PER_SEPARATOR, "kernels_reduced_mfma.hpp:199-201; ndlqr_hip.hip launch_reduced_generic"),
    "generic-reduced-records": (PER_SEPARATOR, "kernels_reduced_mfma.hpp:199-201; ndlqr_hip.hip launch_reduced_generic"),
    # launch_generic: one separator launch per level -- separator_mfma (sep_cholesky, kernels_mfma.hpp:54-55, per
    # diagonal block) or separator_generic (its pivot loop, kernels_generic.hpp:140-141)
    "generic-lean": (PER_SEPARATOR, "kernels_mfma.hpp:54-55; kernels_generic.hpp:140-141"),
    "generic-keep": (PER_SEPARATOR, "kernels_mfma.hpp:54-55; kernels_generic.hpp:140-141"),
    "generic-strict": (PER_SEPARATOR, "kernels_generic.hpp:140-141"),
}


def count_bound(schedule, k, N):
    kind, _ = COUNT_BOUNDS[schedule]
    assert kind == PER_SEPARATOR
    return len(contaminated(k, N))


# ------------------------------------------------------------------------------------------------------- placements
class Placement:
    """one value written into one entry of one field of one knot; bound: what it must add to the member's word"""

    def __init__(self, field, knot, entry, value, bound=1):
        self.field, self.knot, self.entry, self.value, self.bound = field, knot, entry, value, bound

    def __repr__(self):
        return "%s[%d][%d]=%r" % (self.field, self.knot, self.entry, self.value)


def matrix_entries(n, cols):
    """flat (column-major, n rows) indices of the entries (n - 1, 0) and (0, last column)"""
    return [n - 1, (cols - 1) * n]


def dynamics_placements(n, m, N, schedule):
    """NaN and +Inf, each in the entries (n - 1, 0) and (0, last column) of A_k and of B_k, for every separator of
    separators_to_test(N)"""
    out = []
    for k in separators_to_test(N):
        for field, cols in (("A", n), ("B", m)):
            for e in matrix_entries(n, cols):
                for v in (np.nan, np.inf):
                    out.append(Placement(field, k, e, v, count_bound(schedule, k, N)))
    return out


def weight_placements(n, m, N):
    """-1, 0, NaN and +Inf in one entry of Q_k (the separators' knots and the terminal knot) and of R_k"""
    out = []
    for k in separators_to_test(N) + [N - 1]:
        for field, size in (("Q", n), ("R", m)):
            if field == "R" and k == N - 1:
                continue  # (not part of the problem)
            for v in (-1.0, 0.0, np.nan, np.inf):
                out.append(Placement(field, k, k % size, v, 1))
    return out


def unused_placements(n, m, N):
    """NaN over A, B, R, r, d of the caller's last knot"""
    return [Placement(f, N - 1, slice(None), np.nan, 0) for f in ("A", "B", "R", "r", "d")]


def kkt_relative_residual(g, z):
    """||K z - b|| / ||b|| of the reference's KKT system (src/solver.c:122-194) in float64 numpy, for one problem's
    arrays g (dict) and its solution z in the order lambda, x, u per knot"""
    n, m = g["Q"].shape[1], g["R"].shape[1]
    N = g["Q"].shape[0]
    zb = 2 * n + m
    full = np.zeros(N * zb)
    full[: z.size] = z
    Z = full.reshape(N, zb)
    lam, x, u = Z[:, :n], Z[:, n:2 * n], Z[:, 2 * n:]
    A = g["A"].reshape(N, n, n).transpose(0, 2, 1)
    B = g["B"].reshape(N, m, n).transpose(0, 2, 1)
    res, rhs = [x[0] - g["x0"]], [g["x0"]]
    for k in range(N):
        nxt = A[k].T @ lam[k + 1] if k < N - 1 else 0.0
        res.append(g["Q"][k] * x[k] - lam[k] + nxt + g["q"][k])
        rhs.append(g["q"][k])
        if k < N - 1:
            res.append(g["R"][k] * u[k] + B[k].T @ lam[k + 1] + g["r"][k])
            res.append(A[k] @ x[k] + B[k] @ u[k] - x[k + 1] + g["d"][k])
            rhs += [g["r"][k], g["d"][k]]
    with np.errstate(all="ignore"):
        return float(np.linalg.norm(np.concatenate(res)) / np.linalg.norm(np.concatenate(rhs)))


# ------------------------------------------------------------------------------------------------------------ runner
def flag_value(R, name):
    return {"none": 0, "records": R.FLAG_KEEP_RECORDS, "fact": R.FLAG_KEEP_FACT,
            "strict": R.FLAG_STRICT_FP | R.FLAG_KEEP_FACT, "generic": R.FLAG_GENERIC}[name]


def bad_members(batch):
    """batch 5: members 1 and 3 (each its own placement); a smaller batch: member 1"""
    return (1, 3) if batch >= 5 else (1,)


class Runner:
    """One solver per case, re-initialised per placement. Every check appends what it finds wrong to `violations` (a
    list of strings: it travels through the child-process harnesses as JSON) and the tests assert that it is empty."""

    def __init__(self, R, n, m, N, batch, flags):
        self.R, self.n, self.m, self.N, self.batch = R, n, m, N, batch
        self.keep = flags in ("records", "fact", "strict")
        self.bs = R.BatchSolver(n, m, N, batch, flags=flag_value(R, flags))
        self.healthy = [R.generate_synthetic(n, m, N, SEED + p) for p in range(batch)]
        self.violations = []
        self.solves = 0
        rng = np.random.default_rng(SEED)
        self.rhs2 = [rng.standard_normal((batch, N, n)), rng.standard_normal((batch, N, m)),
                     0.1 * rng.standard_normal((batch, N, n)), rng.standard_normal((batch, n))]
        self.g = rng.standard_normal((batch, self.bs.nvars))
        self.base = self._run(self.healthy)
        if self.base["rc"] != 0 or self.base["grow"].any() or not np.isfinite(self.base["sol"]).all():
            self.violations.append("baseline: rc %d, counts grew by %s" % (self.base["rc"], self.base["grow"].tolist()))
        self.schedule = self.bs.schedule()

    def close(self):
        self.bs.close()

    def _stack(self, gs):
        return [np.stack([g[k] for g in gs]) for k in KEYS]

    def _run(self, gs):
        """initialise with the problems gs, solve, read everything the checks compare"""
        bs = self.bs
        before = bs.cholesky_failure_counts()
        bs.initialize_flat(*self._stack(gs))
        out = dict(rc=bs.solve())
        self.solves += 1
        out["failures"] = bs.cholesky_failures()
        out["grow"] = bs.cholesky_failure_counts().astype(np.int64) - before
        out["sol"] = bs.solutions().copy()
        out["res"] = np.stack(bs.kkt_residuals())
        if self.keep:
            bs.set_rhs_flat(*self.rhs2)
            out["rhs_rc"] = bs.solve_rhs_only()
            out["rhs_sol"] = bs.solutions().copy()
            out["adj_rc"] = bs.solve_adjoint(self.g)
            out["adj"] = bs.adjoint().copy()
            out["grow_after"] = bs.cholesky_failure_counts().astype(np.int64) - before
        return out

    def poisoned(self, placements):
        """the healthy batch with {member: [Placement, ..]} written in"""
        gs = [{k: v.copy() for k, v in g.items()} for g in self.healthy]
        for p, pls in placements.items():
            for pl in pls:
                gs[p][pl.field][pl.knot][pl.entry] = pl.value
        return gs

    def _same(self, got, members, tag):
        """solutions, device KKT residuals and, with a KEEP flag, the rhs-only re-solve and the adjoint of `members`
        equal the baseline's bit for bit"""
        for key in ("sol", "res") + (("rhs_sol", "adj") if self.keep else ()):
            for p in members:
                a, b = got[key], self.base[key]
                a, b = (a[:, p], b[:, p]) if key == "res" else (a[p], b[p])
                if not np.array_equal(a, b):
                    self.violations.append("%s: %s of healthy member %d differs from the baseline" % (tag, key, p))
        if self.keep and (got["rhs_rc"] != self.base["rhs_rc"] or got["adj_rc"] != self.base["adj_rc"]):
            self.violations.append("%s: re-solve return codes %d, %d (baseline %d, %d)"
                                   % (tag, got["rhs_rc"], got["adj_rc"], self.base["rhs_rc"], self.base["adj_rc"]))

    def recover(self, tag):
        """re-initialised with the healthy batch the solver returns 0, no word grows, every solution is the baseline's"""
        got = self._run(self.healthy)
        if got["rc"] != 0 or got["failures"] != 0 or got["grow"].any():
            self.violations.append("%s: recovery solve rc %d, failures %d, counts grew by %s"
                                   % (tag, got["rc"], got["failures"], got["grow"].tolist()))
        self._same(got, range(self.batch), tag + " (recovery)")

    def check_flagged(self, placements):
        """placements {member: [Placement]}: return code and total, index, lower bound, isolation, recovery"""
        tag = repr(placements)
        gs = self.poisoned(placements)
        for p in range(self.batch):
            assert must_flag(self.n, self.m, self.N, *[gs[p][k] for k in "ABQR"]) == (p in placements), (p, tag)
        got = self._run(gs)
        grow = got["grow"]
        if got["rc"] != NOT_SPD:
            self.violations.append("%s: solve returned %d, counts grew by %s" % (tag, got["rc"], grow.tolist()))
        if got["failures"] != int(grow.sum()):
            self.violations.append("%s: cholesky_failures() %d, the words grew by %s" % (tag, got["failures"], grow.tolist()))
        for p in range(self.batch):
            want = max(pl.bound for pl in placements[p]) if p in placements else 0
            if (p in placements and grow[p] < want) or (p not in placements and grow[p] != 0):
                self.violations.append("%s: word of member %d grew by %d, expected %s %d"
                                       % (tag, p, grow[p], ">=" if p in placements else "==", want))
        if self.keep and not np.array_equal(got["grow_after"], grow):
            self.violations.append("%s: the re-solves changed the words: %s -> %s" % (tag, grow.tolist(), got["grow_after"].tolist()))
        self._same(got, [p for p in range(self.batch) if p not in placements], tag)
        self.recover(tag)

    def check_unused(self):
        """NaN in A, B, R, r, d of the caller's last knot of the bad members: nothing is reported, nothing changes"""
        placements = {p: unused_placements(self.n, self.m, self.N) for p in bad_members(self.batch)}
        tag = "unused data of knot %d" % (self.N - 1)
        got = self._run(self.poisoned(placements))
        if got["rc"] != 0 or got["failures"] != 0 or got["grow"].any():
            self.violations.append("%s: rc %d, failures %d, counts grew by %s" % (tag, got["rc"], got["failures"], got["grow"].tolist()))
        for p in range(self.batch):
            if not np.array_equal(got["sol"][p], self.base["sol"][p]):
                self.violations.append("%s: solution of member %d differs from the baseline" % (tag, p))
        self.recover(tag)

    def check_isolated_infinity(self):
        """Q_{N-1}[n-1] = 1e-310 in member 1: positive, its reciprocal overflows; it reaches S_{N-2}(n-1, n-1) alone. The
        member is flagged (then everything of check_flagged but the model holds), or its solution is one: finite, with a
        float64 KKT residual of at most REL_TOL ||b||. Returns what happened."""
        pl = Placement("Q", self.N - 1, self.n - 1, 1e-310, 1)
        tag = repr(pl)
        gs = self.poisoned({1: [pl]})
        got = self._run(gs)
        grow = got["grow"]
        flagged = bool(grow[1] >= 1)
        if got["failures"] != int(grow.sum()) or (got["rc"] == NOT_SPD) != (got["failures"] > 0) or got["rc"] not in (0, NOT_SPD):
            self.violations.append("%s: rc %d, cholesky_failures() %d, the words grew by %s" % (tag, got["rc"], got["failures"], grow.tolist()))
        if grow[[p for p in range(self.batch) if p != 1]].any():
            self.violations.append("%s: words of healthy members grew: %s" % (tag, grow.tolist()))
        eta = float("nan")
        if not flagged:
            z = got["sol"][1]
            eta = kkt_relative_residual(gs[1], z) if np.isfinite(z).all() else float("inf")
            if not eta <= REL_TOL:
                self.violations.append("%s: not flagged (rc %d), yet the solution is none: finite %s, KKT residual / |b| = %.3e"
                                       % (tag, got["rc"], bool(np.isfinite(z).all()), eta))
        self._same(got, [p for p in range(self.batch) if p != 1], tag)
        self.recover(tag)
        return dict(flagged=flagged, rc=got["rc"], grow=grow.tolist(), eta=eta)

    def check_all(self, placements):
        """a list of placements, dealt to the bad members: each solve gives every bad member its own (the second member
        walks the list from the other end, so the two differ in knot, field and value)"""
        members = bad_members(self.batch)
        if len(members) == 1:
            for pl in placements:
                self.check_flagged({members[0]: [pl]})
            return
        half = (len(placements) + 1) // 2
        for i in range(half):
            self.check_flagged({members[0]: [placements[i]], members[1]: [placements[len(placements) - 1 - i]]})


def run_case(R, n, m, N, batch, flags, want=None):
    """everything of one case; returns a JSON-able summary (the child-process harnesses print it)"""
    rn = Runner(R, n, m, N, batch, flags)
    out = dict(schedule=rn.schedule, compact1=bool(rn.bs.compact_level1()), paired=bool(rn.bs.level1_paired()))
    if want is not None and rn.schedule != want:
        rn.violations.append("schedule %s, the case claims %s" % (rn.schedule, want))
    elif not rn.violations:
        rn.check_all(dynamics_placements(n, m, N, rn.schedule))
        rn.check_all(weight_placements(n, m, N))
        rn.check_unused()
        out["isolated"] = rn.check_isolated_infinity()
    out["solves"] = rn.solves
    out["violations"] = rn.violations
    rn.close()
    return out
