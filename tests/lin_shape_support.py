"""Test infrastructure of the launch-class tests of the linear-inequality kernels (kernels_lin.hpp, kernels_lin_infeas.hpp;
tests/test_gpu_lin_shapes.py, tests/test_lin_shapes_host.py; DESIGN.md sections 3.17, 3.19, 3.20). numpy only.

- CASES and TABLE: the ten shapes (n, m, p, N) and the loop classes each was chosen for, written down by hand;
  launch_classes() restates the same classes from the kernels' loop bounds alone, and the host test holds one to the other.

      case (n, m, p, N)   row passes   column passes   lin_multipliers groups   G    lin_certify passes (nk / nl)   chosen for
      (6, 3, 1, 2)        1            1               1                        28   2 / 2                          one row, two knots: waves 2-3 and 63 lanes idle
      (12, 4, 64, 8)      1 (exact)    1               2 (exact)                16   8 / 8                          N p = 512; nk p = 512: strided dmu load
      (12, 4, 65, 5)      2 (tail 1)   1               2                        16   5 / 5                          padded horizon (5 -> 8), one-row second pass
      (6, 3, 130, 8)      3 (tail 2)   1               5                        28   8 / 8                          p far above n + m; N p = 1040
      (12, 4, 6, 32)      1            1               1                        16   16 / 17, 16 / 16               the knot behind the first pass; 8 knots a wavefront
      (12, 4, 6, 20)      1            1               1                        16   16 / 17, 4 / 4                 horizon padded 20 -> 32
      (13, 4, 6, 16)      1            1               1                        15   15 / 16, 1 / 1                 a tail pass of one knot
      (20, 5, 7, 16)      1            1               1                        10   10 / 11, 6 / 6                 passes of 10 + 6
      (40, 2, 8, 8)       1            1               1                        6    6 / 7, 2 / 2                   dlam load 7 * 40 = 280 > 256; n > 32
      (48, 20, 8, 4)      1            2 (tail 4)      1                        3    3 / 4, 1 / 1                   n + m = 68: two column passes of lin_next_rhs

  A class with n + m >= 256 (G = 1 by the clamp of lin_certify_group) cannot exist: the records of such a knot alone are
  beyond the LDS of a workgroup, and ndlqr_hip_init_constrained refuses the shape by name (the host test asserts the
  formula for every split of 256).
- dense_rows(): p dense rows per knot with seeded entries, in the "two_sided" or the "mixed" bound pattern.
- batch(): the shared, read-only problems, rows and float64 iterates of one (case, pattern).
- update_reference() / update_bars(): one ADMM update in numpy.longdouble as a function of its inputs, the sums of absolute
  terms its rounding bounds are made of, and the bounds.
- row_classes(), certificate_inputs(): what the input conditions of the host test are read from.
"""
import functools

import numpy as np

import cost_support as cs
import lin_adaptive_support as las
import lin_support as ls

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
RHO, ALPHA = ls.RHO, ls.ALPHA
LDS_LIMIT = 160 * 1024
K_UPDATE, K_CERTIFY, ADAPT_EVERY, ADAPT_ITERS = 3, 4, 2, 3
PATTERNS = ("two_sided", "mixed")

CASES = [(6, 3, 1, 2), (12, 4, 64, 8), (12, 4, 65, 5), (6, 3, 130, 8), (12, 4, 6, 32), (12, 4, 6, 20), (13, 4, 6, 16),
         (20, 5, 7, 16), (40, 2, 8, 8), (48, 20, 8, 4)]
TALL = [c for c in CASES if c[2] >= 64]        # the cases of part a (with WIDE) ...
WIDE = (48, 20, 8, 4)
ADAPT_CASES = [(12, 4, 65, 5), (6, 3, 130, 8)]  # ... and of part e

# the table above as data: row passes, rows of the last row pass, column passes, columns of the last, workgroups of
# lin_multipliers per problem, G, the passes of lin_certify as (nk, nl), the largest dlam and dmu load of a pass
TABLE = {
    (6, 3, 1, 2): dict(row_passes=1, row_tail=1, col_passes=1, col_tail=9, groups=1, G=28, passes=[(2, 2)], dlam=12, dmu=2),
    (12, 4, 64, 8): dict(row_passes=1, row_tail=64, col_passes=1, col_tail=16, groups=2, G=16, passes=[(8, 8)], dlam=96, dmu=512),
    (12, 4, 65, 5): dict(row_passes=2, row_tail=1, col_passes=1, col_tail=16, groups=2, G=16, passes=[(5, 5)], dlam=60, dmu=325),
    (6, 3, 130, 8): dict(row_passes=3, row_tail=2, col_passes=1, col_tail=9, groups=5, G=28, passes=[(8, 8)], dlam=48, dmu=1040),
    (12, 4, 6, 32): dict(row_passes=1, row_tail=6, col_passes=1, col_tail=16, groups=1, G=16, passes=[(16, 17), (16, 16)],
                         dlam=204, dmu=96),
    (12, 4, 6, 20): dict(row_passes=1, row_tail=6, col_passes=1, col_tail=16, groups=1, G=16, passes=[(16, 17), (4, 4)],
                         dlam=204, dmu=96),
    (13, 4, 6, 16): dict(row_passes=1, row_tail=6, col_passes=1, col_tail=17, groups=1, G=15, passes=[(15, 16), (1, 1)],
                         dlam=208, dmu=90),
    (20, 5, 7, 16): dict(row_passes=1, row_tail=7, col_passes=1, col_tail=25, groups=1, G=10, passes=[(10, 11), (6, 6)],
                         dlam=220, dmu=70),
    (40, 2, 8, 8): dict(row_passes=1, row_tail=8, col_passes=1, col_tail=42, groups=1, G=6, passes=[(6, 7), (2, 2)],
                        dlam=280, dmu=48),
    (48, 20, 8, 4): dict(row_passes=1, row_tail=8, col_passes=2, col_tail=4, groups=1, G=3, passes=[(3, 4), (1, 1)],
                         dlam=192, dmu=24),
}

# Seeds of the rows per (case, pattern), one per problem, and the fraction of the rows >= 64: chosen on the CPU so that
# the input conditions of test_lin_shapes_host.py hold for every problem (the default: 500 + i and FRACTION)
FRACTION = 0.6
ROW_SEEDS = {((12, 4, 65, 5), "two_sided"): (500, 500, 501), ((12, 4, 65, 5), "mixed"): (500, 504, 505)}
# (at 0.6 the single row 64 of (12,4,65,5) is on a bound at none or one of its five knots; at (6,3,130,8) one problem of
#  three has no row >= 64 on its lower bound)
TAIL_FRACTION = {((12, 4, 65, 5), "two_sided"): 0.15, ((12, 4, 65, 5), "mixed"): 0.15,
                 ((6, 3, 130, 8), "two_sided"): 0.3, ((6, 3, 130, 8), "mixed"): 0.3}


# ------------------------------------------------------------------------------------------------ the launcher, restated

def lin_wave_lds(n, m, p):
    """doubles one wavefront of lin_update stages for its knot: L, L_R (odd leading dimensions), G, C, D, and the vectors
    lambda | x | u~ | u | three row vectors"""
    return n * (n | 1) + m * (m | 1) + m * n + p * n + p * m + 2 * n + 2 * m + 3 * p


def lds_bytes(n, m, p):
    """LDS of a workgroup of lin_update: four wavefronts' staging, the five maxima of 256 threads, two words"""
    return 8 * 4 * lin_wave_lds(n, m, p) + 8 * 5 * 256 + 16


def launch_classes(n, m, p, N):
    """the loop classes of a case from the kernels' loop bounds alone (the keys of TABLE, and `lds`)"""
    w = n + m
    G = 1 if w >= 256 else 256 // w
    passes, k0 = [], 0
    while k0 < N:
        nk = G if k0 + G < N else N - k0
        nl = nk + 1 if k0 + nk < N else nk
        passes.append((nk, nl))
        k0 += G
    return dict(row_passes=-(-p // 64), row_tail=p - 64 * ((p - 1) // 64), col_passes=-(-w // 64), col_tail=w - 64 * ((w - 1) // 64),
                groups=-(-(N * p) // 256), G=G, passes=passes, dlam=max(nl * n for _, nl in passes),
                dmu=max(nk * p for nk, _ in passes), lds=lds_bytes(n, m, p))


# ------------------------------------------------------------------------------------------------ rows and bounds

def row_kind(N, p):
    """(k + r) % 4 over knot k and row r, [N, p]: 0 bounded on both sides, 1 above only, 2 below only, 3 not at all"""
    return (np.arange(N)[:, None] + np.arange(p)[None, :]) % 4


def pinned_row(N, p):
    """(k, r) of the row of the mixed pattern that gets lo == hi: the first two-sided one in knot order"""
    k, r = np.argwhere(row_kind(N, p) == 0)[0]
    return int(k), int(r)


def dense_rows(problem, z_unc, p, seed, pattern, fraction=FRACTION, tail_fraction=None):
    """(C [N, p, n], D [N, p, m], lo, hi [N, p]) for the problem whose unconstrained solution is z_unc: entries
    N(0,1)/sqrt(n) and N(0,1)/sqrt(m); bounds +-fraction x the largest |w| of the unconstrained solution per row, over the
    knots (lin_support.constraint_rows), the rows >= 64 with tail_fraction instead where given. pattern "two_sided":
    every row as it is. "mixed": by row_kind() both bounds, the upper one alone, the lower one alone or none, and the row
    pinned_row() gets lo == hi == half its upper bound."""
    assert pattern in PATTERNS
    n, m, N = cs.dims(problem)
    rng = np.random.default_rng([seed, n, m, N, p, 23])
    C = rng.standard_normal((N, p, n)) / np.sqrt(n)
    D = rng.standard_normal((N, p, m)) / np.sqrt(m)
    w = ls.rows_of(problem, C, D, np.asarray(z_unc, dtype=np.float64))
    frac = np.full(p, float(fraction))
    if tail_fraction is not None:
        frac[64:] = tail_fraction
    hi = np.broadcast_to(frac * np.abs(w).max(axis=0), (N, p)).copy()
    lo = -hi
    if pattern == "mixed":
        kind = row_kind(N, p)
        k, r = pinned_row(N, p)
        pin = 0.5 * hi[k, r]
        lo[(kind == 1) | (kind == 3)] = -np.inf
        hi[(kind == 2) | (kind == 3)] = np.inf
        lo[k, r] = hi[k, r] = pin
    return C, D, lo, hi


def bounded(lo, hi):
    return np.isfinite(lo) | np.isfinite(hi)


@functools.lru_cache(maxsize=None)
def batch(case, pattern):
    """The shared, read-only batch of one (case, pattern): per problem of cost_support.family(n, m, N, "moderate") a dict
    p, C, D, lo, hi and `its`, the first K_CERTIFY iterates of the float64 restatement lin_support.admm (it, z, v, y,
    resid), eps = 1e-300."""
    n, m, p, N = case
    fam = cs.family(n, m, N, "moderate")
    seeds = ROW_SEEDS.get((case, pattern), tuple(500 + i for i in range(cs.BATCH)))
    out = []
    for i, prob in enumerate(fam["probs"]):
        C, D, lo, hi = dense_rows(prob, fam["z"][i], p, seeds[i], pattern, tail_fraction=TAIL_FRACTION.get((case, pattern)))
        its = []
        ls.admm(prob, C, D, lo, hi, eps_abs=1e-300, eps_rel=1e-300, max_iter=K_CERTIFY, trace=its)
        for a in (C, D, lo, hi):
            a.setflags(write=False)
        out.append(dict(p=prob, C=C, D=D, lo=lo, hi=hi, its=its))
    return out


def released_bounds(lo, hi):
    """the bounds of the second warm start of part c: the rows >= 64 -- without such rows, the last row -- unbounded at
    the even knots (copies). The pattern changes: the solve factors again, and lin_start zeroes y there."""
    lo, hi = lo.copy(), hi.copy()
    first = 64 if lo.shape[1] > 64 else lo.shape[1] - 1
    lo[0::2, first:] = -np.inf
    hi[0::2, first:] = np.inf
    return lo, hi


def row_classes(lo, hi, v, rows=slice(None)):
    """among the rows `rows` (all knots): how many bounded entries with lo < hi have v on lo / on hi / strictly inside, and
    how many entries are unbounded: (on_lo, on_hi, inside, unbounded)"""
    lo, hi, v = lo[:, rows], hi[:, rows], np.asarray(v)[:, rows]
    M = bounded(lo, hi)
    open_ = M & (lo < hi)
    return (int((open_ & (v == lo)).sum()), int((open_ & (v == hi)).sum()), int((open_ & (v > lo) & (v < hi)).sum()),
            int((~M).sum()))


def certificate_inputs(c, rho=RHO):
    """(dlam [N, n], dmu [N, p]) a check at K_CERTIFY judges, from the float64 iterates of a batch() entry"""
    n, m, N = cs.dims(c["p"])
    a, b = c["its"][K_CERTIFY - 2], c["its"][K_CERTIFY - 1]
    return cs.split(b["z"], n, m, N)[0] - cs.split(a["z"], n, m, N)[0], rho * b["y"] - rho * a["y"]


@functools.lru_cache(maxsize=None)
def adaptive_runs(case):
    """Part e, per problem of batch(case, "mixed"): the float64 restatement with the penalty rule evaluated at iteration
    ADAPT_EVERY of ADAPT_ITERS (the rule is never evaluated at the last iteration of a solve): dict run (lin_adaptive_support
    .admm_adaptive), its (its trace with the iterates), margin (the decision margin of lin_adaptive_support.margin)."""
    out = []
    for c in batch(case, "mixed"):
        its = []
        run = las.admm_adaptive(c["p"], c["C"], c["D"], c["lo"], c["hi"], eps_abs=1e-300, eps_rel=1e-300, max_iter=ADAPT_ITERS,
                                every=ADAPT_EVERY, trace=its, iterates=True)
        out.append(dict(run=run, its=its, margin=las.margin(its)))
    return out


# ------------------------------------------------------------------------------------------------ one update, restated

def update_reference(prob, C, D, x, u, v0, y0, lo, hi, rho, alpha, vn_read=None, yn_read=None):
    """One ADMM update in longdouble as a function of its inputs: the iterate x [N, n], u [N, m]
    in the caller's variables, v0, y0 [N, p] of the iteration before, the bounds, rho and alpha (1 - alpha formed once in
    double, as the host does). Returns a dict:
      w, vn, yn [N, p]        C x + D u (the last knot: C x), v+ and y+ (0 on the unbounded rows);
      resid                   (r_prim, r_dual, s_prim, s_dual). r_dual = rho max |G'M(v+ - v0)| and s_dual = rho max |G'M y+|
                              are those of the read-out values vn_read, yn_read where given (the device forms v+ - v0 with one
                              double subtraction, as numpy does: the same bits), else of this update's own;
      w_scale [N, p]          |C||x| + |D||u|, the sum of absolute terms of w;
      t_scale [N, p]          alpha w_scale + |1 - alpha||v0| + |y0|, that of wh + y0;
      rd_scale, sd_scale      the largest sum of absolute terms of an entry of G'M(v+ - v0) and of G'M y+;
      M                       the bounded rows."""
    n, m, N = cs.dims(prob)
    M = bounded(lo, hi)
    Cl, Dl = np.asarray(C, dtype=LD), np.asarray(D, dtype=LD)
    xl, ul = np.asarray(x, dtype=LD), np.asarray(u, dtype=LD)
    v0l, y0l = np.asarray(v0, dtype=LD), np.asarray(y0, dtype=LD)
    al, oma = LD(alpha), LD(1.0 - alpha)
    w = np.einsum("krj,kj->kr", Cl, xl)
    w_scale = np.einsum("krj,kj->kr", np.abs(Cl), np.abs(xl))
    w[: N - 1] += np.einsum("krj,kj->kr", Dl[: N - 1], ul[: N - 1])
    w_scale[: N - 1] += np.einsum("krj,kj->kr", np.abs(Dl[: N - 1]), np.abs(ul[: N - 1]))
    wh = al * w + oma * v0l
    t = wh + y0l
    vn = np.where(M, np.minimum(np.maximum(t, lo.astype(LD)), hi.astype(LD)), 0).astype(LD)
    yn = np.where(M, t - vn, 0).astype(LD)
    t_scale = al * w_scale + abs(oma) * np.abs(v0l) + np.abs(y0l)
    mx = lambda a: LD(np.abs(a).max()) if a.size else LD(0)
    # (the read-out values: float64 arithmetic on purpose, to have the kernel's M (v+ - v0) bit for bit)
    t1 = np.where(M, np.asarray(vn_read, dtype=np.float64) - np.asarray(v0, dtype=np.float64), 0.0).astype(LD) \
        if vn_read is not None else np.where(M, vn - v0l, 0).astype(LD)
    t2 = np.where(M, np.asarray(yn_read, dtype=np.float64), 0.0).astype(LD) if yn_read is not None else yn
    rho_ = LD(rho)
    absCD = (np.abs(C), np.abs(D))
    resid = (mx((w - vn)[M]), rho_ * mx(ls.perturbation(prob, C, D, t1)), max(mx(w[M]), mx(vn[M])),
             rho_ * mx(ls.perturbation(prob, C, D, t2)))
    return dict(w=w, vn=vn, yn=yn, t=t, resid=resid, w_scale=w_scale, t_scale=t_scale, M=M,
                rd_scale=mx(ls.perturbation(prob, *absCD, np.abs(t1))), sd_scale=mx(ls.perturbation(prob, *absCD, np.abs(t2))))


def update_bars(ref, n, m, p, rho):
    """The rounding bounds of the device's update against update_reference(), from the operation counts and the sums of
    absolute terms (the derivation is in the docstring of test_gpu_lin_shapes.py). A dict: w, t (also that of v+), y
    [N, p], and resid (4)."""
    bw = (n + m + 2) * EPS * ref["w_scale"]
    bt = float(ALPHA) * bw + 2 * EPS * ref["t_scale"]
    by = 2 * bt + EPS * np.abs(ref["yn"])
    M = ref["M"]
    mx = lambda a: LD(a[M].max()) if M.any() else LD(0)
    br = (mx(bw + bt + EPS * (np.abs(ref["w"]) + np.abs(ref["vn"]))), (p + 3) * EPS * LD(rho) * ref["rd_scale"],
          max(mx(bw), mx(bt)), (p + 3) * EPS * LD(rho) * ref["sd_scale"])
    return dict(w=bw, t=bt, y=by, resid=br)


def kkt_residual(prob, C, D, lo, hi, rho, z, v, y):
    """(largest |K^ z - rhs|, ||rhs||_inf) in longdouble with K^, b^ of the problem shifted by rho C'MC, rho C'MD, rho D'MD
    and rhs = b^ - [C'; D'] rho M (y - v): what the re-solve behind an update that left (v, y) solves"""
    M = bounded(lo, hi)
    K, b = ls.kkt_ld(ls.shifted_problem(prob, C, D, lo, hi, rho, LD))
    t = np.where(M, LD(rho) * (np.asarray(y, dtype=LD) - np.asarray(v, dtype=LD)), 0).astype(LD)
    rhs = b - ls.perturbation(prob, C, D, t)
    return float(np.abs(K @ np.asarray(z, dtype=LD) - rhs).max()), float(np.abs(rhs).max())
