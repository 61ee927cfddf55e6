"""Test infrastructure of the read-out of box_certify (ndlqr_CopyBatchInfeasibilityMeasures): a
plain high-precision evaluation of the four numbers the kernel decides on, as a function of the differences of two
consecutive iterates, and a restatement of how the kernel divides a problem into passes, so that the cases of
tests/test_gpu_box_infeas_measures.py can be held to the branches they were chosen for. Nothing here shares code with
the kernel or with box_infeas_support.farkas_check.

The numbers, for dlam [N, n], dmu = (dmu_x | dmu_u) [N, n + m] (zero on the unbounded entries):
    E = max over the knots k and columns j of [A_k | B_k] of |e_kj|,
        e_kj = dmu_kj + sum_i [A_k | B_k]_ij dlam_(k+1),i (k < N - 1) - dlam_kj (j < n)
    D = max |dmu_kj|
    I = max |dmu_kj| over the entries with dmu_kj != 0 whose bound on the side of sign(dmu_kj) is infinite
    S = sum over the other entries with dmu_kj != 0 of bound_kj dmu_kj - x0' dlam_0 - sum_k d_k' dlam_(k+1)

Tolerances (u = 2^-53):
  - D and I are maxima of the fp64 values handed in: exact.
  - E: the kernel forms e_kj by an fma chain of n terms from dmu_kj and one subtraction, n + 1 roundings, each relative
    to a partial sum that is at most a_kj = |dmu_kj| + sum_i |a_ij| |dlam_(k+1),i| + |dlam_kj| in size (up to 1 + O(n u)); the
    long-double evaluation here adds less than one more u a_kj. So |e_dev - e_ref| <= (n + 2) u a_kj per entry, and since
    |max a - max b| <= max |a - b|, |E_dev - E_ref| <= tol_E = max_kj (n + 2) u a_kj.
  - S: every product of two doubles, and their sum, is exact in fractions.Fraction. The kernel adds T terms p_t: TwoProd
    (fma) and TwoSum (dd_add) are exact, so the only roundings are those of the low words, lo <- lo + (e + es), two per
    dd_add. A low word is a sum of errors e <= u |p| and es <= u |partial sum|, so along a chain of L additions (a
    thread's own terms, then the eight levels of the tree) |lo| <= (L + 1) u sum |p_t|, and the 2 L roundings of it add up
    to at most 2 L (L + 1) u^2 sum |p_t| over all chains together. L <= T, and for every shape of the tests L <= 24, so
    this is below T 2^-96 sum |p_t| (T >= 9 there). The final hi + lo rounds once, u |S|, and so does float(S_ref):
    tol_S = 2^-52 |S| + T 2^-96 sum |p_t|.
"""
from fractions import Fraction

import numpy as np

from box_support import masks, matrices

LD = np.longdouble
U = 2.0 ** -53


def measures_reference(prob, bounds, dlam, dmu_x, dmu_u):
    """bounds = (xlo, xhi, ulo, uhi), each [N, n] / [N, m]; dlam, dmu_x [N, n], dmu_u [N, m] in fp64, as the device formed
    them. Returns a dict: E, D, I, S (floats; E and S rounded once from long double / the exact sum), tol_E, tol_S, and
    terms (T) and abs_terms (sum |p_t|) of S."""
    n, m, N = prob.n, prob.m, prob.N
    xlo, xhi, ulo, uhi = [np.asarray(a, dtype=np.float64) for a in bounds]
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    lo = np.concatenate([np.where(Mx > 0, xlo, -np.inf), np.where(Mu > 0, ulo, -np.inf)], axis=1)
    hi = np.concatenate([np.where(Mx > 0, xhi, np.inf), np.where(Mu > 0, uhi, np.inf)], axis=1)
    dl = np.asarray(dlam, dtype=np.float64).reshape(N, n)
    dm = np.concatenate([np.asarray(dmu_x, dtype=np.float64).reshape(N, n),
                         np.asarray(dmu_u, dtype=np.float64).reshape(N, m)], axis=1)
    A, B = matrices(prob)
    AB = np.concatenate([A, B], axis=2)  # [N][n][n + m]: column j of [A_k | B_k] is AB[k][:, j]
    # D and I: exactly as defined
    D = float(np.abs(dm).max())
    side = np.where(dm > 0, hi, lo)
    toward_inf = (dm != 0) & np.isinf(side)
    I = float(np.abs(dm[toward_inf]).max()) if toward_inf.any() else 0.0
    # E, entry by entry in long double, with the bound on the fp64 chain's error
    E, tol_E = LD(0), 0.0
    for k in range(N):
        e = dm[k].astype(LD)
        a = np.abs(dm[k]).astype(LD)
        if k < N - 1:
            e = e + (AB[k].astype(LD) * dl[k + 1].astype(LD)[:, None]).sum(axis=0)
            a = a + (np.abs(AB[k]).astype(LD) * np.abs(dl[k + 1]).astype(LD)[:, None]).sum(axis=0)
        e[:n] = e[:n] - dl[k].astype(LD)
        a[:n] = a[:n] + np.abs(dl[k]).astype(LD)
        E = max(E, np.abs(e).max())
        tol_E = max(tol_E, float((n + 2) * U * a.max()))
    # S, exactly
    terms = []
    for k in range(N):
        for j in range(n + m):
            if dm[k, j] != 0 and not toward_inf[k, j]:
                terms.append(Fraction(float(side[k, j])) * Fraction(float(dm[k, j])))
        rhs = prob.x0 if k == 0 else prob.d[k - 1]
        for i in range(n):
            terms.append(-Fraction(float(rhs[i])) * Fraction(float(dl[k, i])))
    S = sum(terms, Fraction(0))
    abs_terms = float(sum((abs(t) for t in terms), Fraction(0)))
    tol_S = 2.0 ** -52 * abs(float(S)) + len(terms) * 2.0 ** -96 * abs_terms
    return {"E": float(E), "D": D, "I": I, "S": float(S), "tol_E": tol_E, "tol_S": tol_S, "terms": len(terms),
            "abs_terms": abs_terms}


def conditions(ref, eps):
    """the four conditions of the certificate test on the reference's numbers"""
    tol = eps * ref["D"]
    return ref["D"] > 0 and ref["E"] <= tol and ref["I"] <= tol and ref["S"] < -tol


def certify_group(w):
    """knots of a pass (certify_group of kernels_box_infeas.hpp)"""
    return 1 if w >= 256 else 256 // w


def certify_launch(n, m, N):
    """How box_certify walks a problem of this shape: (padded (n, m), w, G, the knots of every pass, the largest dlam
    load nl * n of a pass, the largest task count nk * w of a pass), restated from certify_group and the loops of the
    kernel on the block size the device works on (residual_support.padded_dims)."""
    from residual_support import padded_dims
    pn, pm = padded_dims(n, m, N)
    w = pn + pm
    G = certify_group(w)
    passes, load, tasks = [], 0, 0
    for k0 in range(0, N, G):
        nk = G if k0 + G < N else N - k0
        nl = nk + 1 if k0 + nk < N else nk
        passes.append(nk)
        load = max(load, nl * pn)
        tasks = max(tasks, nk * w)
    return (pn, pm), w, G, passes, load, tasks
