"""Test infrastructure of the active-set polish of the solve with linear inequality rows
(ndlqr_PolishBatchLinConstrained): a numpy restatement of the whole polish of one problem, in
float64 or in longdouble (one code path: `dtype` decides), and an independent direct solve of the active-set system.

One problem at a time: a problem dict of cost_support.py, rows C [N, p, n], D [N, p, m], bounds lo, hi [N, p]. Row codes:
0 unbounded, 1 bounded and inactive, 2 active at lo, 3 active at hi (an equality reports on hi). The packed vectors are
[lam x u] per knot (cost_support.split / join).

- residual(): r_z = b - K z - G_A' mu and r_c = c_A - G_A z on the UNSHIFTED problem, the right-hand side of the
  correction r_z + sigma_p G_A' r_c and the norm max(|r_z|_inf, |r_c|_inf). The device accumulates every row of r_z and
  r_c in double-double and rounds once; the float64 restatement does the same with longdouble rows rounded to float64, the
  longdouble one with exact rational rows rounded to longdouble (a longdouble sum could not judge a double-double one).
- Resolve: the correction K^ delta = rhs on the problem shifted by sigma_p on the active rows. float64: through
  cost_support.reduce of the shifted problem, an LU of the reduced KKT matrix and apply_S / apply_St -- the restatement then
  carries the conditioning of the reduction, as the device does. longdouble: an LU of the shifted matrix refined against
  the longdouble matrix.
- polish_reference(): steps 1-6 of the section.
- active_direct(): the bordered system [[K, G_A'], [G_A, 0]] by cost_support.refined_solve: the independent yardstick.
"""
import warnings
from fractions import Fraction

import numpy as np
import scipy.linalg as sla

import cost_support as cs
import lin_support as ls
from polish_support import initial_codes, sweep_winner  # noqa: F401  (the same exact comparisons; the same rule)

DEFAULT_SIGMA = 1e8  # NDLQR_LIN_POLISH_DEFAULT_SIGMA (test_lin_polish_host.py has the sweep)
DEFAULT_MAX_STEPS = 8
DEFAULT_MAX_ROUNDS = 3
SWEEP_SIGMAS = [1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8]
SHAPES = [(6, 3), (12, 4), (7, 9), (20, 5)]
HORIZONS = [2, 5, 8, 16]
CASES = [(n, m, N) for (n, m) in SHAPES for N in HORIZONS]
ADMM_EPS = 1e-3
STATUS1_CAP = 42  # of the 48 problems of CASES at least this many end as status 1


def bounded(lo, hi):
    return np.isfinite(lo) | np.isfinite(hi)


def sigma_of(p, C, D, lo, hi, sigma):
    """sigma_p = (sigma x the largest entry of diag Q, diag R) / g2, g2 the largest squared row norm of the bounded rows of
    [C D] (R, D of the last knot left out), every product and sum rounded on its own, j ascending, C before D; a problem
    without a bounded row: g2 = 1"""
    n, m, N = cs.dims(p)
    big = 0.0
    for a in (np.einsum("kii->ki", p["Q"]), np.einsum("kii->ki", p["R"][: N - 1])):
        for val in np.asarray(a, dtype=np.float64).reshape(-1):
            big = val if (val > big or val != val) else big
    s = np.zeros(lo.shape)
    for j in range(n):
        s = s + C[:, :, j] * C[:, :, j]
    for j in range(m):
        t = D[:, :, j] * D[:, :, j]
        t[N - 1] = 0.0
        s = np.where(np.arange(N)[:, None] < N - 1, s + t, s)
    g2 = 0.0
    for val in s[bounded(lo, hi)].reshape(-1):
        g2 = val if (val > g2 or val != val) else g2
    return (sigma * big) / (g2 if g2 > 0.0 else 1.0)


def weighted_problem(p, C, D, weight, dtype=np.float64):
    """the problem dict with Q + C' W C, H + C' W D, R + D' W D, W = diag(weight [N, p]) (knot N-1: Q alone), in `dtype`"""
    n, m, N = cs.dims(p)
    out = {k: np.asarray(p[k], dtype=dtype).copy() for k in cs.NAMES}
    Cd, Dd, W = C.astype(dtype), D.astype(dtype), weight.astype(dtype)
    for k in range(N):
        CM = Cd[k].T * W[k]
        out["Q"][k] = 0.5 * (out["Q"][k] + out["Q"][k].T) + CM @ Cd[k]
        if k < N - 1:
            out["H"][k] = out["H"][k] + CM @ Dd[k]
            out["R"][k] = 0.5 * (out["R"][k] + out["R"][k].T) + (Dd[k].T * W[k]) @ Dd[k]
    return out


class Resolve:
    """delta = K^-1 rhs of the problem shifted by sig on the rows with code >= 2"""

    def __init__(self, p, C, D, codes, sig, dtype):
        self.dtype = dtype
        ps = weighted_problem(p, C, D, np.where(codes >= 2, sig, 0.0), dtype)
        if dtype == np.float64:
            self.red = cs.reduce(ps)
            Kt, _ = cs.dense_kkt(cs.reduced_problem(self.red))
            self.lu = sla.lu_factor(Kt)
        else:
            self.solver = ls.Solver(ls.kkt_ld(ps)[0])

    def __call__(self, rhs):
        if self.dtype == np.float64:
            return cs.apply_S(self.red, sla.lu_solve(self.lu, cs.apply_St(self.red, rhs)))
        return self.solver(rhs)


class System:
    """K, b of the unshifted problem in `dtype`, and the residual of the active-set system"""

    def __init__(self, p, C, D, lo, hi, dtype):
        self.p, self.C, self.D, self.dtype = p, C, D, dtype
        self.lo, self.hi = lo.astype(dtype), hi.astype(dtype)
        # (the rows are accumulated beyond `dtype` and rounded to it once: float64 from longdouble sums, as the device
        #  rounds its double-double sums; longdouble from exact rational sums -- every input is a float64 --, so that
        #  the yardstick is better than what it measures)
        self.K, self.b = ls.kkt_ld({k: np.asarray(p[k], dtype=np.longdouble) for k in cs.NAMES})
        self.exact = None
        if dtype == np.longdouble:
            n, m, N = cs.dims(p)
            zb, nv = 2 * n + m, self.b.size
            G = np.zeros((N * C.shape[1], nv))
            for k in range(N):
                for r in range(C.shape[1]):
                    G[k * C.shape[1] + r, k * zb + n:k * zb + 2 * n] = C[k, r]
                    if k < N - 1:
                        G[k * C.shape[1] + r, k * zb + 2 * n:k * zb + 2 * n + m] = D[k, r]
            frac = lambda a: Fraction(float(a))
            K64 = np.asarray(self.K, dtype=np.float64)
            assert (K64.astype(np.longdouble) == self.K).all()  # (float64 data: nothing is lost)
            self.exact = dict(K=[[(j, frac(row[j])) for j in np.flatnonzero(row)] for row in K64],
                              G=[[(j, frac(row[j])) for j in np.flatnonzero(row)] for row in G],
                              Gt=[[(e, frac(col[e])) for e in np.flatnonzero(col)] for col in G.T],
                              b=[frac(v) for v in self.b])

    @staticmethod
    def _ld(fr):
        """a Fraction rounded to longdouble (two float64 pieces: 106 bits before the last rounding)"""
        hi = float(fr)
        return np.longdouble(hi) + np.longdouble(float(fr - Fraction(hi)))

    @staticmethod
    def _fr(v):
        """a longdouble as a Fraction, exactly (two float64 pieces hold its 64 bits)"""
        hi = float(v)
        return Fraction(hi) + Fraction(float(v - np.longdouble(hi)))

    def _exact_rows(self, act, c, z, mu):
        """(r_z, r_c) as longdouble arrays from exact rational sums"""
        X = self.exact
        zf = [self._fr(v) for v in z]
        mf = [self._fr(v) for v in mu.reshape(-1)]
        r_z = [X["b"][i] - sum(a * zf[j] for j, a in X["K"][i]) - sum(a * mf[e] for e, a in X["Gt"][i]) for i in range(len(zf))]
        cf = [Fraction(float(v)) for v in c.reshape(-1)]
        r_c = [cf[e] - sum(a * zf[j] for j, a in X["G"][e]) if on else Fraction(0) for e, on in enumerate(act.reshape(-1))]
        return (np.array([self._ld(v) for v in r_z], dtype=np.longdouble),
                np.array([self._ld(v) for v in r_c], dtype=np.longdouble).reshape(act.shape))

    def residual(self, codes, sig, z, mu):
        """(rhs of the correction, norm, |r_c|_inf, r_z, r_c)"""
        act = codes >= 2
        LD = np.longdouble
        z = np.asarray(np.asarray(z, dtype=self.dtype), dtype=LD)
        mu = np.where(act, np.asarray(np.asarray(mu, dtype=self.dtype), dtype=LD), 0).astype(LD)
        c = np.where(codes == 3, self.hi, np.where(codes == 2, self.lo, 0)).astype(LD)
        with np.errstate(invalid="ignore", over="ignore"):
            if self.exact is not None and np.isfinite(z.astype(np.float64)).all() and np.isfinite(mu.astype(np.float64)).all():
                r_z, r_c = self._exact_rows(act, c, z, mu)
            else:
                r_z = (self.b - self.K @ z - ls.perturbation(self.p, self.C, self.D, mu)).astype(self.dtype)
                r_c = np.where(act, c - ls.rows_of(self.p, self.C, self.D, z), 0).astype(self.dtype)
            rhs = r_z + self.dtype(sig) * ls.perturbation(self.p, self.C, self.D, r_c)
        nz = np.abs(r_z).max()
        nc = np.abs(r_c).max() if r_c.size else self.dtype(0)
        nan = not (np.isfinite(float(nz)) and np.isfinite(float(nc)))
        norm = self.dtype(np.nan) if nan else max(nz, nc)
        return rhs, norm, nc, r_z, r_c


def polish_reference(p, C, D, lo, hi, z0, v, y, rho, sigma=0.0, max_steps=0, max_rounds=0, forward_status=1,
                     dtype=np.float64, trace=None):
    """The polish of DESIGN.md section 3.23 on one problem. z0: the resident (ADMM) solution, packed; v, y [N, p]: the ADMM
    iterate; rho: the problem's final penalty. Returns a dict: z (packed), mu, codes [N, p], sig (sigma_p, float64), steps,
    status, rounds (the factorisations), v, y (what a warm start finds), norms (per round: the norms of its slots), norm
    and rc (max(|r_z|, |r_c|) and |r_c|_inf of the last accepted iterate). trace: a list that gets one dict per formed candidate (round, step, z, mu, norm)."""
    n, m, N = cs.dims(p)
    sigma = sigma if sigma > 0.0 else DEFAULT_SIGMA
    max_steps = max_steps or DEFAULT_MAX_STEPS
    max_rounds = 0 if max_rounds < 0 else (max_rounds or DEFAULT_MAX_ROUNDS)  # (negative: no correction round)
    M = bounded(lo, hi)
    v64, y64 = np.asarray(v, dtype=np.float64), np.asarray(y, dtype=np.float64)
    codes = initial_codes(lo, hi, M, v64, y64)
    sig = sigma_of(p, C, D, lo, hi, sigma)
    out = dict(z=np.asarray(z0, dtype=dtype), mu=(rho * y64).astype(dtype), v=v64, y=y64, steps=0, rounds=0, norms=[], sig=sig,
               codes=codes, rc=None, norm=None)
    if forward_status in (3, 4):
        out["status"] = 3 if forward_status == 3 else 2
        return out
    system = System(p, C, D, lo, hi, dtype)
    lo_, hi_ = system.lo, system.hi
    z = np.asarray(z0, dtype=dtype).copy()
    mu = np.where(codes >= 2, dtype(rho) * y64.astype(dtype), 0).astype(dtype)
    sg = dtype(sig)
    steps, status = 0, 2
    for rnd in range(max_rounds + 1):
        out["rounds"] = rnd + 1
        act = codes >= 2
        resolve = Resolve(p, C, D, codes, sig, dtype)
        rhs, norm, nc, _, r_c = system.residual(codes, sig, z, mu)
        norms, here = [norm], 0
        for step in range(1, max_steps + 1):
            delta = np.asarray(resolve(rhs), dtype=dtype)
            with np.errstate(invalid="ignore", over="ignore"):
                zc = z + delta
                t = ls.rows_of(p, C, D, delta) - r_c
                t = sg * t
                muc = np.where(act, mu + t, 0).astype(dtype)
            if not (np.isfinite(zc.astype(np.float64)).all() and np.isfinite(muc.astype(np.float64)).all()):
                out.update(status=3, codes=codes)
                return out
            rhs_c, normc, ncc, _, r_cc = system.residual(codes, sig, zc, muc)
            norms.append(normc)
            if trace is not None:
                trace.append(dict(round=rnd, step=step, z=zc.copy(), mu=muc.copy(), norm=normc))
            if not normc < norm:
                break
            z, mu, rhs, norm, nc, r_c = zc, muc, rhs_c, normc, ncc, r_cc
            here += 1
        out["norms"].append(norms)
        steps += here
        # validation of the last accepted iterate, exact comparisons
        w = ls.rows_of(p, C, D, z)
        wrong3 = (codes == 3) & (lo < hi) & (mu < 0)
        wrong2 = (codes == 2) & (mu > 0)
        above = (codes == 1) & (w > hi_)
        below = (codes == 1) & (w < lo_)
        valid = not (wrong3.any() or wrong2.any() or above.any() or below.any())
        if valid or rnd == max_rounds:
            status = 1 if valid and here >= 1 else 2
            out["rc"], out["norm"] = nc, norm
            break
        codes = np.where(wrong3 | wrong2, 1, np.where(above, 3, np.where(below, 2, codes))).astype(np.int8)
        mu = np.where(wrong3 | wrong2 | above | below, 0, mu).astype(dtype)
    out.update(codes=codes, steps=steps, status=status)
    if status == 1:
        w = ls.rows_of(p, C, D, z)
        out.update(z=z, mu=mu, v=np.where(M, np.minimum(np.maximum(w, lo_), hi_), v64.astype(dtype)),
                   y=np.where(M, mu / dtype(rho), y64.astype(dtype)))
    return out


def active_direct(p, C, D, lo, hi, codes):
    """(z packed, mu [N, p]) of K z + G_A' mu = b, G_A z = c_A: the bordered system by cost_support.refined_solve. None
    when the active rows are linearly dependent (a pivot of the LU below 1e-12 of the largest): the system is singular and
    there is no yardstick."""
    n, m, N = cs.dims(p)
    K, b = cs.dense_kkt(p)
    nv = b.size
    idx = [(k, r) for k in range(N) for r in range(C.shape[1]) if codes[k, r] >= 2]
    G = np.zeros((len(idx), nv))
    c = np.zeros(len(idx))
    zb = 2 * n + m
    for i, (k, r) in enumerate(idx):
        G[i, k * zb + n:k * zb + 2 * n] = C[k, r]
        if k < N - 1:
            G[i, k * zb + 2 * n:k * zb + 2 * n + m] = D[k, r]
        c[i] = hi[k, r] if codes[k, r] == 3 else lo[k, r]
    big = np.block([[K, G.T], [G, np.zeros((len(idx), len(idx)))]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        piv = np.abs(np.diag(sla.lu_factor(big)[0]))
    if piv.min() <= 1e-12 * piv.max():
        return None
    sol = cs.refined_solve(big, np.concatenate([b, c]))
    mu = np.zeros(lo.shape)
    for i, (k, r) in enumerate(idx):
        mu[k, r] = sol[nv + i]
    return sol[:nv], mu


def stationarity_ld(p, C, D, z, mu):
    """|K z - b + G' mu|_inf in longdouble"""
    pl = {k: np.asarray(p[k], dtype=np.longdouble) for k in cs.NAMES}
    K, b = ls.kkt_ld(pl)
    s = K @ np.asarray(z, dtype=np.longdouble) - b + ls.perturbation(p, C, D, np.asarray(mu, dtype=np.longdouble))
    return float(np.abs(s).max())


_STARTS = {}


def admm_start(n, m, N, eps=ADMM_EPS, max_iter=2000):
    """per problem of lin_support.case(n, m, N): the float64 restatement's ADMM at `eps` (dict of lin_support.admm);
    shared and read-only"""
    key = (n, m, N, eps, max_iter)
    if key not in _STARTS:
        out = []
        for c in ls.case(n, m, N):
            a = ls.admm(c["p"], c["C"], c["D"], c["lo"], c["hi"], eps_abs=eps, eps_rel=eps, max_iter=max_iter)
            for k in ("z", "v", "y", "mu"):
                a[k].setflags(write=False)
            out.append(a)
        _STARTS[key] = out
    return _STARTS[key]


def polish_case(n, m, N, i, **kw):
    """polish_reference of problem i of the case from its admm_start"""
    c, a = ls.case(n, m, N)[i], admm_start(n, m, N)[i]
    return polish_reference(c["p"], c["C"], c["D"], c["lo"], c["hi"], a["z"], a["v"], a["y"], ls.RHO,
                            forward_status=a["status"], **kw)


def sigma_sweep(cases=CASES, sigmas=SWEEP_SIGMAS):
    """rows (sigma, total steps, worst ratio of the final stationarity to that of active_direct on the same final set -- both
    evaluated in longdouble --, at least STATUS1_CAP problems ended as status 1, their count) over `cases`, each from
    ADMM at ADMM_EPS, default steps and rounds. A problem whose final active rows are linearly dependent (active_direct:
    None) has no yardstick and stays out of the ratio."""
    runs = {sg: [] for sg in sigmas}
    for (n, m, N) in cases:
        for i, c in enumerate(ls.case(n, m, N)):
            for sg in sigmas:
                o = polish_case(n, m, N, i, sigma=sg)
                ratio = 0.0
                direct = active_direct(c["p"], c["C"], c["D"], c["lo"], c["hi"], o["codes"]) if o["status"] == 1 else None
                if direct is not None:
                    zt, mt = direct
                    mine = stationarity_ld(c["p"], c["C"], c["D"], o["z"], o["mu"])
                    ratio = mine / max(stationarity_ld(c["p"], c["C"], c["D"], zt, mt), np.finfo(float).tiny)
                runs[sg].append((o["status"], o["steps"], ratio))
    rows = []
    for sg in sigmas:
        ones = [r for r in runs[sg] if r[0] == 1]
        rows.append((sg, sum(r[1] for r in runs[sg]), max([r[2] for r in ones], default=0.0), len(ones) >= STATUS1_CAP, len(ones)))
    return rows
