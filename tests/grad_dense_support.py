"""The nine gradients of dense-cost mode (ndlqr_BatchGradientsDense) restated in numpy, in the flat
column-major layout of the device and with the operation order of strict mode: every matrix entry is
    t1 = a * b (the w factor first), t2 = c * e, s = t1 + t2, out = -s (-0.5 * s for Q, R)
with no contraction (numpy rounds every product and the sum), so the per-problem outputs of a strict-mode solver are
these bits. lam+ = lambda_(k+1):
    gA(i,j) = -(w_lam+[i] z_x[j] + z_lam+[i] w_x[j])    gB(i,j) = -(w_lam+[i] z_u[j] + z_lam+[i] w_u[j])
    gH(i,j) = -(w_x[i] z_u[j] + z_x[i] w_u[j])
    gQ(i,j) = -1/2 (w_x[i] z_x[j] + z_x[i] w_x[j])      gR(i,j) = -1/2 (w_u[i] z_u[j] + z_u[i] w_u[j])
    gq = -w_x    gr = -w_u    gd = -w_lam+    gx0 = -w_lam0
A, B, H, R, r, d of the last knot are zero.

- restate(): dict name -> [batch, N, width] ([batch, n] for x0) from z, w [batch, nvars]; with mags=True also the dict of
  |t1| + |t2| per matrix entry (the scale of the default mode's bound: one contracted against one uncontracted sum).
- ordered_sum(): the batch sum in problem order, 0 + g_0 + g_1 + ...
- fsum(): the exactly rounded batch sum, per entry.
- to_math(): one problem's flat output as the math-convention array of cost_support.gradient_reference.
Test infrastructure.
"""
import math

import numpy as np

NAMES = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
MATRICES = ("A", "B", "Q", "H", "R")
EPS = np.finfo(float).eps
# the host code's constants of the batch split (kernels_grad_dense.hpp: kGradDenseWorkgroups, kGradDenseChunk): a batch sum
# aims at WORKGROUPS workgroups of CHUNK knots at most; a workgroup row takes ceil(batch / nsplit) problems in order
WORKGROUPS = 2048
CHUNK = 8


def blocks(v, n, m, N):
    """[batch, nvars] -> lam [batch, N, n], x [batch, N, n], u [batch, N, m] (u of knot N-1: zero)"""
    v = np.asarray(v, dtype=np.float64)
    full = np.zeros((v.shape[0], N * (2 * n + m)))
    full[:, : v.shape[1]] = v
    V = full.reshape(v.shape[0], N, 2 * n + m)
    return V[:, :, :n], V[:, :, n:2 * n], V[:, :, 2 * n:]


def _next(lam):
    """lambda of the knot after each knot (zero behind the last: those entries are never delivered)"""
    out = np.zeros_like(lam)
    out[:, :-1] = lam[:, 1:]
    return out


def restate(z, w, n, m, N, mags=False):
    zl, zx, zu = blocks(z, n, m, N)
    wl, wx, wu = blocks(w, n, m, N)
    zl1, wl1 = _next(zl), _next(wl)
    out, mag = {}, {}

    def matrix(name, wa, zb, za, wb, half, zero_last):
        # entry (i, j) at i + rows j: [batch, N, j, i]
        t1 = wa[:, :, None, :] * zb[:, :, :, None]
        t2 = za[:, :, None, :] * wb[:, :, :, None]
        s = t1 + t2
        g = -0.5 * s if half else -s
        a = np.abs(t1) + np.abs(t2)
        if zero_last:
            g[:, N - 1] = 0.0
            a[:, N - 1] = 0.0
        out[name] = g.reshape(g.shape[0], N, -1)
        mag[name] = a.reshape(out[name].shape)

    matrix("A", wl1, zx, zl1, wx, False, True)
    matrix("B", wl1, zu, zl1, wu, False, True)
    matrix("Q", wx, zx, zx, wx, True, False)
    matrix("H", wx, zu, zx, wu, False, True)
    matrix("R", wu, zu, zu, wu, True, True)
    out["q"] = -wx
    out["r"] = -wu
    out["d"] = -wl1
    for k in ("r", "d"):
        out[k] = out[k].copy()
        out[k][:, N - 1] = 0.0
    out["x0"] = -wl[:, 0]
    out = {k: np.ascontiguousarray(out[k]) for k in NAMES}
    return (out, mag) if mags else out


def ordered_sum(per):
    """0 + per[0] + per[1] + ... (the order of a workgroup row and of the split pass)"""
    s = np.zeros(per.shape[1:])
    for g in per:
        s = s + g
    return s


def fsum(per):
    """the exactly rounded sum over the leading axis, per entry"""
    flat = per.reshape(per.shape[0], -1)
    return np.array([math.fsum(col) for col in flat.T]).reshape(per.shape[1:])


def rows_of(name, n, m):
    return m if name == "R" else n


def to_math(name, flat, n, m):
    """one problem's [N, width] (or [n]) -> the math-convention array: matrices [N, rows, cols]"""
    if name not in MATRICES:
        return flat
    r = rows_of(name, n, m)
    return flat.reshape(flat.shape[0], flat.shape[1] // r, r).transpose(0, 2, 1)
