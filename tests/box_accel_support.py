"""Reference for the safeguarded Anderson acceleration of the box-constrained batch solve (ndlqr_BatchSetBoxAcceleration;
DESIGN.md section 3.15).

- cholesky_solve(): the regularised normal equations of one accelerated step, in Python floats and in the operation
  order of the kernel's thread 0 (no fused multiply-add), or None where a pivot is not positive or a coefficient is not
  finite.
- admm_accel_reference(): box_adaptive_support.admm_adaptive_reference (and with it box_support.admm_reference) with the
  rule of section 3.15 per problem over its bounded entries, each solve by a caller-given solver, every element-wise
  operation in the order of strict mode. The dot products -- the only sums over entries the rule adds -- run in the
  order of the kernel's fixed reduction (tree_dot), so that strict mode is reproduced down to the sums, or with the
  products permuted first (`perm`, a permutation of range(number of bounded entries)): the difference between two
  orders is what a result may depend on the order of its sums by.
  With `infeas_every` it runs the certificate test of section 3.14 (box_infeas_support.farkas_check) at the check
  iterations; the iteration before a check and the check iteration take plain steps, the history still recorded.
Test infrastructure.
"""
import math
from types import SimpleNamespace

import numpy as np

from box_adaptive_support import RHO_MAX, RHO_MIN, penalty_step
from box_support import blocks, masks, shifted_problem

MEM_MAX = 16


def cholesky_solve(A, b, c):
    """gamma (list of c floats) with A gamma = b, A = L L' (A: c x c nested lists, already regularised); None when a
    pivot is not positive or a coefficient is not finite"""
    L = [[0.0] * c for _ in range(c)]
    for j in range(c):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return None
        d = math.sqrt(d)
        L[j][j] = d
        for i in range(j + 1, c):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / d
    x = [0.0] * c
    for i in range(c):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * x[k]
        x[i] = s / L[i][i]
    for i in range(c - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, c):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x if all(math.isfinite(a) for a in x) else None


def tree_dot(a, b, dev, perm=None):
    """sum of a * b in the order of the kernel in strict mode. a, b: the values of the bounded entries, dev: the index of
    each in the device layout [N][n+m]. Thread e mod 256 adds the products of its entries e in rising order to 0.0
    (multiply, then add: no fma); each of the four wavefronts folds its 64 partial sums by halves (lane l takes lane
    l + 32, then l + 16, ... l + 1); the four results add as (s0 + s1) + (s2 + s3). perm: the products take each
    other's places first (p[perm]) -- another order of the same sum."""
    p = a * b
    if perm is not None:
        p = p[perm]
    part = np.zeros(256)
    rounds = dev // 256
    for r in range(int(rounds.max()) + 1 if dev.size else 0):
        sel = rounds == r
        idx = dev[sel] % 256
        part[idx] = part[idx] + p[sel]
    w = part.reshape(4, 64).copy()
    off = 32
    while off:
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
        off //= 2
    return float((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))


def admm_accel_reference(prob, solve, xlo, xhi, ulo, uhi, rho, alpha, eps_abs, eps_rel, max_iter, mem=0, safeguard=1.0,
                         reg=1e-10, adapt_every=0, rho_min=RHO_MIN, rho_max=RHO_MAX, perm=None, infeas_every=0,
                         infeas_eps=1e-4, device_dims=None):
    """The iteration of DESIGN.md sections 3.9, 3.11 and 3.15 in the operation order of strict mode; solve(problem) -> z
    (nvars). mem == 0: box_support.admm_reference array for array (`plain` holds its tuple). Returns a namespace: x, u
    (from v, [N, n], [N, m]), mu_x, mu_u, lam (of the last solve), iters, status (1, 2, 3; 4 with infeas_every: certified
    at `iters`), rho, plain = (x, u, mu_x, mu_u, lam, iters, status); accepted, rejected; gamma [mem] and columns of the
    latest accelerated step (device_dims: the block sizes (n, m) of the device layout when the shape runs padded; they
    fix which thread adds which entry); ratios: |g| / (safeguard |g_prev|) of every safeguard decision, as (iteration, ratio); drops: the
    pushes that found the ring full."""
    n, m, N = prob.n, prob.m, prob.N
    dn, dm = (n, m) if device_dims is None else device_dims
    Mx, Mu = masks(n, m, N, xlo, xhi, ulo, uhi)
    M = np.concatenate([Mx, Mu], axis=1) > 0
    lo = np.concatenate([np.where(Mx > 0, xlo, -np.inf), np.where(Mu > 0, ulo, -np.inf)], axis=1)
    hi = np.concatenate([np.where(Mx > 0, xhi, np.inf), np.where(Mu > 0, uhi, np.inf)], axis=1)
    lob, hib = lo[M], hi[M]
    q = np.concatenate([prob.q, prob.r], axis=1)
    v = np.zeros((N, n + m))
    y = np.zeros((N, n + m))
    oma = 1.0 - alpha
    qt = q.copy()
    rho = float(rho)
    status, it = 0, 0
    Z = None
    mx = lambda a: float(np.abs(a[M]).max()) if M.any() else 0.0
    # the device index of every bounded entry, in the order of a[M]: entry (k, j) of [N][dn + dm]
    cols = np.concatenate([np.arange(n), dn + np.arange(m)])
    dev = (np.arange(N)[:, None] * (dn + dm) + cols[None, :])[M]
    order = None if perm is None else np.asarray(perm)
    dot = lambda a, b: tree_dot(a, b, dev, order)
    # the history, oldest first, over the bounded entries: T, G at most mem + 1 entries; gram[i][j] = dG_i . dG_j of the
    # columns dG_i = G[i + 1] - G[i], kept up by one row and column per push
    T, G, gram = [], [], []
    pv = py = None       # the plain successor saved by an accelerated step
    accelerated = False  # the iterate this iteration starts from is an accelerated one
    g_prev = 0.0
    accepted = rejected = columns = drops = 0
    gamma = np.zeros(max(mem, 0))
    ratios = []
    lam_prev = mu_prev = None
    is_check = lambda i: infeas_every > 0 and i >= 2 and i <= max_iter and i % infeas_every == 0
    for it in range(1, max_iter + 1):
        z = solve(shifted_problem(prob, rho, Mx, Mu, np.ascontiguousarray(qt[:, :n]), np.ascontiguousarray(qt[:, n:])))
        Z = blocks(z, n, m, N)
        zx = Z[:, n:]
        zh = alpha * zx + oma * v
        t = zh + y
        vn = np.minimum(np.maximum(t, lo), hi)
        yn = (y + zh) - vn
        vn = np.where(M, vn, 0.0)
        yn = np.where(M, yn, 0.0)
        r_prim = mx(zx - vn)
        r_dual = rho * mx(vn - v)
        sp = max(mx(zx), mx(vn))
        sd = rho * mx(yn)
        finite = all(math.isfinite(a) for a in (r_prim, r_dual, mx(zx), mx(vn), mx(yn)))
        conv = finite and r_prim <= eps_abs + eps_rel * sp and r_dual <= eps_abs + eps_rel * sd
        v0, y0 = v, y
        v, y = vn, yn  # the plain step: what every branch below that does not say otherwise takes
        if conv or not finite:
            status = 1 if conv else 3
            break
        new = rho
        if adapt_every > 0 and it % adapt_every == 0 and it < max_iter:
            new = penalty_step(rho, r_prim, r_dual, sp, sd, rho_min, rho_max)
        if new != rho:  # w changes scale with rho: the plain step, y rescaled, the history gone
            y = np.where(M, y * (rho / new), 0.0)
            rho = new
            T, G, gram, accelerated = [], [], [], False
        elif mem > 0:
            tb = t[M]
            gb = tb - (v0 + y0)[M]
            gnorm = math.sqrt(dot(gb, gb))
            reject = False
            if accelerated:
                ratios.append((it, gnorm / (safeguard * g_prev) if safeguard * g_prev > 0.0 else math.inf))
                reject = gnorm > safeguard * g_prev
            if reject:  # back to the plain successor of the iterate before; g_prev stays
                v, y = pv, py
                T, G, gram, accelerated = [], [], [], False
                rejected += 1
            else:
                if len(T) == mem + 1:
                    T.pop(0)
                    drops += 1
                    G.pop(0)
                    gram = [row[1:] for row in gram[1:]]
                if G:
                    dgn = gb - G[-1]
                    row = [dot(G[i + 1] - G[i], dgn) for i in range(len(G) - 1)] + [dot(dgn, dgn)]
                    for i, r in enumerate(gram):
                        r.append(row[i])
                    gram.append(list(row))
                T.append(tb)
                G.append(gb)
                c = len(T) - 1
                w = None
                if c >= 1 and not (is_check(it) or is_check(it + 1)):
                    b = [dot(G[i + 1] - G[i], gb) for i in range(c)]
                    tr = 0.0
                    for i in range(c):
                        tr = tr + gram[i][i]
                    shift = reg * tr / c
                    A = [[gram[i][j] + (shift if i == j else 0.0) for j in range(c)] for i in range(c)]
                    gam = cholesky_solve(A, b, c)
                    if gam is not None:
                        corr = np.zeros_like(tb)
                        for j in range(c):
                            corr = corr + gam[j] * (T[j + 1] - T[j])
                        w = tb - corr
                        if not np.isfinite(w).all():
                            w = None
                    if w is None:  # a pivot that is not positive, or a value that is not finite: plain, the history gone
                        T, G, gram = [], [], []
                if w is not None:
                    pv, py = vn, yn
                    vb = np.minimum(np.maximum(w, lob), hib)
                    v = np.zeros((N, n + m))
                    y = np.zeros((N, n + m))
                    v[M] = vb
                    y[M] = w - vb
                    accelerated = True
                    accepted += 1
                    gamma = np.zeros(mem)
                    gamma[:c] = gam
                    columns = c
                else:
                    accelerated = False
                g_prev = gnorm
        if infeas_every > 0:
            from box_infeas_support import farkas_check
            lam, mu = Z[:, :n].copy(), rho * y
            if is_check(it):
                dlam, dmu = lam - lam_prev, mu - mu_prev
                if farkas_check(prob, (xlo, xhi, ulo, uhi), dlam, dmu[:, :n], dmu[:, n:], infeas_eps)["ok"]:
                    status = 4
                    break
            lam_prev, mu_prev = lam, mu
        tt = y - v
        tt = rho * tt
        qt = np.where(M, q + tt, q)
    xu = np.where(M, v, Z[:, n:])
    mu = rho * y
    status = status or 2
    out = SimpleNamespace(x=xu[:, :n], u=xu[:, n:], mu_x=mu[:, :n], mu_u=mu[:, n:], lam=Z[:, :n], iters=it, status=status,
                          rho=rho, accepted=accepted, rejected=rejected, gamma=gamma, columns=columns, ratios=ratios,
                          drops=drops)
    out.plain = (out.x, out.u, out.mu_x, out.mu_u, out.lam, it, status)
    return out
