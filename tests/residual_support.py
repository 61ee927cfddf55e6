"""Test infrastructure of the device residual kernels (kkt_residual_generic behind ndlqr_BatchKktResiduals,
kkt_residual_dd behind ndlqr_BatchKktResidualVector and ndlqr_RefineBatch): a plain extended-precision evaluation of the
KKT rows that shares no code with the oracle, the kernels or refine_support.residual_dd; a restatement of how the host
layer pads a block size and shapes the launch of kkt_residual_dd, so that the cases of tests/test_gpu_residuals.py can
be held to the branches they were chosen for; and the problems and settings of the strict-mode termination test of the
box-constrained solve, which the CPU suite pins (test_residual_support_host.py) and the GPU suite uses.

The rows of K z - b, from the comment above kkt_residual_generic (b = -(x_init | d_(k-1)) | -q_k | -r_k):
    lambda_0:      x_init - x_0
    lambda_(k+1):  A_k x_k + B_k u_k + d_k - x_(k+1)              (k < N - 1)
    x_k:           Q_k x_k + q_k - lambda_k + A_k' lambda_(k+1)   (no A' term at the last knot)
    u_k:           R_k u_k + r_k + B_k' lambda_(k+1)              (k < N - 1)
The u slot of the last knot is not part of the system: it is in neither vector."""
import numpy as np

LD = np.longdouble


def rhs_ld(prob):
    """b [nvars] of the raw problem in np.longdouble: -(x_init | d_(k-1)) | -q_k | -r_k per knot, without the u slot of
    the last knot."""
    n, m, N = prob.n, prob.m, prob.N
    b = np.zeros((N, 2 * n + m), dtype=LD)
    b[0, :n] = -prob.x0.astype(LD)
    b[1:, :n] = -prob.d[: N - 1].astype(LD)
    b[:, n:2 * n] = -prob.q.astype(LD)
    b[: N - 1, 2 * n:] = -prob.r[: N - 1].astype(LD)
    return b.reshape(-1)[: prob.nvars]


def norm_ld(v):
    v = np.asarray(v, dtype=LD)
    return np.sqrt(np.sum(v * v))


def kkt_rows_ld(prob, z):
    """(K z - b [nvars], b [nvars], ||K z - b||_2, ||b||_2) in np.longdouble, for z packed in the reference's
    [lambda x u] order ([nvars]: the u slot of the last knot is absent)."""
    n, m, N = prob.n, prob.m, prob.N
    rows = 2 * n + m
    z = np.asarray(z, dtype=LD)
    assert z.size == prob.nvars
    Z = np.concatenate([z, np.zeros(m, dtype=LD)]).reshape(N, rows)
    lam, x, u = Z[:, :n], Z[:, n:2 * n], Z[:, 2 * n:]
    # column-major storage: entry (i, j) of A_k at j * n + i, so the stored array is [k][j][i]
    At = prob.A.astype(LD).reshape(N, n, n)[: N - 1]
    Bt = prob.B.astype(LD).reshape(N, m, n)[: N - 1]
    res = np.zeros((N, rows), dtype=LD)
    res[0, :n] = prob.x0.astype(LD) - x[0]
    # lambda_(k+1), entry i: sum_j A[i, j] x_k[j] + sum_j B[i, j] u_k[j] + d_k[i] - x_(k+1)[i]
    res[1:, :n] = ((At * x[: N - 1, :, None]).sum(axis=1) + (Bt * u[: N - 1, :, None]).sum(axis=1)
                   + prob.d[: N - 1].astype(LD) - x[1:])
    res[:, n:2 * n] = prob.Q.astype(LD) * x + prob.q.astype(LD) - lam
    # x_k, entry i: + sum_j A[j, i] lambda_(k+1)[j]
    res[: N - 1, n:2 * n] += (At * lam[1:, None, :]).sum(axis=2)
    res[: N - 1, 2 * n:] = (prob.R[: N - 1].astype(LD) * u[: N - 1] + prob.r[: N - 1].astype(LD)
                            + (Bt * lam[1:, None, :]).sum(axis=2))
    res = res.reshape(-1)[: prob.nvars]
    b = rhs_ld(prob)
    return res, b, norm_ld(res), norm_ld(b)


def mixed_problem(first, other):
    """The matrices of `first` with the right-hand side (q, r, d, x0) of `other`."""
    from support import Problem
    return Problem(first.n, first.m, first.N, first.A, first.B, first.Q, first.R, other.q, other.r, other.d, other.x0)


# ------------------------------------------------------------------------ the launch of kkt_residual_dd, restated

LDS_MAX = 160 * 1024  # kLdsMax of csrc/hip_context.hpp


def padded_dims(n, m, N):
    """The block size the device works on (ndlqr_hip_create): a size without a size-specialised instance runs inside
    the cheapest instance of six states or more that contains it when N >= 8 (pick_pad_instance), and beyond 128 states a
    block that does not fill 16 x 16 tiles is padded to the next one that does."""
    from rslqr_amd.build import small_instances
    inst = small_instances()
    pn, pm = n, m
    if (n, m) not in inst and N >= 8:
        best = None
        for nx, nu in inst:
            if nx < n or nu < m or nx < 6:
                continue
            cost = nx * nx * (nx + nu)
            if best is None or cost < best:
                best, pn, pm = cost, nx, nu
    if n > 128 and (n % 16 != 0 or (n + m) % 4 != 0):
        pn = (n + 15) // 16 * 16
        pm = m + (4 - (pn + m) % 4) % 4
    return pn, pm


def residual_dd_launch(n, m, N):
    """(threads, staged, passes of the task loop in block 0, padded (n, m)) of kkt_residual_dd at this shape, by the
    formulas of launch_residual_dd and refine_lds_bytes."""
    pn, pm = padded_dims(n, m, N)
    rows, w = 2 * pn + pm, pn + pm
    staged = 8 * (pn * (w | 1) + 2 * rows) + 64 <= LDS_MAX
    ntask = rows + pn
    threads = 64 if ntask <= 64 else 128 if ntask <= 128 else 256
    return threads, staged, -(-ntask // threads), (pn, pm)


# ---------------------------------------------------------------------------- strict-mode termination of the box solve

# (n, m, N, seed of the first problem; the second has seed + 1): the settings below end both problems of every pair by
# convergence before max_iter -- on the restatement driven by the oracle (test_residual_support_host.py pins that)
BOX_TERMINATION_CASES = [(12, 4, 16, 80), (7, 9, 16, 80), (20, 6, 16, 80), (6, 3, 4, 80)]
BOX_TERMINATION = dict(rho=0.37, alpha=1.6, eps_abs=1e-4, eps_rel=1e-4, max_iter=400)


def box_termination_reference(ndlqr, oracle, n, m, N, seed):
    """(problems, (xlo, xhi, ulo, uhi) [2, N, .], the restatement's result per problem) of one termination case: the
    bounds of test_gpu_box.test_strict_mode_is_the_numpy_restatement_bit_for_bit (inputs at half their mean unconstrained
    size, states at 0.7 of their unconstrained range)."""
    from box_support import admm_reference
    from test_gpu_box import input_box, state_box, synth
    probs = [synth(ndlqr, n, m, N, seed + p) for p in range(2)]
    ulo, uhi = input_box(oracle, probs, 0.5)
    xlo, xhi = state_box(oracle, probs, 0.7)
    solve = lambda pr: oracle.solve(pr, 1)[0][: pr.nvars]
    s = BOX_TERMINATION
    ref = [admm_reference(prob, solve, xlo[p], xhi[p], ulo[p], uhi[p], s["rho"], s["alpha"], s["eps_abs"], s["eps_rel"],
                          s["max_iter"]) for p, prob in enumerate(probs)]
    return probs, (xlo, xhi, ulo, uhi), ref
