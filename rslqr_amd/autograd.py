"""Differentiable batch LQR solve: ``lqr_solve`` is a ``torch.autograd.Function`` over float64 tensors on one ROCm device.

Forward: the problems are packed on the device (ndlqr_InitializeBatchFlatDevice) and solved with
NDLQR_FLAG_KEEP_RECORDS. Backward: the adjoint solve against the kept factorisation (ndlqr_SolveBatchAdjoint) and the
gradient kernels (ndlqr_BatchGradients) write straight into torch tensors.

Shapes (ordinary row-major math convention; b problems, N knots, n states, m inputs):
    A [b, N, n, n]   B [b, N, n, m]   Q, q, d [b, N, n]   R, r [b, N, m]   x0 [b, n]   ->   z [b, nvars]
Q and R are the diagonals. Any argument may leave out the leading batch dimension: it is then shared by every problem
(broadcast in the forward pass) and its gradient is the batch sum computed by the library. z holds, per knot,
[lambda_k x_k u_k] (no u at the last knot); ``split_solution`` gives the three views.

Streams: the library runs on streams of its own. Before it reads torch memory, torch's current stream is synchronised;
every call into the library returns only after its writes are complete. That is the whole contract: the tensors this
module returns may be used on any stream at once.

``lqr_solve_dense`` takes dense cost matrices Q, R and a state-input cross term H (ndlqr_InitializeBatchFlatDense); its
backward is one adjoint solve and the gradient kernel of dense-cost mode (ndlqr_BatchGradientsDense), which writes the
gradients that are asked for straight into torch tensors -- batch-summed on the device for a shared argument.

``lqr_solve_constrained`` adds rows lo <= C x + D u <= hi to the dense-cost problem (ndlqr_SolveBatchLinConstrained); its
backward is the adjoint of the active-set system (ndlqr_SolveBatchLinAdjoint), the nine problem gradients from ndlqr_BatchGradientsDense as for
``lqr_solve_dense`` and the four row gradients from ndlqr_BatchConstraintGradients.

``lqr_solve_box`` adds bounds on x and u (ndlqr_SolveBatchBoxConstrained); its backward is the adjoint of the
active-set system (ndlqr_SolveBatchBoxAdjoint) plus the gradients with respect to the bounds (ndlqr_BatchBoundGradients).

``lqr_value`` and ``lqr_value_dense`` return the optimal values J* [b] of the problems of ``lqr_solve`` and of
``lqr_solve_dense`` (ndlqr_BatchObjective behind a plain solve on the same cached solvers); their backward needs no adjoint
solve: by the envelope theorem it is the partial derivative of the Lagrangian at the saved solution, in torch.

Process start-up: torch ships its own HIP runtime next to the system one this library links. Initialise torch's device
(any CUDA tensor) before the library's first device call in a process; the other order may leave torch without a device.
"""
import itertools

import torch

from .api import BatchSolver, FLAG_KEEP_RECORDS, GRAD_DENSE_NAMES, GRAD_NAMES

# (what `from rslqr_amd.autograd import *` gives; lqr_solve_dense, lqr_solve_constrained, lqr_value, lqr_value_dense and
# their Function classes are public too and are imported by name)
__all__ = ["LqrSolve", "LqrSolveRefined", "LqrSolveBox", "lqr_solve", "lqr_solve_box", "split_solution"]

_ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
_BOUNDS = ("xlo", "xhi", "ulo", "uhi")
_DENSE_ARGS = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
_ROW_ARGS = ("C", "D", "lo", "hi")
# Four caches, key -> [BatchSolver, token of the forward it holds]. The box solve has one of its own, so that lqr_solve and
# lqr_solve_box do not evict each other's solvers; a solver in dense-cost mode serves no diagonal forward in between; a
# solver in constrained mode retains its problem on the device.
_cache = {}                  # (n, m, N, b, device index)
_box_cache = {}              # (n, m, N, b, device index)
_dense_cache = {}            # (n, m, N, b, device index)
_lin_cache = {}              # (n, m, N, p, b, device index)
_tokens = itertools.count(1)


class _View:
    """A tensor's device memory as the library's bindings take it (``ptr``, ``size``)."""

    def __init__(self, t):
        self.ptr, self.size = t.data_ptr(), t.numel()


def split_solution(z, n, m, N):
    """Views of z [..., nvars]: lambda [..., N, n], x [..., N, n], u [..., N - 1, m]."""
    zb = 2 * n + m
    full = torch.nn.functional.pad(z, (0, m)).reshape(*z.shape[:-1], N, zb)
    return full[..., :n], full[..., n:2 * n], full[..., :N - 1, 2 * n:]


# ------------------------------------------------------------------------------------------------ what every entry point shares
def _require_float64(who, name, t, or_none=""):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch.Tensor%s" % (who, name, or_none))
    if t.dtype != torch.float64:
        raise TypeError("%s: %s must be float64, got %s" % (who, name, t.dtype))


def _check(who, names, args, shapes):
    """The argument checks of every entry point (`who` opens the messages): float64 tensors on one ROCm device, each of
    its shape in `shapes(who, *args)` -- a dict per name, which checks A, B (and C), the arguments that decide the sizes --
    or with a batch dimension in front. Returns (device, per argument whether it is shared, (n, m, N, b))."""
    dev = None
    for name, t in zip(names, args):
        _require_float64(who, name, t)
        if t.device.type != "cuda":
            raise ValueError("%s: %s must live on a ROCm device, got %s" % (who, name, t.device))
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("%s: every argument must be on one device (%s is on %s, A on %s)" % (who, name, t.device, dev))
    per = shapes(who, *args)
    batch = set()
    shared = []
    for name, t in zip(names, args):
        shape = per[name]
        if tuple(t.shape) == shape:
            shared.append(True)
        elif t.dim() == len(shape) + 1 and tuple(t.shape[1:]) == shape:
            shared.append(False)
            batch.add(t.shape[0])
        elif name in ("Q", "R") and len(shape) == 2 and t.dim() >= 3 and t.shape[-1] == t.shape[-2] == shape[-1]:
            raise ValueError("%s: %s must hold the diagonals, [b, N, %d] or [N, %d]; got the matrices %s"
                             % (who, name, shape[-1], shape[-1], tuple(t.shape)))
        else:
            raise ValueError("%s: %s must be [b, %s] or %s, got %s"
                             % (who, name, ", ".join(str(x) for x in shape), list(shape), tuple(t.shape)))
    if len(batch) > 1:
        raise ValueError("%s: batch dimensions disagree: %s" % (who, sorted(batch)))
    N, n, m = per["B"]
    return dev, tuple(shared), (n, m, N, batch.pop() if batch else 1)


def _diagonal_shapes(who, A, B, *rest):
    if A.dim() not in (3, 4) or A.shape[-1] != A.shape[-2]:
        raise ValueError("%s: A must be [b, N, n, n] or [N, n, n], got %s" % (who, tuple(A.shape)))
    N, n = A.shape[-3], A.shape[-1]
    if B.dim() not in (3, 4) or B.shape[-3] != N or B.shape[-2] != n:
        raise ValueError("%s: B must be [b, N, n, m] or [N, n, m], got %s" % (who, tuple(B.shape)))
    m = B.shape[-1]
    return dict(A=(N, n, n), B=(N, n, m), Q=(N, n), R=(N, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))


def _dense_shapes(who, A, B, *rest):
    if A.dim() not in (3, 4) or A.shape[-1] != A.shape[-2] or B.dim() not in (3, 4) or B.shape[-3:-1] != A.shape[-3:-1]:
        raise ValueError("%s: A must be [b, N, n, n] and B [b, N, n, m] (b optional), got %s and %s"
                         % (who, tuple(A.shape), tuple(B.shape)))
    N, n, m = B.shape[-3:]
    return dict(A=(N, n, n), B=(N, n, m), Q=(N, n, n), H=(N, n, m), R=(N, m, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))


def _row_shapes(who, *args):
    per = _dense_shapes(who, *args)
    C = args[9]
    N, n, m = per["B"]
    if C.dim() not in (3, 4) or C.shape[-3] != N or C.shape[-1] != n or C.shape[-2] < 1:
        raise ValueError("%s: C must be [b, N, p, n] or [N, p, n] with p >= 1, got %s" % (who, tuple(C.shape)))
    p = C.shape[-2]
    return dict(per, C=(N, p, n), D=(N, p, m), lo=(N, p), hi=(N, p))


def _flat(args, shared, b):
    """The flat layout of ndlqr_InitializeBatchFlat and ndlqr_InitializeBatchFlatDense, contiguous on the device: matrices
    column-major per knot (the transpose, stored row-major); an argument without its batch dimension (`shared`) expanded
    to the batch."""
    out = []
    for t, sh in zip(args, shared):
        t = t.detach()
        if sh:
            t = t.unsqueeze(0)
        if t.dim() == 4:
            t = t.transpose(-1, -2)
        out.append(t.expand(b, *t.shape[1:]).contiguous().reshape(b, -1))
    return out


def _solver(cache, dev, dims, p=()):
    """(key, solver) of `cache` for problems of dims = (n, m, N, b) -- and p rows -- on `dev`: made with
    NDLQR_FLAG_KEEP_RECORDS on that device when the cache has none."""
    n, m, N, b = dims
    key = (n, m, N) + tuple(p) + (b, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in cache:
        cache[key] = [BatchSolver(n, m, N, b, device=key[-1], flags=FLAG_KEEP_RECORDS), None]
    return key, cache[key][0]


def _solution(bs, dev):
    """The resident solution z [b, nvars] in a new torch tensor."""
    z = torch.empty((bs.batch, bs.nvars), dtype=torch.float64, device=dev)
    bs.solutions_to_device(z.data_ptr())
    bs.synchronize()
    return z


def _resume(cache, ctx, gz, resolve):
    """What every backward starts with: (the node's solver, gz contiguous in float64, torch's stream synchronised). If the
    solver has served another forward since, `resolve(solver)` redoes this node's first."""
    bs, token = cache[ctx.key]
    if token != ctx.token:
        resolve(bs)
    gz = gz.detach().to(torch.float64).contiguous()
    torch.cuda.current_stream(gz.device).synchronize()
    return bs, gz


def _require_converged(status, infeasible, message):
    """RuntimeError message % (how many, of how many, their statuses) unless every problem that is not certified
    `infeasible` ended with status 1."""
    bad = int(((status != 1) & ~infeasible).sum())
    if bad:
        raise RuntimeError(message % (bad, status.size, sorted(set(status[~infeasible].tolist()) - {1})))


def _named_gradients(names, shared, needs, shape_of, compute, rows, device):
    """The gradients of `names`, those that `needs` asks for, written by the library (`compute(sum mask, views)`) into new
    torch tensors of `shape_of(name, summed)`; a `shared` argument's is the batch sum computed on the device. A list in
    the order of `names`, None where none is needed. rows: name -> rows of the matrices, which come back row-major (the
    math convention). Torch's stream needs no synchronisation here: _resume drained it before the adjoint solve, and
    nothing but allocations has gone through torch since."""
    mask = 0
    out = {}
    for i, (name, sh, need) in enumerate(zip(names, shared, needs)):
        if not need:
            continue
        if sh:
            mask |= 1 << i
        out[name] = torch.empty(shape_of(name, sh), dtype=torch.float64, device=device)
    if out:
        compute(mask, {name: _View(g) for name, g in out.items()})
    grads = []
    for name in names:
        g = out.get(name)
        if g is not None and name in rows:  # flat column-major -> row-major math convention
            g = g.reshape(*g.shape[:-1], g.shape[-1] // rows[name], rows[name]).transpose(-1, -2)
        grads.append(g)
    return grads


# ------------------------------------------------------------------------------------------------ diagonal costs
def _solve(bs, flat, token, key, refine=0):
    """Factor + solve of `flat` on the cached solver (and `refine` steps of iterative refinement at most); the solver then
    holds forward `token`."""
    torch.cuda.current_stream(flat[0].device).synchronize()  # (the library reads torch memory on its own stream)
    bs.initialize_flat_device(*[t.data_ptr() for t in flat])
    err = bs.solve()
    if err or bs.cholesky_failures() > 0:
        _cache[key][1] = None
        raise RuntimeError("lqr_solve: the factorisation failed (%d non-positive pivots): Q, R or the problem are not "
                           "positive definite" % max(bs.cholesky_failures(), 1))
    if refine > 0:
        bs.refine(refine)
    _cache[key][1] = token


def _forward(ctx, refine, args):
    dev, shared, dims = _check("lqr_solve", _ARGS, args, _diagonal_shapes)
    key, bs = _solver(_cache, dev, dims)
    flat = _flat(args, shared, dims[3])
    token = next(_tokens)
    _solve(bs, flat, token, key, refine)
    ctx.key, ctx.token, ctx.flat, ctx.shared, ctx.dims, ctx.refine = key, token, flat, shared, dims, refine
    return _solution(bs, dev)


def _backward(ctx, gz, needs_input_grad):
    bs, gz = _resume(_cache, ctx, gz, lambda bs: _solve(bs, ctx.flat, ctx.token, ctx.key, ctx.refine))
    err = bs.solve_adjoint(_View(gz))
    if err:
        raise RuntimeError("lqr_solve backward: adjoint solve failed: %d" % err)
    if ctx.refine > 0:
        bs.refine_adjoint(ctx.refine)
    n = ctx.dims[0]
    return tuple(_named_gradients(GRAD_NAMES, ctx.shared, needs_input_grad, bs.gradient_shape, bs.gradients, dict(A=n, B=n),
                                  gz.device))


class LqrSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        return _forward(ctx, 0, args)

    @staticmethod
    def backward(ctx, gz):
        return _backward(ctx, gz, ctx.needs_input_grad)


class LqrSolveRefined(torch.autograd.Function):
    """LqrSolve with `refine` steps of iterative refinement (ndlqr_RefineBatch) behind the forward solve and behind the
    adjoint solve of the backward (ndlqr_RefineBatchAdjoint)."""

    @staticmethod
    def forward(ctx, refine, *args):
        return _forward(ctx, refine, args)

    @staticmethod
    def backward(ctx, gz):
        return (None,) + _backward(ctx, gz, ctx.needs_input_grad[1:])


def lqr_solve(A, B, Q, R, q, r, d, x0, refine=0):
    """z [b, nvars] of the LQR problems (see the module docstring), differentiable in every argument. refine > 0: that
    many steps of iterative refinement with a double-double residual at most (BatchSolver.refine) on the solution, and in
    the backward on the adjoint before the gradients are assembled; 0: neither."""
    refine = int(refine)
    if refine < 0 or refine > 8:
        raise ValueError("lqr_solve: refine must lie in 0 .. 8, got %d" % refine)
    if refine == 0:
        return LqrSolve.apply(A, B, Q, R, q, r, d, x0)
    return LqrSolveRefined.apply(refine, A, B, Q, R, q, r, d, x0)


# ------------------------------------------------------------------------------------------------ box-constrained
def _check_bounds(bounds, dev, n, m, N, b):
    """Each bound None, [N, n|m] (shared by every problem) or [b, N, n|m]; returns the per-bound shared flags."""
    shared = []
    for name, t in zip(_BOUNDS, bounds):
        if t is None:
            shared.append(None)
            continue
        _require_float64("lqr_solve_box", name, t, " or None")
        if t.device != dev:
            raise ValueError("lqr_solve_box: %s must be on the problem's device %s, got %s" % (name, dev, t.device))
        k = n if name[0] == "x" else m
        if tuple(t.shape) == (N, k):
            shared.append(True)
        elif tuple(t.shape) == (b, N, k):
            shared.append(False)
        else:
            raise ValueError("lqr_solve_box: %s must be [%d, %d] or [%d, %d, %d], got %s" % (name, N, k, b, N, k, tuple(t.shape)))
    if all(s is None for s in shared):
        raise ValueError("lqr_solve_box: no bounds given (use lqr_solve)")
    return shared


def _flat_bounds(bounds, bshared, b):
    """(NDLQR_BOUNDS_SHARED when every given bound is shared, contiguous device copies): shared bounds are expanded to
    the batch when others are per problem."""
    all_shared = all(s is not False for s in bshared)
    out = []
    for t, sh in zip(bounds, bshared):
        if t is None:
            out.append(None)
            continue
        t = t.detach()
        if sh and not all_shared:
            t = t.unsqueeze(0).expand(b, *t.shape)
        out.append(t.contiguous())
    return all_shared, out


def _solve_box(bs, flat, bflat, all_shared, settings, token, key):
    """Factor + constrained solve (cold) of `flat` with the bounds `bflat` on the cached solver; it then holds `token`."""
    from .api import BOUNDS_SHARED, _any_ptr
    torch.cuda.current_stream(flat[0].device).synchronize()  # (the library reads torch memory on its own stream)
    _box_cache[key][1] = None
    bs.initialize_flat_device(*[t.data_ptr() for t in flat])
    # (through the library itself: BatchSolver.set_bounds has no way to say that bounds in device memory are shared)
    ptrs = [None if t is None else _any_ptr(_View(t), t.numel()) for t in bflat]
    err = bs.L.ndlqr_BatchSetBounds(bs.h, BOUNDS_SHARED if all_shared else 0, *ptrs)
    if err:
        raise ValueError("lqr_solve_box: the bounds were refused (%s)" % bs.L.ndlqr_hip_last_error().decode())
    rho, alpha, eps_abs, eps_rel, max_iter, adapt_every, polish, infeas_every, accel_mem = settings
    bs.set_box_infeasibility(infeas_every)  # (the cached solver keeps the setting of whoever used it last)
    bs.set_box_acceleration(accel_mem)
    try:
        _, status = bs.solve_box(rho=rho, alpha=alpha, eps_abs=eps_abs, eps_rel=eps_rel, max_iter=max_iter,
                                 adapt_every=adapt_every)
    except RuntimeError as e:
        raise RuntimeError("lqr_solve_box: the constrained solve failed (%s)" % e) from None
    infeasible = status == 4  # (only with infeas_every > 0: certified, z is the last iterate, the gradients are zero)
    _require_converged(status, infeasible, "lqr_solve_box: %d of %d problems did not converge (status %s): raise max_iter, "
                       "change rho or set adapt_every (the per-problem adaptive penalty)")
    if polish:
        try:
            _, status = bs.polish_box()
        except RuntimeError as e:
            raise RuntimeError("lqr_solve_box: the polish failed (%s)" % e) from None
        _require_converged(status, infeasible, "lqr_solve_box: %d of %d problems were not polished (status %s): the active "
                           "set ADMM left was not corrected within the rounds; tighten eps_abs / eps_rel")
    _box_cache[key][1] = token
    return infeasible


class LqrSolveBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, settings, *args):
        problem, bounds = args[:8], args[8:]
        dev, shared, dims = _check("lqr_solve", _ARGS, problem, _diagonal_shapes)
        n, m, N, b = dims
        bshared = _check_bounds(bounds, dev, n, m, N, b)
        key, bs = _solver(_box_cache, dev, dims)
        flat = _flat(problem, shared, b)
        all_shared, bflat = _flat_bounds(bounds, bshared, b)
        token = next(_tokens)
        ctx.infeasible = _solve_box(bs, flat, bflat, all_shared, settings, token, key)
        ctx.key, ctx.token, ctx.flat, ctx.shared, ctx.dims = key, token, flat, shared, dims
        ctx.bflat, ctx.bshared, ctx.all_shared, ctx.settings = bflat, bshared, all_shared, settings
        return _solution(bs, dev)

    @staticmethod
    def backward(ctx, gz):
        n, m, N, b = ctx.dims
        bs, gz = _resume(_box_cache, ctx, gz, lambda bs: _solve_box(bs, ctx.flat, ctx.bflat, ctx.all_shared, ctx.settings,
                                                                     ctx.token, ctx.key))
        _, alpha, eps_abs, eps_rel, max_iter, _, polish, _, _ = ctx.settings
        if polish:
            _, status = bs.solve_polished_adjoint(_View(gz))
        else:
            _, status = bs.solve_box_adjoint(_View(gz), alpha=alpha, eps_abs=eps_abs, eps_rel=eps_rel, max_iter=max_iter)
        # (a certified problem is not iterated: w = 0, nu = 0)
        _require_converged(status, ctx.infeasible, "lqr_solve_box backward: the adjoint of %d of %d problems did not converge "
                           "(status %s)")
        need, need_b = ctx.needs_input_grad[1:9], ctx.needs_input_grad[9:]
        grads = _named_gradients(GRAD_NAMES, ctx.shared, need, bs.gradient_shape, bs.gradients, dict(A=n, B=n), gz.device)
        bout = {}
        for name, t, nd in zip(_BOUNDS, ctx.bflat, need_b):
            if nd and t is not None:
                k = n if name[0] == "x" else m
                bout[name] = torch.empty((N, k) if ctx.all_shared else (b, N, k), dtype=torch.float64, device=gz.device)
        if bout:
            bs.bound_gradients(ctx.all_shared, {k: _View(v) for k, v in bout.items()})
        for name, sh in zip(_BOUNDS, ctx.bshared):
            g = bout.get(name)
            if g is not None and sh and not ctx.all_shared:  # a shared bound expanded to the batch: its gradient summed
                g = g.sum(0)
            grads.append(g)
        return (None,) + tuple(grads)


def lqr_solve_box(A, B, Q, R, q, r, d, x0, xlo=None, xhi=None, ulo=None, uhi=None, *, rho=0.0, alpha=0.0, eps_abs=0.0,
                  eps_rel=0.0, max_iter=0, adapt_every=0, polish=False, infeas_every=0, accel_mem=0):
    """z* [b, nvars] of the LQR problems of lqr_solve with xlo <= x_k <= xhi (k >= 1) and ulo <= u_k <= uhi, by the
    box-constrained batch solve (ndlqr_SolveBatchBoxConstrained, cold start; 0 = the library's default for every
    setting; adapt_every > 0: the per-problem adaptive penalty, considered every that many iterations, so that rho
    need not be tuned to the problem family), differentiable in all twelve tensors: the backward is the adjoint of the
    active-set system (ndlqr_SolveBatchBoxAdjoint) with the same settings, on the penalties the forward ended with. Bounds: None (unbounded), [N, n] / [N, m] shared by every problem
    or [b, N, n] / [b, N, m]; entries may be +-inf. Raises RuntimeError when a problem's forward or adjoint iteration
    does not converge (status != 1). The gradients hold where the active set is locally stable (strict
    complementarity); at a degenerate active set the bound gradients are one of many.
    polish=True: the forward is ADMM followed by the active-set polish (ndlqr_PolishBatchBoxConstrained, default
    settings), so a loose eps_abs / eps_rel such as 1e-3 suffices, and the backward is the polished adjoint
    (ndlqr_SolveBatchPolishedAdjoint) with the same gradient assembly; raises when a problem's polish status is not 1.
    infeas_every > 0: primal infeasibility detection every that many iterations (ndlqr_BatchSetInfeasibilityDetection,
    default eps). A problem that is certified infeasible (status 4) does not raise: its z is the last iterate, which solves
    nothing, and it gets zero gradients in every tensor -- the adjoint does not iterate it (w = 0, nu = 0).
    accel_mem > 0: the forward's ADMM takes safeguarded Anderson-accelerated steps with that memory
    (ndlqr_BatchSetBoxAcceleration, default safeguard and weight): fewer iterations to the same convergence test; the
    backward is unchanged (the adjoint's ADMM is not accelerated)."""
    return LqrSolveBox.apply((float(rho), float(alpha), float(eps_abs), float(eps_rel), int(max_iter), int(adapt_every),
                              bool(polish), int(infeas_every), int(accel_mem)),
                             A, B, Q, R, q, r, d, x0, xlo, xhi, ulo, uhi)


# ------------------------------------------------------------------------------------------------ dense cost matrices
def _dense_solve(bs, flat, token, key):
    torch.cuda.current_stream(flat[0].device).synchronize()  # (the library reads torch memory on its own stream)
    bs.initialize_flat_dense(*[_View(t) for t in flat])
    err = bs.solve()
    if err or bs.cholesky_failures() > 0:
        _dense_cache[key][1] = None
        raise RuntimeError("lqr_solve_dense: the factorisation failed (%d non-positive pivots): R or Q - H R^-1 H' are not "
                           "positive definite" % max(bs.cholesky_failures(), 1))
    _dense_cache[key][1] = token


def _dense_gradients(z, w, n, m, N):
    """dL/d(A, B, Q, H, R, q, r, d, x0) [b, ...] in the math convention from the solutions z and the adjoint solutions w
    [b, nvars], both in the caller's variables: the outer products per knot with the signs and per-knot conventions of
    kernels_grad.hpp (zero for A, B, H, R, r, d of the last knot; Q and R as symmetric matrices). They hold for the plain
    dense-cost solve and, with w of the active-set system, for the constrained one (G_A w = 0 drops the constraint term).
    The independent restatement of ndlqr_BatchGradientsDense in torch: tools/grad_dense_bench.py times the kernel against
    it; no backward and no test calls it."""
    zl, zx, zu = split_solution(z, n, m, N)
    wl, wx, wu = split_solution(w, n, m, N)
    outer = lambda a, c: a.unsqueeze(-1) * c.unsqueeze(-2)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0) * (t.dim() - 2) + (0, 1))  # a zero last knot
    zx1, wx1 = zx[:, :N - 1], wx[:, :N - 1]
    gA = pad(-(outer(wl[:, 1:], zx1) + outer(zl[:, 1:], wx1)))
    gB = pad(-(outer(wl[:, 1:], zu) + outer(zl[:, 1:], wu)))
    gQ = -0.5 * (outer(wx, zx) + outer(zx, wx))
    gH = pad(-(outer(wx1, zu) + outer(zx1, wu)))
    gR = pad(-0.5 * (outer(wu, zu) + outer(zu, wu)))
    gq = -wx
    gr = pad(-wu)
    gd = pad(-wl[:, 1:])
    gx0 = -wl[:, 0]
    return (gA, gB, gQ, gH, gR, gq, gr, gd, gx0)


def _dense_named_gradients(bs, shared, needs, dims, device):
    """dL/d(A, B, Q, H, R, q, r, d, x0) from the resident solution and adjoint (ndlqr_BatchGradientsDense)."""
    n, m = dims[:2]
    return _named_gradients(GRAD_DENSE_NAMES, shared, needs, bs.dense_gradient_shape, bs.gradients_dense,
                            dict(A=n, B=n, Q=n, H=n, R=m), device)


class LqrSolveDense(torch.autograd.Function):
    """Forward: ndlqr_InitializeBatchFlatDense + solve with NDLQR_FLAG_KEEP_RECORDS. Backward: one adjoint solve
    (ndlqr_SolveBatchAdjoint) and ndlqr_BatchGradientsDense: the gradients that are asked for, outer products per knot of
    z and w in the caller's variables (zero for A, B, H, R, r, d of the last knot), written by the kernel into torch
    tensors. shared: per argument, whether it came without its batch dimension -- its gradient is the batch sum, computed
    on the device. dims: (n, m, N, b)."""

    @staticmethod
    def forward(ctx, shared, dims, A, B, Q, H, R, q, r, d, x0):
        key, bs = _solver(_dense_cache, A.device, dims)
        flat = _flat((A, B, Q, H, R, q, r, d, x0), shared, dims[3])
        token = next(_tokens)
        _dense_solve(bs, flat, token, key)
        ctx.key, ctx.token, ctx.flat, ctx.dims, ctx.shared = key, token, flat, tuple(dims), shared
        return _solution(bs, A.device)

    @staticmethod
    def backward(ctx, gz):
        bs, gz = _resume(_dense_cache, ctx, gz, lambda bs: _dense_solve(bs, ctx.flat, ctx.token, ctx.key))
        err = bs.solve_adjoint(_View(gz))
        if err:
            raise RuntimeError("lqr_solve_dense backward: adjoint solve failed: %d" % err)
        return (None, None) + tuple(_dense_named_gradients(bs, ctx.shared, ctx.needs_input_grad[2:], ctx.dims, gz.device))


def lqr_solve_dense(A, B, Q, H, R, q, r, d, x0):
    """z [b, nvars] of LQR problems with dense cost matrices and a state-input cross term, differentiable in every argument:
        A [b, N, n, n]   B [b, N, n, m]   Q [b, N, n, n]   H [b, N, n, m]   R [b, N, m, m]   q, d [b, N, n]   r [b, N, m]   x0 [b, n]
    in the row-major math convention; per knot the cost is 1/2 x'Q x + x'H u + 1/2 u'R u + q'x + r'u. Any argument may leave
    out the batch dimension (shared: its gradient is the batch sum). Q and R are read as symmetric matrices through their
    lower triangles, and dL/dQ, dL/dR come back symmetric: the gradient in the space of symmetric matrices. Needs R_k > 0
    and Q_k - H_k R_k^-1 H_k' > 0. H, R of the last knot are not part of the problem (zero gradient), like its A, B, r, d."""
    args = (A, B, Q, H, R, q, r, d, x0)
    _, shared, dims = _check("lqr_solve_dense", _DENSE_ARGS, args, _dense_shapes)
    # (a shared argument goes in as it is: the library sums its gradient over the batch)
    return LqrSolveDense.apply(shared, dims, *args)


# ------------------------------------------------------------------------------------------------ linear inequality constraints
def _lin_solve(bs, flat, settings, token, key):
    """Initialise + constrained solve (cold) of `flat` on the cached solver; it then holds `token`. Returns the mask of
    the problems certified infeasible (status 4: only with infeas_every > 0)."""
    torch.cuda.current_stream(flat[0].device).synchronize()  # (the library reads torch memory on its own stream)
    _lin_cache[key][1] = None
    rho, alpha, eps_abs, eps_rel, max_iter, check_every, adapt_every, infeas_every, infeas_eps = settings
    try:
        bs.set_constraint_adaptation(adapt_every)
        bs.set_constraint_infeasibility(infeas_every, infeas_eps)  # (the cached solver keeps the setting of whoever used it last)
        bs.initialize_flat_constrained(*[_View(t) for t in flat])
        _, status = bs.solve_constrained(rho=rho, alpha=alpha, eps_abs=eps_abs, eps_rel=eps_rel, max_iter=max_iter,
                                         check_every=check_every)
    except RuntimeError as e:
        raise RuntimeError("lqr_solve_constrained: the constrained solve failed (%s)" % e) from None
    infeasible = status == 4  # (certified: z is the last iterate, the gradients are zero)
    _require_converged(status, infeasible, "lqr_solve_constrained: %d of %d problems did not converge (status %s): raise "
                       "max_iter or change rho")
    _lin_cache[key][1] = token
    return infeasible


class LqrSolveConstrained(torch.autograd.Function):
    """Forward: ndlqr_InitializeBatchFlatConstrained + ndlqr_SolveBatchLinConstrained (cold). Backward: the adjoint of the
    active-set system (ndlqr_SolveBatchLinAdjoint, the forward's alpha, tolerances and max_iter); the nine problem
    gradients from z* and w by ndlqr_BatchGradientsDense, those that are asked for, batch-summed on the device for an
    argument that is shared (shared, in the order of the nine), dL/d(C, D, lo, hi) from ndlqr_BatchConstraintGradients --
    batch-summed on the device when every row argument is shared (row_shared), else per problem. dims: (n, m, N, b)."""

    @staticmethod
    def forward(ctx, settings, row_shared, shared, dims, A, B, Q, H, R, q, r, d, x0, C_, D_, lo, hi):
        n, m, N, b = dims
        p = C_.shape[-2]
        key, bs = _solver(_lin_cache, A.device, dims, (p,))
        flat = _flat((A, B, Q, H, R, q, r, d, x0, C_, D_, lo, hi), tuple(shared) + tuple(row_shared), b)
        token = next(_tokens)
        ctx.infeasible = _lin_solve(bs, flat, settings, token, key)
        ctx.key, ctx.token, ctx.flat, ctx.dims, ctx.settings, ctx.row_shared = key, token, flat, (n, m, N, p, b), settings, row_shared
        ctx.shared = shared
        return _solution(bs, A.device)

    @staticmethod
    def backward(ctx, gz):
        n, m, N, p, b = ctx.dims
        bs, gz = _resume(_lin_cache, ctx, gz, lambda bs: _lin_solve(bs, ctx.flat, ctx.settings, ctx.token, ctx.key))
        _, alpha, eps_abs, eps_rel, max_iter, check_every = ctx.settings[:6]
        try:
            _, status = bs.solve_constrained_adjoint(_View(gz), alpha=alpha, eps_abs=eps_abs, eps_rel=eps_rel, max_iter=max_iter,
                                                     check_every=check_every)
        except RuntimeError as e:
            raise RuntimeError("lqr_solve_constrained backward: the adjoint failed (%s)" % e) from None
        # (a certified problem is not iterated: w = 0, nu = 0)
        _require_converged(status, ctx.infeasible, "lqr_solve_constrained backward: the adjoint of %d of %d problems did not "
                           "converge (status %s)")
        need = ctx.needs_input_grad[4:]
        grads = _dense_named_gradients(bs, ctx.shared, need[:9], (n, m, N, b), gz.device)
        need_rows = need[9:]
        wanted = [k for k, nd in zip(_ROW_ARGS, need_rows) if nd]
        summed = bool(wanted) and all(sh for k, sh in zip(_ROW_ARGS, ctx.row_shared) if k in wanted)
        width = dict(C=p * n, D=p * m, lo=p, hi=p)
        out = {k: torch.empty(((N, width[k]) if summed else (b, N, width[k])), dtype=torch.float64, device=gz.device) for k in wanted}
        if out:
            bs.constraint_gradients(summed, {k: _View(v) for k, v in out.items()})
        for k, sh in zip(_ROW_ARGS, ctx.row_shared):
            g = out.get(k)
            if g is not None:
                if sh and not summed:
                    g = g.sum(0)
                if k in ("C", "D"):  # flat column-major -> row-major math convention
                    g = g.reshape(*g.shape[:-1], n if k == "C" else m, p).transpose(-1, -2)
            grads.append(g)
        return (None, None, None, None) + tuple(grads)


def lqr_solve_constrained(A, B, Q, H, R, q, r, d, x0, C, D, lo, hi, *, rho=0.0, alpha=0.0, eps_abs=0.0, eps_rel=0.0,
                          max_iter=0, check_every=0, adapt_every=0, infeas_every=0, infeas_eps=0.0):
    """z* [b, nvars] of the dense-cost LQR problems of lqr_solve_dense subject to, per knot, p rows
        lo_k <= C_k x_k + D_k u_k <= hi_k,     C [b, N, p, n]   D [b, N, p, m]   lo, hi [b, N, p]
    (entries of lo, hi may be +-inf; D of the last knot is not part of the problem), by the solve with linear inequality
    constraints (ndlqr_SolveBatchLinConstrained, cold start; 0 = the library's default for every setting; adapt_every > 0:
    the per-problem adaptive penalty of ndlqr_BatchSetConstraintPenaltyAdaptation, considered every that many iterations,
    0: off; infeas_every > 0: infeasibility detection every that many iterations with the tolerance infeas_eps, 0: 1e-4
    (ndlqr_BatchSetConstraintInfeasibilityDetection) -- a problem certified infeasible (status 4) does not raise: its z is
    the last iterate and every gradient of it is zero), differentiable in all thirteen tensors. Any argument may leave out the batch dimension (shared: its gradient is the batch sum -- for
    C, D, lo, hi computed on the device when all of them that need a gradient are shared). The backward is the adjoint
    of the active-set system (ndlqr_SolveBatchLinAdjoint) with the same alpha, tolerances, max_iter and check_every on the
    forward's factorisation and final penalties. Raises RuntimeError when a problem's forward or adjoint iteration does not converge (status
    != 1). The gradients hold where the active set is locally stable (strict complementarity, independent active rows);
    dL/dC and dL/dD are exactly zero on the rows that are not active."""
    args = (A, B, Q, H, R, q, r, d, x0, C, D, lo, hi)
    _, shared, dims = _check("lqr_solve_constrained", _DENSE_ARGS + _ROW_ARGS, args, _row_shapes)
    # (every argument goes in as it is: the library sums the gradient of a shared one over the batch)
    settings = (float(rho), float(alpha), float(eps_abs), float(eps_rel), int(max_iter), int(check_every), int(adapt_every),
                int(infeas_every), float(infeas_eps))
    return LqrSolveConstrained.apply(settings, shared[9:], shared[:9], dims, *args)


# ------------------------------------------------------------------------------------------------ the optimal value
# J* = min J as a function of the problem (ndlqr_BatchObjective behind a plain solve). By the envelope theorem its
# gradient is the partial derivative of the Lagrangian at the solution -- no adjoint solve, no kept factorisation. The
# Lagrangian that fits the KKT rows of the library (kkt_residual_generic: Q x + q - lambda_k + A' lambda_(k+1) = 0,
# R u + r + B' lambda_(k+1) = 0) is
#     L = J - lambda_0'(x_0 - x_init) + sum_k lambda_(k+1)'(A_k x_k + B_k u_k + d_k - x_(k+1)).

def value_gradients(z, n, m, N, dense):
    """dJ*/d(A, B, Q, R, q, r, d, x0) -- dense: (A, B, Q, H, R, q, r, d, x0) -- per problem, [b, ...] in the math convention,
    from the solutions z [b, nvars]: dJ/dx0 = lambda_0, dJ/dd_k = lambda_(k+1), dJ/dA_k = lambda_(k+1) x_k',
    dJ/dB_k = lambda_(k+1) u_k', dJ/dq = x, dJ/dr = u; diagonal costs dJ/dQ = x*x / 2, dJ/dR = u*u / 2; dense costs
    dJ/dQ = x x' / 2, dJ/dH = x u', dJ/dR = u u' / 2 (symmetric, the convention of lqr_solve_dense). Exactly zero for A, B,
    H, R, r, d of the last knot, which are never read. Torch operations on any device."""
    lam, x, u = split_solution(z, n, m, N)
    outer = lambda a, c: a.unsqueeze(-1) * c.unsqueeze(-2)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0) * (t.dim() - 2) + (0, 1))  # a zero last knot
    x1, l1 = x[:, :N - 1], lam[:, 1:]
    gA, gB = pad(outer(l1, x1)), pad(outer(l1, u))
    gq, gr, gd, gx0 = x.clone(), pad(u), pad(l1), lam[:, 0].clone()
    if dense:
        return (gA, gB, 0.5 * outer(x, x), pad(outer(x1, u)), pad(0.5 * outer(u, u)), gq, gr, gd, gx0)
    return (gA, gB, 0.5 * x * x, pad(0.5 * u * u), gq, gr, gd, gx0)


def _value_forward(ctx, bs, dev, shared, dims):
    """J* [b] of the solution the solver holds (ndlqr_BatchObjective); the solution is saved for the backward."""
    z = _solution(bs, dev)
    J = torch.empty((bs.batch,), dtype=torch.float64, device=dev)
    bs.objective(out={"J": _View(J)})
    ctx.save_for_backward(z)
    ctx.shared, ctx.dims = shared, dims
    return J


def _value_backward(ctx, gJ, dense, needs):
    n, m, N, b = ctx.dims
    (z,) = ctx.saved_tensors
    grads = []
    for g, sh, need in zip(value_gradients(z, n, m, N, dense), ctx.shared, needs):
        if not need:
            grads.append(None)
            continue
        g = g * gJ.reshape((b,) + (1,) * (g.dim() - 1))
        grads.append(g.sum(0) if sh else g)
    return tuple(grads)


class LqrValue(torch.autograd.Function):
    """Forward: a plain solve on lqr_solve's cached solver, then ndlqr_BatchObjective into a torch tensor. Backward: the
    envelope theorem on the saved solution (value_gradients), in torch."""

    @staticmethod
    def forward(ctx, *args):
        dev, shared, dims = _check("lqr_solve", _ARGS, args, _diagonal_shapes)
        key, bs = _solver(_cache, dev, dims)
        _solve(bs, _flat(args, shared, dims[3]), next(_tokens), key)
        return _value_forward(ctx, bs, dev, shared, dims)

    @staticmethod
    def backward(ctx, gJ):
        return _value_backward(ctx, gJ, False, ctx.needs_input_grad)


class LqrValueDense(torch.autograd.Function):
    """LqrValue for dense costs, on lqr_solve_dense's cached solver. shared, dims: as LqrSolveDense's."""

    @staticmethod
    def forward(ctx, shared, dims, *args):
        dev = args[0].device
        key, bs = _solver(_dense_cache, dev, dims)
        _dense_solve(bs, _flat(args, shared, dims[3]), next(_tokens), key)
        return _value_forward(ctx, bs, dev, shared, dims)

    @staticmethod
    def backward(ctx, gJ):
        return (None, None) + _value_backward(ctx, gJ, True, ctx.needs_input_grad[2:])


def lqr_value(A, B, Q, R, q, r, d, x0):
    """J* [b]: the optimal value of the LQR problems of lqr_solve (same shapes, same sharing rules: an argument without its
    batch dimension is shared and its gradient is the batch sum), differentiable in every argument. The forward is a plain
    solve and ndlqr_BatchObjective (double-double, rounded once); the backward needs no adjoint solve: by the envelope
    theorem dJ*/dtheta is the partial derivative of the Lagrangian at the solution (value_gradients). Gradients are zero
    for A, B, R, r, d of the last knot, which are not part of the problem."""
    return LqrValue.apply(A, B, Q, R, q, r, d, x0)


def lqr_value_dense(A, B, Q, H, R, q, r, d, x0):
    """J* [b] of the dense-cost problems of lqr_solve_dense (same shapes and sharing rules), differentiable in every
    argument as lqr_value is; dJ*/dQ and dJ*/dR come back symmetric, the convention of lqr_solve_dense."""
    args = (A, B, Q, H, R, q, r, d, x0)
    _, shared, dims = _check("lqr_value_dense", _DENSE_ARGS, args, _dense_shapes)
    return LqrValueDense.apply(shared, dims, *args)
