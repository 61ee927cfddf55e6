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

Process start-up: torch ships its own HIP runtime next to the system one this library links. Initialise torch's device
(any CUDA tensor) before the library's first device call in a process; the other order may leave torch without a device.
"""
import itertools

import torch

from .api import BatchSolver, FLAG_KEEP_RECORDS, GRAD_NAMES

_ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
_cache = {}                  # (n, m, N, b, device index) -> [BatchSolver, token of the forward it holds]
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


def _check(args):
    dev = None
    for name, t in zip(_ARGS, args):
        if not isinstance(t, torch.Tensor):
            raise TypeError("lqr_solve: %s must be a torch.Tensor" % name)
        if t.dtype != torch.float64:
            raise TypeError("lqr_solve: %s must be float64, got %s" % (name, t.dtype))
        if t.device.type != "cuda":
            raise ValueError("lqr_solve: %s must live on a ROCm device, got %s" % (name, t.device))
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("lqr_solve: every argument must be on one device (%s is on %s, A on %s)" % (name, t.device, dev))
    A, B = args[0], args[1]
    if A.dim() not in (3, 4) or A.shape[-1] != A.shape[-2]:
        raise ValueError("lqr_solve: A must be [b, N, n, n] or [N, n, n], got %s" % (tuple(A.shape),))
    N, n = A.shape[-3], A.shape[-1]
    if B.dim() not in (3, 4) or B.shape[-3] != N or B.shape[-2] != n:
        raise ValueError("lqr_solve: B must be [b, N, n, m] or [N, n, m], got %s" % (tuple(B.shape),))
    m = B.shape[-1]
    per = dict(A=(N, n, n), B=(N, n, m), Q=(N, n), R=(N, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))
    batch = set()
    shared = []
    for name, t in zip(_ARGS, args):
        shape = per[name]
        if tuple(t.shape) == shape:
            shared.append(True)
        elif t.dim() == len(shape) + 1 and tuple(t.shape[1:]) == shape:
            shared.append(False)
            batch.add(t.shape[0])
        elif name in ("Q", "R") and t.dim() >= 3 and t.shape[-1] == t.shape[-2] == shape[-1]:
            raise ValueError("lqr_solve: %s must hold the diagonals, [b, N, %d] or [N, %d]; got the matrices %s"
                             % (name, shape[-1], shape[-1], tuple(t.shape)))
        else:
            raise ValueError("lqr_solve: %s must be [b, %s] or %s, got %s"
                             % (name, ", ".join(str(x) for x in shape), list(shape), tuple(t.shape)))
    if len(batch) > 1:
        raise ValueError("lqr_solve: batch dimensions disagree: %s" % sorted(batch))
    b = batch.pop() if batch else 1
    return dev, n, m, N, b, shared


def _flat(args, n, m, N, b, shared):
    """The flat layout of ndlqr_InitializeBatchFlat, contiguous on the device: A, B column-major (A^T stored row-major)."""
    out = []
    for name, t, sh in zip(_ARGS, args, shared):
        t = t.detach()
        if sh:
            t = t.unsqueeze(0)
        if name in ("A", "B"):
            t = t.transpose(-1, -2)
        t = t.expand(b, *t.shape[1:]).contiguous().reshape(b, -1)
        out.append(t)
    return out


def _solve(bs, flat, token, key):
    """Factor + solve of `flat` on the cached solver; the solver then holds forward `token`."""
    torch.cuda.current_stream(flat[0].device).synchronize()  # (the library reads torch memory on its own stream)
    bs.initialize_flat_device(*[t.data_ptr() for t in flat])
    err = bs.solve()
    if err or bs.cholesky_failures() > 0:
        _cache[key][1] = None
        raise RuntimeError("lqr_solve: the factorisation failed (%d non-positive pivots): Q, R or the problem are not "
                           "positive definite" % max(bs.cholesky_failures(), 1))
    _cache[key][1] = token


class LqrSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        dev, n, m, N, b, shared = _check(args)
        key = (n, m, N, b, dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in _cache:
            _cache[key] = [BatchSolver(n, m, N, b, device=key[4], flags=FLAG_KEEP_RECORDS), None]
        bs = _cache[key][0]
        flat = _flat(args, n, m, N, b, shared)
        token = next(_tokens)
        _solve(bs, flat, token, key)
        z = torch.empty((b, bs.nvars), dtype=torch.float64, device=dev)
        bs.solutions_to_device(z.data_ptr())
        bs.synchronize()
        ctx.key, ctx.token, ctx.flat, ctx.shared, ctx.dims = key, token, flat, shared, (n, m, N, b)
        return z

    @staticmethod
    def backward(ctx, gz):
        n, m, N, b = ctx.dims
        bs = _cache[ctx.key][0]
        if _cache[ctx.key][1] != ctx.token:  # the solver has served another forward since: this node's factorisation again
            _solve(bs, ctx.flat, ctx.token, ctx.key)
        gz = gz.detach().to(torch.float64).contiguous()
        torch.cuda.current_stream(gz.device).synchronize()
        err = bs.solve_adjoint(_View(gz))
        if err:
            raise RuntimeError("lqr_solve backward: adjoint solve failed: %d" % err)
        mask = 0
        out, views = {}, {}
        for i, (name, sh, need) in enumerate(zip(GRAD_NAMES, ctx.shared, ctx.needs_input_grad)):
            if not need:
                continue
            if sh:
                mask |= 1 << i
            out[name] = torch.empty(bs.gradient_shape(name, sh), dtype=torch.float64, device=gz.device)
            views[name] = _View(out[name])
        if views:
            bs.gradients(mask, views)
        grads = []
        for name, sh in zip(GRAD_NAMES, ctx.shared):
            g = out.get(name)
            if g is not None and name in ("A", "B"):  # flat column-major -> row-major math convention
                cols = n if name == "A" else m
                g = g.reshape(*g.shape[:-1], cols, n).transpose(-1, -2)
            grads.append(g)
        return tuple(grads)


def lqr_solve(A, B, Q, R, q, r, d, x0):
    """z [b, nvars] of the LQR problems (see the module docstring), differentiable in every argument."""
    return LqrSolve.apply(A, B, Q, R, q, r, d, x0)


__all__ = ["LqrSolve", "lqr_solve", "split_solution"]
