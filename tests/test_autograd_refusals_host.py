"""Every refusal of the six entry points of rslqr_amd.autograd, pinned against a recorded list (host, no GPU).

Each refusal is raised before any device call, so the arguments can be fake tensors: under torch's FakeTensorMode a tensor
with device="cuda:0" or "cuda:1" exists on a machine without a GPU. For each entry point the record holds (exception type,
full message) of: every argument as a non-tensor, as float32, on the CPU, on the other device, with a wrong shape per
problem and shared; A not square and with a wrong number of dimensions; B with the wrong N and the wrong n; two batch sizes;
for lqr_solve and lqr_value, Q and R given as matrices; for lqr_solve_box, each bound with a wrong type, dtype, device and
shape, and no bounds at all; for lqr_solve_constrained, C with the wrong N, the wrong n and no rows; lqr_solve's refine out
of range. Shapes n, m, N, b, p = 3, 2, 5, 2, 2. It is compared exactly with tests/golden/autograd_refusals.json.

The fixture is this module's own output at the commit before the autograd layer was rewritten: the recorder uses nothing but
the public functions, so it runs unchanged on any commit --

    python tests/test_autograd_refusals_host.py > tests/golden/autograd_refusals.json
"""
import json
import os
import sys

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rslqr_amd import autograd as AG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autograd_refusals.json")
n, m, N, b, p = 3, 2, 5, 2, 2
DIAG = dict(A=(N, n, n), B=(N, n, m), Q=(N, n), R=(N, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))
BOUNDS = dict(xlo=(N, n), xhi=(N, n), ulo=(N, m), uhi=(N, m))
DENSE = dict(A=(N, n, n), B=(N, n, m), Q=(N, n, n), H=(N, n, m), R=(N, m, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))
ROWS = dict(C=(N, p, n), D=(N, p, m), lo=(N, p), hi=(N, p))
# entry point -> (the shapes of its problem arguments, the shapes of its optional bounds)
ENTRY = {"lqr_solve": (DIAG, {}), "lqr_value": (DIAG, {}), "lqr_solve_box": (DIAG, BOUNDS), "lqr_solve_dense": (DENSE, {}),
         "lqr_value_dense": (DENSE, {}), "lqr_solve_constrained": (dict(DENSE, **ROWS), {})}


def tensor(shape, dtype=torch.float64, device="cuda:0"):
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def wider(shape):
    return tuple(shape[:-1]) + (shape[-1] + 1,)


def variants(shape):
    """(label, replacement) of one argument whose good form is [b, *shape]: each is refused"""
    yield "not a tensor", [0.0]
    yield "float32", tensor((b,) + shape, dtype=torch.float32)
    yield "on the CPU", tensor((b,) + shape, device="cpu")
    yield "on the other device", tensor((b,) + shape, device="cuda:1")
    yield "wrong shape per problem", tensor((b,) + wider(shape))
    yield "wrong shape shared", tensor(wider(shape))
    yield "another batch size", tensor((b + 1,) + shape)
    yield "two dimensions too many", tensor((b, 1) + shape)


def cases():
    """(label, function, positional arguments, keyword arguments), every one of which is refused"""
    for who, (shapes, bounds) in ENTRY.items():
        fn = getattr(AG, who)
        names = list(shapes)
        good = lambda: [tensor((b,) + shapes[k]) for k in names]
        kw = dict(ulo=tensor((b,) + BOUNDS["ulo"])) if bounds else {}

        def swapped(name, t):
            args = good()
            args[names.index(name)] = t
            return args

        for name in names:
            for label, t in variants(shapes[name]):
                yield "%s: %s %s" % (who, name, label), fn, swapped(name, t), kw
        # A and B decide n, m, N: their own messages
        for label, shape in (("not square", (b, N, n, n + 1)), ("not square, shared", (N, n + 1, n)), ("as [n, n]", (n, n)),
                             ("with five dimensions", (1, b, N, n, n))):
            yield "%s: A %s" % (who, label), fn, swapped("A", tensor(shape)), kw
        for label, shape in (("with the wrong N", (b, N + 1, n, m)), ("with the wrong n", (b, N, n + 1, m)),
                             ("with the wrong n, shared", (N, n + 1, m)), ("as [n, m]", (n, m))):
            yield "%s: B %s" % (who, label), fn, swapped("B", tensor(shape)), kw
        yield "%s: every argument shared but q and r, whose batch sizes differ" % who, fn, \
            [tensor(((b,) if k == "q" else (b + 1,) if k == "r" else ()) + shapes[k]) for k in names], kw
        if shapes is DIAG:
            for name, k in (("Q", n), ("R", m)):
                yield "%s: %s as matrices" % (who, name), fn, swapped(name, tensor((b, N, k, k))), kw
                yield "%s: %s as matrices, shared" % (who, name), fn, swapped(name, tensor((N, k, k))), kw
        for bname, shape in bounds.items():
            for label, t in variants(shape):
                yield "%s: %s %s" % (who, bname, label), fn, good(), {bname: t}
            yield "%s: %s for the other kind of bound" % (who, bname), fn, good(), \
                {bname: tensor((b,) + BOUNDS["ulo" if bname[0] == "x" else "xlo"])}
        if bounds:
            yield "%s: no bounds" % who, fn, good(), {}
            yield "%s: a good bound and a bad one" % who, fn, good(), dict(kw, xhi=tensor((N, n), dtype=torch.float32))
        if "C" in shapes:
            for label, shape in (("with the wrong N", (b, N + 1, p, n)), ("with the wrong n", (b, N, p, n + 1)),
                                 ("with the wrong n, shared", (N, p, n + 1)), ("with no rows", (b, N, 0, n)),
                                 ("as [p, n]", (p, n))):
                yield "%s: C %s" % (who, label), fn, swapped("C", tensor(shape)), kw
            yield "%s: D with other rows than C" % who, fn, swapped("D", tensor((b, N, p + 1, m))), kw
    good = [tensor((b,) + DIAG[k]) for k in DIAG]
    for refine in (-1, 9):
        yield "lqr_solve: refine=%d" % refine, AG.lqr_solve, good, dict(refine=refine)


def record():
    out = {}
    with FakeTensorMode():
        for label, fn, args, kw in cases():
            assert label not in out, label
            try:
                fn(*args, **kw)
                out[label] = None  # (ran through: the test refuses such a record)
            except Exception as e:  # noqa: BLE001 (whatever is raised is what the record is about)
                out[label] = [type(e).__name__, str(e)]
    return out


def dump(rec):
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rec.items()) + "\n}\n"


def test_every_case_is_refused_by_a_check_of_the_module():
    got = record()
    assert len(got) > 300
    for label, v in got.items():
        assert v is not None and v[0] in ("TypeError", "ValueError") and v[1].startswith("lqr_"), (label, v)


def test_refusals_match_the_recorded_list():
    want = json.load(open(GOLDEN))
    got = record()
    assert list(got) == list(want)
    differing = [k for k in got if got[k] != want[k]]
    assert not differing, "\n".join("%s:\n  got  %s\n  want %s" % (k, got[k], want[k]) for k in differing[:10])


if __name__ == "__main__":
    sys.stdout.write(dump(record()))
