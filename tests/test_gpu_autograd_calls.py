"""What rslqr_amd.autograd asks of the binding, call by call, pinned against a recorded transcript (on the device).

rslqr_amd.autograd.BatchSolver is replaced by a recording subclass of the real one: it logs every method the module calls
on a solver, in order, and the direct library calls through `bs.L` (the one that sets the bounds of lqr_solve_box) -- the
name and each argument: numbers and booleans by value, raw addresses as "ptr", a _View as its size, a dict as its keys with
sizes. Beside the calls the record holds what each public call returned or raised (shape and dtype of z or J) and, per
input, None or the shape of its gradient. No floating-point result and no iteration count is in it: the values are the
library's, and the gradient tests check them. Shapes n, m, N, b, p = 3, 2, 5, 2, 2 (the padded time axis is in play); the
two infeasible batches are those of test_gpu_box_infeas.py and lin_infeas_support.py. Each case runs in a fresh process
that initialises torch's device first (test_gpu_gradients.py has the reason).

At N = 5 the library refuses the box adjoint, the refinement, the polish and the acceleration ("not available for a padded
horizon"): those cases are recorded as they end, refusal included, and run once more at N = 8, where the whole path runs.

The fixture, tests/golden/autograd_call_transcript.json, is this module's own output on the MI355X at the commit before
the autograd layer was rewritten: the recorder uses nothing but the public functions, so it runs unchanged on any commit --

    python tests/test_gpu_autograd_calls.py > tests/golden/autograd_call_transcript.json
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "autograd_call_transcript.json")
n, m, N, B, P = 3, 2, 5, 2, 2
ARGS = ("A", "B", "Q", "R", "q", "r", "d", "x0")
BOUNDS = ("xlo", "xhi", "ulo", "uhi")
DENSE = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")
ROWS = ("C", "D", "lo", "hi")
BOX_KW = dict(rho=1.0, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)
LIN_KW = dict(rho=1.0, alpha=1.6, eps_abs=1e-9, eps_rel=1e-9, max_iter=20000)


# ---------------------------------------------------------------------------- the recorder
def describe(a):
    import ctypes
    if a is None or isinstance(a, str):
        return a
    if isinstance(a, (bool, np.bool_)):
        return bool(a)
    if isinstance(a, (int, np.integer)):
        return "ptr" if int(a) >= 1 << 32 else int(a)
    if isinstance(a, (float, np.floating)):
        return float(a)
    if isinstance(a, (ctypes._Pointer, ctypes.c_void_p)):
        return "ptr" if ctypes.cast(a, ctypes.c_void_p).value else None
    if isinstance(a, dict):
        return {"dict": [[k, describe(v)] for k, v in a.items()]}
    if isinstance(a, (tuple, list)):
        return [describe(x) for x in a]
    if hasattr(a, "ptr") and hasattr(a, "size"):
        return {"view": int(a.size)}
    return {"other": type(a).__name__}


def recording_solver(log):
    """A subclass of the real BatchSolver that appends [name, arguments, keyword arguments] of every public method called
    from outside (not of the calls the binding makes on itself) and of every call through `L` from outside to `log`."""
    import functools
    import inspect
    from rslqr_amd import api

    class Library:
        def __init__(self, lib, owner):
            self._lib, self._owner = lib, owner

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if self._owner._depth > 0:
                return fn

            def logged(*args):
                log.append(["L." + name, describe(args), {}])
                return fn(*args)
            return logged

    class Recorder(api.BatchSolver):
        _depth = 1  # (the constructor's own calls are the binding's)

        def __init__(self, *args, **kw):
            log.append(["BatchSolver", describe(args), describe(kw)["dict"]])
            super().__init__(*args, **kw)
            self.L = Library(self.L, self)
            self._depth = 0

    def wrap(name, fn):
        @functools.wraps(fn)
        def method(self, *args, **kw):
            if self._depth == 0:
                log.append([name, describe(args), describe(kw)["dict"]])
            self._depth += 1
            try:
                return fn(self, *args, **kw)
            finally:
                self._depth -= 1
        return method

    for name, fn in inspect.getmembers(api.BatchSolver, inspect.isfunction):
        if not name.startswith("_") and name != "close":
            setattr(Recorder, name, wrap(name, fn))
    return Recorder


class Session:
    """the steps of one case: each public call with what it returned or raised and the solver calls it made"""

    def __init__(self):
        from rslqr_amd import autograd
        self.log, self.steps = [], []
        autograd.BatchSolver = recording_solver(self.log)

    def step(self, label, call):
        mark = len(self.log)
        rec, out = {}, None
        try:
            out = call()
            rec["returns"] = out if out is None or isinstance(out, dict) else [list(out.shape), str(out.dtype)]
        except Exception as e:  # noqa: BLE001 (whatever is raised is what the record is about)
            rec["raises"] = [type(e).__name__, str(e)]
        rec["calls"] = self.log[mark:]
        self.steps.append([label, rec])
        return out

    def forward(self, label, fn, *args, **kw):
        return self.step(label, lambda: fn(*args, **kw))

    def backward(self, label, out, leaves):
        """(out * fixed weights).sum().backward(); per leaf None or the gradient's shape"""
        import torch

        def call():
            for v in leaves.values():
                if v is not None:
                    v.grad = None
            w = torch.cos(torch.arange(out.numel(), dtype=torch.float64, device=out.device)).reshape(out.shape)
            (out * w).sum().backward()
            return {k: None if v is None or v.grad is None else list(v.grad.shape) for k, v in leaves.items()}
        return self.step(label, call)


# ---------------------------------------------------------------------------- the problems
def leaf(t, grad=True):
    return t.detach().clone().requires_grad_(grad)


def share(t, names, grad=True):
    """the dict of leaves with those of `names` replaced by their first problem's, without the batch dimension"""
    return {k: leaf(v[0] if k in names else v, grad and v.requires_grad) for k, v in t.items()}


def only(t, names):
    return {k: leaf(v, k in names) for k, v in t.items()}


def diagonal(ndlqr, seed=3100):
    from test_gpu_gradients import _torch_problem
    return _torch_problem(ndlqr, n, m, N, B, seed)


def boxed(ndlqr, seed=3100):
    """the diagonal problem and per-problem bounds that cut its inputs and states"""
    from test_gpu_box_gradients import _torch_bounds
    t = diagonal(ndlqr, seed)
    return dict(t, **_torch_bounds(t, n, m, N, B, "per_problem"))


def dense(scale=1.0):
    import torch
    import cost_support as cs
    probs = cs.family(n, m, N, "moderate")["probs"][:B]
    t = {k: torch.tensor(np.stack([p[k] for p in probs]), dtype=torch.float64, device="cuda", requires_grad=True) for k in DENSE}
    t["q"] = leaf(t["q"] * scale)
    return t


def constrained(scale=1.0):
    """the dense problem with the two dense rows of lin_support.constraint_rows (p = 2)"""
    import torch
    import cost_support as cs
    import lin_support as ls
    fam = cs.family(n, m, N, "moderate")
    rows = [ls.constraint_rows(p, fam["z"][i], 300 + i) for i, p in enumerate(fam["probs"][:B])]
    t = dense(scale)
    for j, k in enumerate(ROWS):
        a = np.stack([r[j][:, m:] for r in rows])
        t[k] = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)
    return t


def values(t, names):
    return [t[k] for k in names]


# ---------------------------------------------------------------------------- the cases
def entry(ndlqr, who):
    """(function, argument names, leaves, keyword arguments) of one entry point at the shapes of this module"""
    from rslqr_amd import autograd as AG
    if who in ("lqr_solve", "lqr_value"):
        return getattr(AG, who), ARGS, diagonal(ndlqr), {}
    if who == "lqr_solve_box":
        return AG.lqr_solve_box, ARGS + BOUNDS, boxed(ndlqr), BOX_KW
    if who in ("lqr_solve_dense", "lqr_value_dense"):
        return getattr(AG, who), DENSE, dense(), {}
    return AG.lqr_solve_constrained, DENSE + ROWS, constrained(), LIN_KW


def pair(s, fn, names, t, kw, label=""):
    out = s.forward("forward" + label, fn, *values(t, names), **kw)
    if out is not None:
        s.backward("backward" + label, out, t)


def _case_plain(ndlqr, s, who):
    fn, names, t, kw = entry(ndlqr, who)
    pair(s, fn, names, t, kw)


def _case_shared(ndlqr, s, who, shared):
    fn, names, t, kw = entry(ndlqr, who)
    if who == "lqr_solve_box":  # (a shared state bound is the widest of the batch: feasible for every problem)
        wide = dict(xlo=lambda v: v.amin(0, keepdim=True), xhi=lambda v: v.amax(0, keepdim=True))
        t = dict(t, **{k: leaf(f(t[k]).expand_as(t[k])) for k, f in wide.items() if k in shared})
    pair(s, fn, names, share(t, shared), kw)


def _case_needs(ndlqr, s, who):
    fn, names, t, kw = entry(ndlqr, who)
    pair(s, fn, names, only(t, ("B", "r")), kw)


def _case_options(ndlqr, s, who, options):
    fn, names, t, kw = entry(ndlqr, who)
    pair(s, fn, names, t, dict(kw, **options))


def _case_eviction(ndlqr, s, who):
    """two forwards on one cached solver, then the backward of the first and of the second"""
    fn, names, t1, kw = entry(ndlqr, who)
    t2 = {k: leaf(v * 0.9 if k == "q" else v) for k, v in t1.items()}
    z1 = s.forward("forward 1", fn, *values(t1, names), **kw)
    z2 = s.forward("forward 2", fn, *values(t2, names), **kw)
    s.backward("backward 1", z1, t1)
    s.backward("backward 2", z2, t2)


def _case_infeasible_box(ndlqr, s):
    import torch
    from rslqr_amd.autograd import lqr_solve_box
    from support import Oracle
    from test_gpu_box_infeas import ALPHA, EPS_ADMM, EVERY, Case, stack
    case = Case(ndlqr, Oracle(), "compact")
    t = {}
    for k, a in zip(ARGS, stack(case.probs)):
        if k in ("A", "B"):
            a = a.reshape(case.batch, case.N, case.n if k == "A" else case.m, case.n).transpose(0, 1, 3, 2)
        t[k] = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda", requires_grad=True)
    t["xlo"] = None
    for k, a in zip(BOUNDS[1:], case.bounds[1:]):
        t[k] = torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    kw = dict(rho=case.rho, alpha=ALPHA, eps_abs=EPS_ADMM, eps_rel=EPS_ADMM, max_iter=2000, infeas_every=EVERY)
    pair(s, lqr_solve_box, ARGS + BOUNDS, t, kw)


def _case_infeasible_constrained(ndlqr, s):
    import torch
    import lin_infeas_support as li
    from rslqr_amd.autograd import lqr_solve_constrained
    inst = li.instance(6, 3, 5, "A")
    arr = {k: np.stack([c["p"][k] for c in inst]) for k in DENSE}
    arr.update({k: np.stack([c[k] for c in inst]) for k in ROWS})
    t = {k: torch.tensor(np.ascontiguousarray(arr[k]), dtype=torch.float64, device="cuda", requires_grad=True) for k in DENSE + ROWS}
    kw = dict(rho=li.RHO, alpha=li.ALPHA, eps_abs=1e-9, eps_rel=1e-9, max_iter=4000, infeas_every=li.EVERY, infeas_eps=0.0)
    pair(s, lqr_solve_constrained, DENSE + ROWS, t, kw)


def _case_indefinite(ndlqr, s, who):
    """a cost that is not positive definite is refused; a valid forward on the same cached solver then succeeds"""
    fn, names, t, kw = entry(ndlqr, who)
    bad = {k: v.detach().clone() for k, v in t.items()}
    bad["Q"][:, 1] = -bad["Q"][:, 1]
    s.forward("forward, Q of knot 1 negated", fn, *values(bad, names), **kw)
    pair(s, fn, names, t, kw, " after it")


def _case_one_iteration(ndlqr, s, who):
    fn, names, t, kw = entry(ndlqr, who)
    s.forward("forward, max_iter=1", fn, *values(t, names), **dict(kw, max_iter=1))


def _case_crossed_bounds(ndlqr, s):
    fn, names, t, kw = entry(ndlqr, "lqr_solve_box")
    t = dict(t, ulo=t["uhi"], uhi=leaf(t["ulo"] - 1.0))
    s.forward("forward, ulo > uhi", fn, *values(t, names), **kw)


SIX = ("lqr_solve", "lqr_solve_box", "lqr_solve_dense", "lqr_solve_constrained", "lqr_value", "lqr_value_dense")
CASES = {}  # label -> (case function, arguments); a label that ends in PADDED_FREE runs at N = 8
PADDED_FREE = " (N = 8)"
PADDED_REFUSAL = "not available for a padded horizon (horizon 5 runs as 8 knots); use a power-of-two horizon"
for _who in SIX:
    CASES["%s: every argument per problem" % _who] = ("_case_plain", (_who,))
for _who, _shared, _label in (("lqr_solve", ("A", "q"), "A and q shared"), ("lqr_solve_dense", ("A", "q"), "A and q shared"),
                              ("lqr_solve_box", BOUNDS, "every bound shared"), ("lqr_solve_box", ("xlo",), "xlo shared"),
                              ("lqr_solve_constrained", ROWS, "every row argument shared"),
                              ("lqr_solve_constrained", ("C",), "C shared")):
    CASES["%s: %s" % (_who, _label)] = ("_case_shared", (_who, _shared))
for _who in SIX:
    CASES["%s: only B and r require a gradient" % _who] = ("_case_needs", (_who,))
for _who, _options in (("lqr_solve", dict(refine=2)), ("lqr_solve_box", dict(polish=True, eps_abs=1e-3, eps_rel=1e-3)),
                       ("lqr_solve_box", dict(accel_mem=3, adapt_every=10)), ("lqr_solve_constrained", dict(adapt_every=10))):
    CASES["%s: %s" % (_who, ", ".join("%s=%s" % kv for kv in _options.items()))] = ("_case_options", (_who, _options))
for _who in SIX[:4]:
    CASES["%s: backwards after the cached solver has moved on" % _who] = ("_case_eviction", (_who,))
CASES["lqr_solve_box: one infeasible problem, infeas_every > 0"] = ("_case_infeasible_box", ())
CASES["lqr_solve_constrained: one infeasible problem, infeas_every > 0"] = ("_case_infeasible_constrained", ())
for _who in ("lqr_solve", "lqr_solve_dense"):
    CASES["%s: Q not positive definite" % _who] = ("_case_indefinite", (_who,))
for _who in ("lqr_solve_box", "lqr_solve_constrained"):
    CASES["%s: max_iter=1" % _who] = ("_case_one_iteration", (_who,))
CASES["lqr_solve_box: ulo > uhi"] = ("_case_crossed_bounds", ())
REFUSED_WHEN_PADDED = [k for k in CASES if ("lqr_solve_box" in k and "infeasible" not in k and "max_iter=1" not in k
                                            and "ulo > uhi" not in k) or "refine=2" in k]
for _label in REFUSED_WHEN_PADDED:
    CASES[_label + PADDED_FREE] = CASES[_label]


def child(label):
    """runs in the fresh process: prints the record of one case as a line of JSON"""
    import rslqr_amd
    global N
    if label.endswith(PADDED_FREE):
        N = 8
    name, args = CASES[label]
    s = Session()
    globals()[name](rslqr_amd, s, *args)
    print("RECORD " + json.dumps(s.steps))


def record(label):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import torch; torch.zeros(1, device='cuda')\n"
            "import test_gpu_autograd_calls as T\n"
            "T.child(%r)\n" % (os.path.dirname(HERE), HERE, label))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
    assert r.returncode == 0 and len(lines) == 1, (label, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[0][len("RECORD "):])


@pytest.mark.parametrize("label", list(CASES))
def test_calls_returns_and_gradient_shapes_match_the_recorded_transcript(label):
    want = json.load(open(GOLDEN))[label]
    got = record(label)
    assert [s[0] for s in got] == [s[0] for s in want]
    for (step, g), (_, w) in zip(got, want):
        assert g == w, "%s, %s:\n  got  %s\n  want %s" % (label, step, json.dumps(g), json.dumps(w))


def test_every_case_is_in_the_transcript_and_ends_as_the_issue_says():
    want = json.load(open(GOLDEN))
    assert list(want) == list(CASES)
    raised = {label: [rec["raises"][1] for _, rec in steps if "raises" in rec] for label, steps in want.items()}
    for label, msgs in raised.items():
        if "not positive definite" in label:
            assert len(msgs) == 1 and "the factorisation failed" in msgs[0] and "returns" in want[label][1][1], label
        elif "max_iter=1" in label:
            assert len(msgs) == 1 and "did not converge" in msgs[0], label
        elif "ulo > uhi" in label:
            assert len(msgs) == 1 and "the bounds were refused" in msgs[0], label
        elif label in REFUSED_WHEN_PADDED:  # (each step that reaches the refused call, and nothing else)
            assert msgs and all(PADDED_REFUSAL in msg for msg in msgs), (label, msgs)
        else:
            assert not msgs, (label, msgs)


if __name__ == "__main__":
    out = {}
    for label in CASES:
        out[label] = record(label)
        sys.stderr.write("recorded %s\n" % label)
    sys.stdout.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")
