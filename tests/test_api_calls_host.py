"""What rslqr_amd.api hands to the C library, call by call, pinned against a recorded transcript (host, no GPU).

A BatchSolver made with BatchSolver.__new__ runs over a stub library: every attribute of the stub is a function that
records its name and the kind of each argument and returns a chosen code; ndlqr_hip_last_error returns b"stub". Every
public method that reaches the library runs with return code 0 and with return code 7 (and the read-outs that return
nvars also with that), and the record -- the C calls in order, what the method returned or raised, the attributes it
left -- is compared exactly with tests/golden/api_call_transcript.json.

The fixture is this module's own output at the commit before the binding was refactored: the recorder uses nothing but
the public methods, so it runs unchanged on any commit --

    python tests/test_api_calls_host.py > tests/golden/api_call_transcript.json

The entries of INT_DESTINATION_CASES are the one intended difference (a numpy destination of the wrong dtype was written
through by the C side; it is a ValueError now): they stay in the fixture as recorded and are asserted on their own.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rslqr_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_call_transcript.json")
n, m, N, B, P, NVARS = 3, 2, 4, 2, 2, 30
DEV0 = 0x7D0000000000  # the fake device addresses start here
INT_DESTINATION_CASES = ("polish_box[float64 steps]", "polish_constrained[float64 status]",
                         "solve_polished_adjoint[float64 steps]")
INT_MESSAGE = "expected a C-contiguous int32 array of %d entries" % B
NO_LIBRARY = {"slice_width", "gradient_shape", "dense_gradient_shape"}  # public methods that never reach the library


class Dev(api.DeviceArray):
    """the two-field fake of device memory: `ptr` and `size` (a DeviceArray by class alone, for the isinstance checks)"""
    count = 0

    def __init__(self, size):
        Dev.count += 1
        self.ptr, self.size = DEV0 + Dev.count * 0x100000, int(size)


def kind(a):
    if a is None:
        return "null"
    if isinstance(a, (bool, np.bool_)):
        return ["bool", bool(a)]
    if isinstance(a, (int, np.integer)):
        return ["int", int(a)]
    if isinstance(a, (float, np.floating)):
        return ["float", float(a)]
    if type(a).__name__ == "CArgObject":  # C.byref(...)
        a = a._obj
        if isinstance(a, C.Structure):
            return ["struct", type(a).__name__, [getattr(a, f[0]) for f in a._fields_]]
        return ["byref", type(a).__name__]
    if isinstance(a, (C._Pointer, C.c_void_p, C.c_char_p, C.Array)):
        addr = C.cast(a, C.c_void_p).value
        return "null" if not addr else "device" if DEV0 <= addr < DEV0 + (1 << 40) else "host"
    return ["other", type(a).__name__]


class Stub:
    def __init__(self, code):
        self.code, self.calls = code, []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "ndlqr_hip_last_error":
            return lambda: b"stub"

        def fn(*args):
            self.calls.append([name] + [kind(a) for a in args])
            return b"stub" if name == "ndlqr_hip_schedule" else self.code  # (the one other call that returns a string)
        return fn


def describe(v, given):
    if v is None:
        return None
    if isinstance(v, Dev):
        return ["device", v.size] + (["given"] if id(v) in given else [])
    if isinstance(v, np.ndarray):
        return ["ndarray", list(v.shape), str(v.dtype)] + (["given"] if id(v) in given else [])
    if isinstance(v, dict):
        return ["dict", [[k, describe(x, given)] for k, x in v.items()]]
    if isinstance(v, (tuple, list)):
        return [type(v).__name__, [describe(x, given) for x in v]]
    if isinstance(v, (bool, int, float, str, np.generic)):
        return [type(v).__name__, v.item() if isinstance(v, np.generic) else v]
    return ["other", type(v).__name__]


def make(code):
    bs = api.BatchSolver.__new__(api.BatchSolver)
    bs.L = Stub(code)
    bs.n, bs.m, bs.N, bs.batch, bs.nvars, bs.h = n, m, N, B, NVARS, 1
    bs._sel, bs._step_refs, bs._rows, bs._accel_mem = None, [], P, 0
    return bs


def z(*shape, dtype=np.float64):
    return np.zeros(shape, dtype=dtype)


def flat8(dev=False):
    shapes = [(B, N, n * n), (B, N, n * m), (B, N, n), (B, N, m), (B, N, n), (B, N, m), (B, N, n), (B, n)]
    return [Dev(np.prod(s)) if dev else z(*s) for s in shapes]


def dense9(dev=False, p=None):
    shapes = [(B, N, n * n), (B, N, n * m), (B, N, n * n), (B, N, n * m), (B, N, m * m), (B, N, n), (B, N, m), (B, N, n), (B, n)]
    if p is not None:
        shapes += [(B, N, p * n), (B, N, p * m)]
    return [Dev(np.prod(s)) if dev else z(*s) for s in shapes]


def rhs4(dev=False):
    shapes = [(B, N, n), (B, N, m), (B, N, n), (B, n)]
    return [Dev(np.prod(s)) if dev else z(*s) for s in shapes]


def flatten(v):
    if isinstance(v, dict):
        v = list(v.values())
    if isinstance(v, (tuple, list)):
        return [y for x in v for y in flatten(x)]
    return [v]


CASES = []  # (label, method, factory of (args, kwargs), setup or None, return codes)


def case(label, factory=lambda: ((), {}), setup=None, codes=(0, 7)):
    CASES.append((label, label.split("[")[0], factory, setup, codes))


def a(*args, **kwargs):
    return lambda: (args, kwargs)


def no_rows(bs):
    bs._rows = 0


# ---- life cycle, flags, the diagonal initialisers
case("close")
case("set_flags", a(8))
case("ctx")
case("initialize_flat", lambda: (flat8(), {}))
case("initialize_flat[lists]", lambda: ([x.tolist() for x in flat8()], {}))
case("initialize_flat[bad size]", lambda: ([z(B, N, n)] + flat8()[1:], {}))
case("initialize_flat_device", a(*range(4096, 4096 + 8 * 64, 64)))
case("initialize_synthetic", a(11))
case("set_rhs_flat", lambda: (rhs4(), {}))
# ---- dense-cost mode
case("initialize_flat_dense", lambda: (dense9(), {}))
case("initialize_flat_dense[device]", lambda: (dense9(dev=True), {}))
case("initialize_flat_dense[mixed, no H]", lambda: (dense9()[:3] + [None] + dense9(dev=True)[4:], {}))
case("initialize_flat_dense[float32]", lambda: ([x.astype(np.float32) for x in dense9()], {}))
case("initialize_flat_dense[no Q]", lambda: (dense9()[:2] + [None] + dense9()[3:], {}))
case("initialize_flat_dense[bad size]", lambda: (dense9()[:8] + [z(n)], {}))
case("initialize_flat_dense[bad device size]", lambda: ([Dev(5)] + dense9()[1:], {}))
case("cost_is_dense")
case("cost_phase_ms")
case("cost_reduction")
# ---- linear inequality constraints
for label, lohi in (("(p,)", lambda p: [z(p), z(p)]), ("(N, p)", lambda p: [z(N, p), z(N, p)]),
                    ("(batch, N, p)", lambda p: [z(B, N, p), z(B, N, p)]), ("(p,) and (batch, N, p)", lambda p: [z(p), z(B, N, p)]),
                    ("device", lambda p: [Dev(B * N * p), Dev(B * N * p)]), ("(p,) and device", lambda p: [z(p), Dev(B * N * p)]),
                    ("lists", lambda p: [[0.0] * p, [[1.0] * p] * N]), ("bad shape", lambda p: [z(p + 1), z(p)]),
                    ("bad device size", lambda p: [Dev(N * p), Dev(N * p)]), ("None", lambda p: [None, z(p)])):
    case("initialize_flat_constrained[bounds %s]" % label, lambda lohi=lohi: (dense9(p=3) + lohi(3), {}))
    case("set_constraint_bounds[%s]" % label, lambda lohi=lohi: (lohi(P), {}))
case("initialize_flat_constrained[device, no H]", lambda: (dense9(dev=True, p=3)[:3] + [None] + dense9(dev=True, p=3)[4:] + [z(3), z(3)], {}))
case("initialize_flat_constrained[no A]", lambda: ([None] + dense9(p=3)[1:] + [z(3), z(3)], {}))
case("initialize_flat_constrained[bad size of C]", lambda: (dense9() + [z(B, N, n + 1), z(B, N, m), z(1), z(1)], {}))
case("initialize_flat_constrained[bad size of D]", lambda: (dense9() + [z(B, N, 3 * n), z(B, N, m), z(3), z(3)], {}))
case("is_constrained")
case("set_constraint_bounds[before initialize_flat_constrained]", lambda: ([z(P), z(P)], {}), setup=no_rows)
case("solve_constrained")
case("solve_constrained[settings]", a(0.5, 1.5, 1e-5, 1e-6, 50, 5, True, 0))
case("solve_constrained[adapt_every]", a(adapt_every=3))
case("set_constraint_adaptation")
case("set_constraint_adaptation[settings]", a(4, 1e-3, 1e3))
case("constraint_penalties")
case("constraint_penalties[host]", lambda: ((z(B),), {}))
case("constraint_penalties[device]", lambda: ((Dev(B),), {}))
case("constraint_penalties[bad size]", lambda: ((z(B + 1),), {}))
case("set_constraint_infeasibility")
case("set_constraint_infeasibility[settings]", a(5, 1e-3))
case("constraint_infeasibility_certificate")
case("constraint_infeasibility_certificate[host, device]", lambda: ((z(B, N, n), Dev(B * N * P)), {}))
case("constraint_multipliers")
case("constraint_residuals")
case("constraint_reduction")
case("solve_constrained_adjoint", lambda: ((z(B, NVARS),), {}))
case("solve_constrained_adjoint[device, settings]", lambda: ((Dev(B * NVARS), 1.5, 1e-5, 1e-6, 50, 5), {}))
case("solve_constrained_adjoint[float32]", lambda: ((z(B, NVARS, dtype=np.float32),), {}))
case("solve_constrained_adjoint[bad size]", lambda: ((z(B, NVARS + 1),), {}))
case("constraint_gradients")
case("constraint_gradients[summed]", a(summed=True))
case("constraint_gradients[out]", lambda: ((), dict(out=dict(lo=z(B, N, P), D=Dev(B * N * P * m), C=None))))
case("constraint_gradients[summed, out]", lambda: ((True, dict(hi=z(N, P))), {}))
case("constraint_gradients[unknown]", lambda: ((), dict(out=dict(lo=z(B, N, P), xlo=z(B, N, n)))))
case("constraint_gradients[bad size]", lambda: ((), dict(out=dict(lo=z(N, P)))))
case("constraint_adjoint_multipliers")
case("constraint_codes")
case("constraint_polish_codes")
case("constraint_polish_residual", lambda: ((z(B, NVARS), z(B, N, P), z(B, N, P, dtype=np.uint8), z(B)), {}))
case("constraint_polish_residual[poison_pad]", lambda: ((z(B, NVARS), z(B, N, P), z(B, N, P), z(B), True), {}))
case("constraint_polish_phase_ms")
case("constraint_polish_state")
case("constraint_polish_state[max_steps]", a(max_steps=3))
case("constraint_adjoint_iterate")
# ---- the int32 destinations
for method in ("infeasibility_measures", "constraint_infeasibility_measures"):
    case(method)
    case(method + "[host]", lambda: ((z(B, 4), z(B, dtype=np.int32)), {}))
    case(method + "[device]", lambda: ((Dev(4 * B), Dev(B)), {}))
    case(method + "[float64 iteration]", lambda: ((None, z(B)), {}))
    case(method + "[bad size of iteration]", lambda: ((None, z(B + 1, dtype=np.int32)), {}))
    case(method + "[strided iteration]", lambda: ((None, z(B, 2, dtype=np.int32)[:, 0]), {}))
    case(method + "[bad size of measures]", lambda: ((z(B, 3),), {}))
for method, lead in (("polish_box", ()), ("polish_constrained", ()), ("solve_polished_adjoint", None)):
    g = (lambda: (z(B, NVARS),)) if lead is None else (lambda: ())
    case(method, lambda g=g: (g(), {}))
    case(method + "[host]", lambda g=g: (g(), dict(steps=z(B, dtype=np.int32), status=z(B, dtype=np.int32))))
    case(method + "[device]", lambda g=g: (g(), dict(steps=Dev(B), status=Dev(B))))
    case(method + "[host steps, device status]", lambda g=g: (g(), dict(steps=z(B, dtype=np.int32), status=Dev(B))))
case("polish_box[settings]", a(1e-6, 4, 3))
case("polish_constrained[settings]", a(1e-6, 4, 3))
case("solve_polished_adjoint[device, max_steps]", lambda: ((Dev(B * NVARS), 4), {}))
case("solve_polished_adjoint[bad size]", lambda: ((z(B, NVARS - 1),), {}))
case(INT_DESTINATION_CASES[0], lambda: ((), dict(steps=z(B))))
case(INT_DESTINATION_CASES[1], lambda: ((), dict(status=z(B))))
case(INT_DESTINATION_CASES[2], lambda: ((z(B, NVARS),), dict(steps=z(B))))
# ---- the solves and steps
case("solve")
case("solve_rhs_only")
case("solve_async")
case("solve_multi_rhs", lambda: ([z(2, *x.shape) for x in rhs4()], {}))
case("solve_multi_rhs[out]", lambda: ([z(2, *x.shape) for x in rhs4()], dict(out=z(2, B, NVARS))))
case("solve_multi_rhs[selection]", lambda: ([z(2, *x.shape) for x in rhs4()], dict(selection=(1, 2, 6))))
case("solve_multi_rhs[selection, out]", lambda: ([z(2, *x.shape) for x in rhs4()], dict(selection=(1, 2, 6), out=z(2, B, 2, n + m))))
case("solve_multi_rhs[bad shape]", lambda: ([z(2, B, N, m)] + [z(2, *x.shape) for x in rhs4()][1:], {}))
case("set_step_selection")
case("set_step_selection[slice]", a(1, 2, 6))
case("solve_slices_async", lambda: ((1, 2, 6, z(B, 2, n + m)), {}))
case("solve_slices_async[device]", lambda: ((1, 2, 6, Dev(B * 2 * (n + m))), {}))
case("solve_slices_async[bad size]", lambda: ((1, 2, 6, z(B, 2, n)), {}))
case("solution_slices", a(1, 2, 7))
case("solution_slices[out]", lambda: ((1, 2, 7, z(B, 2, 2 * n + m)), {}))
case("solution_slices[bad size]", lambda: ((1, 2, 7, z(B, 2, n)), {}))
case("step_async", lambda: (rhs4() + [z(B, NVARS)], {}))
case("step_async[device]", lambda: (rhs4(dev=True) + [Dev(B * NVARS)], {}))
case("step_async[x0 alone]", lambda: ([None, None, None, z(B, n), z(B, NVARS)], {}))
case("step_async[selection]", lambda: (rhs4() + [z(B, 2, n + m)], {}), setup=lambda bs: bs.set_step_selection(1, 2, 6))
case("step_async[bad size]", lambda: (rhs4() + [z(B, NVARS + 1)], {}))
case("step_async[no x0]", lambda: (rhs4()[:3] + [None, z(B, NVARS)], {}))
case("step_dense_async", lambda: (rhs4() + [z(B, NVARS)], {}))
case("step_dense_async[device]", lambda: (rhs4(dev=True) + [Dev(B * NVARS)], {}))
case("step_dense_async[x0 alone, selection]", lambda: ([None, None, None, z(B, n), z(B, 2, n + m)], dict(selection=(1, 2, 6))))
case("step_dense_async[q without r]", lambda: ([z(B, N, n), None, None, z(B, n), z(B, NVARS)], {}))
case("step_dense_async[no out]", lambda: (rhs4() + [None], {}))
case("step_dense_async[bad size]", lambda: (rhs4() + [z(B, NVARS + 1)], {}))
case("step_dense_async[refused]", lambda: (rhs4() + [z(B, NVARS)], {}), codes=(api.ERR_INVALID,))
case("solve_slices_dense_async", lambda: ((1, 2, 6, z(B, 2, n + m)), {}))
case("solve_slices_dense_async[device]", lambda: ((1, 2, 6, Dev(B * 2 * (n + m))), {}))
case("solve_slices_dense_async[bad size]", lambda: ((1, 2, 6, z(B, 2, n)), {}))
case("solve_slices_dense_async[refused]", lambda: ((1, 2, 6, z(B, 2, n + m)), {}), codes=(api.ERR_INVALID,))
case("solution_slices_dense", a(1, 2, 7))
case("solution_slices_dense[device]", lambda: ((1, 2, 7, Dev(B * 2 * (2 * n + m))), {}))
case("solution_slices_dense[bad size]", lambda: ((1, 2, 7, z(B, 2, n)), {}))
case("rhs_raw")
case("time_shard_top_doubles", a(2))
case("time_shard_factor", a(1, 2))
case("time_shard_export", a(2, 4096))
case("time_shard_import", a(2, 4096))
case("time_shard_finish", a(1, 2))
case("synchronize_previous")
case("synchronize", setup=lambda bs: bs.step_async(*(rhs4() + [z(B, NVARS)])))
case("solve_ms")
# ---- read-outs of the plain solve
case("solution", a(1), codes=(0, 7, NVARS))
case("solutions", codes=(0, 7, NVARS))
case("solutions[out]", lambda: ((z(B, NVARS),), {}), codes=(0, 7, NVARS))
case("solutions[bad size]", lambda: ((z(B, NVARS + 1),), {}))
case("solutions_to_device", a(4096), codes=(0, 7, NVARS))
case("kkt_residuals")
case("upload_packed", lambda: ((z(8), z(8), z(8)), {}))
case("factors", a(1))
case("cholesky_failures")
case("cholesky_failure_counts")
case("factor_count")
case("profile")
case("schedule")
case("compact_level1")
case("level1_paired")
case("bottom_lds16")
case("set_pipeline_depth", a(2))
case("pipeline_depth")
case("profile_reset")
# ---- adjoint, gradients, gains, objective, refinement
case("solve_adjoint", lambda: ((z(B, NVARS),), {}))
case("solve_adjoint[device]", lambda: ((Dev(B * NVARS),), {}))
case("solve_adjoint[bad size]", lambda: ((z(B, NVARS + 1),), {}))
case("adjoint", codes=(0, 7, NVARS))
case("adjoint[device]", lambda: ((Dev(B * NVARS),), {}), codes=(0, 7, NVARS))
case("adjoint[bad size]", lambda: ((z(B, NVARS + 1),), {}))
for method, names, wide in (("gradients", api.GRAD_NAMES, n), ("gradients_dense", api.GRAD_DENSE_NAMES, n * n)):
    case(method)
    case(method + "[sum_mask]", a(sum_mask=1 | 4 | (1 << (len(names) - 1))))
    case(method + "[out]", lambda wide=wide: ((), dict(out=dict(Q=z(B, N, wide), x0=Dev(B * n), A=None))))
    case(method + "[sum_mask, out]", lambda wide=wide: ((4, dict(Q=z(N, wide), B=z(B, N, n * m))), {}))
    case(method + "[unknown]", lambda: ((), dict(out=dict(q=z(B, N, n), C=z(B, N, n)))))
    case(method + "[bad size]", lambda wide=wide: ((), dict(out=dict(Q=z(N, wide)))))
case("feedback_gains")
case("feedback_gains[knots, want]", a(1, 2, want=("K", "p")))
case("feedback_gains[out]", lambda: ((), dict(knot0=1, nknots=2, out=dict(K=z(B, 2, m * n), P=Dev(B * 2 * n * n)))))
case("feedback_gains[unknown]", a(want=("K", "Z")))
case("feedback_gains[not positive definite]", codes=(api.ERR_NOT_SPD,))
case("objective")
case("objective[stage]", a(stage=True))
case("objective[out]", lambda: ((), dict(out=dict(J=Dev(B), stage=z(B, N)))))
case("objective[unknown]", lambda: ((), dict(out=dict(J=z(B), cost=z(B)))))
case("refine")
case("refine[max_steps]", a(5))
case("refine_adjoint")
case("kkt_residual_vector")
case("kkt_residual_vector[device]", lambda: ((Dev(B * NVARS),), {}))
case("kkt_residual_vector[bad size]", lambda: ((z(B, NVARS + 1),), {}))
case("refine_phase_ms")
# ---- box constraints
for label, four in (("(n,)", lambda: [z(n), z(n), z(m), z(m)]), ("(N, n)", lambda: [z(N, n), z(N, n), z(N, m), z(N, m)]),
                    ("(batch, N, n)", lambda: [z(B, N, n), z(B, N, n), z(B, N, m), z(B, N, m)]),
                    ("(n,) and (batch, N, m)", lambda: [z(n), None, z(B, N, m), None]), ("none", lambda: [None] * 4),
                    ("states", lambda: [z(n), z(N, n), None, None]), ("device", lambda: [Dev(B * N * n), None, None, Dev(B * N * m)]),
                    ("(n,) and device", lambda: [z(n), None, Dev(B * N * m), None]), ("lists", lambda: [[0.0] * n, None, None, [[1.0] * m] * N]),
                    ("bad shape", lambda: [z(n), z(n), z(n), z(m)]), ("bad device size", lambda: [Dev(N * n), None, None, None])):
    case("set_bounds[%s]" % label, lambda four=four: (four(), {}))
case("solve_box")
case("solve_box[settings]", a(0.5, 1.5, 1e-5, 1e-6, 50, 5, True, 4, 1e-3, 1e3))
case("set_box_infeasibility")
case("set_box_infeasibility[settings]", a(5, 1e-3))
case("infeasibility_certificate")
case("infeasibility_certificate[host, device]", lambda: ((z(B, N, n), Dev(B * N * n)), dict(dmu_u=z(B, N, m))))
case("infeasibility_certificate[bad size]", lambda: ((z(B, N, m),), {}))
case("set_box_acceleration")
case("set_box_acceleration[settings]", a(5, 2.0, 1e-8))
case("box_acceleration")
case("box_acceleration[mem 3]", setup=lambda bs: bs.set_box_acceleration(3))
case("box_penalties")
case("box_penalties[host]", lambda: ((z(B),), {}))
case("box_penalties[device]", lambda: ((Dev(B),), {}))
case("box_penalties[bad size]", lambda: ((z(B + 1),), {}))
for method in ("box_residuals", "box_adjoint_residuals", "constraint_adjoint_residuals"):
    case(method)
    case(method + "[host]", lambda: ((z(B, 4),), {}))
    case(method + "[device]", lambda: ((Dev(4 * B),), {}))
    case(method + "[float32]", lambda: ((z(B, 4, dtype=np.float32),), {}))
case("bound_multipliers")
case("bound_multipliers[host, device]", lambda: ((z(B, N, n), Dev(B * N * m)), {}))
case("solve_box_adjoint", lambda: ((z(B, NVARS),), {}))
case("solve_box_adjoint[device, settings]", lambda: ((Dev(B * NVARS), 1.5, 1e-5, 1e-6, 50, 5), {}))
case("solve_box_adjoint[bad size]", lambda: ((z(B, NVARS + 1),), {}))
case("bound_gradients")
case("bound_gradients[summed]", a(summed=True))
case("bound_gradients[out]", lambda: ((), dict(out=dict(xhi=z(B, N, n), ulo=Dev(B * N * m), uhi=None))))
case("bound_gradients[summed, out]", lambda: ((True, dict(uhi=z(N, m))), {}))
case("bound_gradients[unknown]", lambda: ((), dict(out=dict(xlo=z(B, N, n), lo=z(B, N, n)))))
case("bound_gradients[bad size]", lambda: ((), dict(out=dict(xlo=z(N, n)))))
case("polish_codes")

MODULE_CASES = [  # the calls made without a solver: (label, function of the api module)
    ("device_count", lambda: api.device_count()),
    ("feedback_gains_lds", lambda: api.feedback_gains_lds(n, m, True)),
    ("objective_constants", lambda: api.objective_constants()),
    ("generate_synthetic", lambda: api.generate_synthetic(n, m, N, 5)),
    ("DeviceArray.set", lambda: Dev(6).set(z(2, 3))),
    ("DeviceArray.get", lambda: shaped(Dev(6), (2, 3)).get()),
]


def shaped(d, shape):
    d.shape = shape
    return d


def outcome(stub, call, given=()):
    rec = {}
    try:
        rec["returns"] = describe(call(), given)
    except Exception as e:  # noqa: BLE001 (whatever the method raises is what the record is about)
        rec["raises"] = [type(e).__name__, str(e)]
    rec["calls"] = list(stub.calls)
    return rec


def run(label, method, factory, setup, code):
    Dev.count = 0
    bs = make(0)
    if setup is not None:
        setup(bs)
    bs.L.code, bs.L.calls = code, []
    args, kwargs = factory()
    given = {id(x) for x in flatten(list(args) + list(kwargs.values())) if isinstance(x, (np.ndarray, Dev))}
    attr = getattr(type(bs), method)
    call = (lambda: attr.fget(bs)) if isinstance(attr, property) else (lambda: attr(bs, *args, **kwargs))
    rec = outcome(bs.L, call, given)
    rec["state"] = dict(rows=bs._rows, sel=None if bs._sel is None else list(bs._sel), accel_mem=bs._accel_mem,
                        step_refs=[len(t) for t in bs._step_refs], h=bs.h)
    bs.h = None  # (nothing for the finaliser to free)
    return rec


def record():
    out = {}
    for label, method, factory, setup, codes in CASES:
        out[label] = {str(code): run(label, method, factory, setup, code) for code in codes}
    saved = api._LIB
    try:
        for label, fn in MODULE_CASES:
            out["api." + label] = {}
            for code in (0, 7):
                Dev.count = 0
                api._LIB = Stub(code)
                out["api." + label][str(code)] = outcome(api._LIB, fn)
    finally:
        api._LIB = saved
    return json.loads(json.dumps(out))  # (tuples -> lists, as the fixture holds them)


def dump(transcript):
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in transcript.items()) + "\n}\n"


def test_every_public_method_that_reaches_the_library_is_recorded():
    public = {k for k in dir(api.BatchSolver) if not k.startswith("_")}
    assert public - NO_LIBRARY == {method for _, method, _, _, _ in CASES}


def test_calls_returns_and_errors_match_the_recorded_transcript():
    want = json.load(open(GOLDEN))
    got = record()
    assert list(got) == list(want)
    differing = [k for k in got if k not in INT_DESTINATION_CASES and got[k] != want[k]]
    assert not differing, "\n".join("%s:\n  got  %s\n  want %s" % (k, json.dumps(got[k]), json.dumps(want[k])) for k in differing[:5])


def test_a_numpy_int_destination_of_the_wrong_kind_is_refused():
    """The intended difference from the transcript: polish_box, polish_constrained and solve_polished_adjoint used to
    hand a numpy destination of any dtype, size or layout to the C side."""
    want = json.load(open(GOLDEN))
    got = record()
    for k in INT_DESTINATION_CASES:
        for code in ("0", "7"):
            assert "returns" in want[k]["0"] and want[k][code]["calls"]  # (as recorded: the call went through)
            assert got[k][code]["raises"] == ["ValueError", INT_MESSAGE] and got[k][code]["calls"] == []
    g = z(B, NVARS)
    for bad in (z(B), z(B + 1, dtype=np.int32), z(B, 2, dtype=np.int32)[:, 0], [0] * B):
        for method, lead in (("polish_box", ()), ("polish_constrained", ()), ("solve_polished_adjoint", (g,))):
            for which in ("steps", "status"):
                bs = make(0)
                with pytest.raises(ValueError, match=INT_MESSAGE):
                    getattr(bs, method)(*lead, **{which: bad})
                assert bs.L.calls == []


def test_a_new_solver_has_no_constraint_rows_and_no_acceleration_memory():
    saved = api._LIB
    api._LIB = Stub(1)
    try:
        bs = api.BatchSolver(n, m, N, B)
    finally:
        api._LIB = saved
    assert bs._rows == 0 and bs._accel_mem == 0
    bs.L = Stub(0)
    assert bs.constraint_multipliers().shape == (B, N, 1) and bs.box_acceleration()[2].shape == (B, 0)  # (as when unset)
    with pytest.raises(RuntimeError, match="ndlqr_BatchSetConstraintBounds: initialize_flat_constrained first"):
        bs.set_constraint_bounds(z(1), z(1))


if __name__ == "__main__":
    sys.stdout.write(dump(record()))
