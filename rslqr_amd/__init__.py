"""rslqr_amd -- MI355X-native nested-dissection LQR solver behind the rsLQR `ndlqr_*` C API.

The product is the shared library ``librslqr_amd.so`` (plain-C host code + HIP kernels for
gfx950, see ``csrc/`` and ``include/ndlqr.h``). This Python package is only the host-side mirror
used by tests and the benchmark: ctypes bindings with the same names and argument meaning as the
C API, plus a numpy-friendly ``BatchSolver``; ``rslqr_amd.autograd`` puts the solve behind a
``torch.autograd.Function`` (adjoint solve and parameter gradients on the device).
"""
from .api import (  # noqa: F401
    BOUNDS_SHARED,
    BatchSolver,
    DeviceArray,
    FLAG_GENERIC,
    FLAG_KEEP_FACT,
    FLAG_KEEP_RECORDS,
    FLAG_PROFILE,
    FLAG_STRICT_FP,
    GRAD_A,
    GRAD_B,
    GRAD_NAMES,
    GRAD_Q,
    GRAD_R,
    GRAD_d,
    GRAD_q,
    GRAD_r,
    GRAD_x0,
    LQRData,
    LQRProblem,
    Matrix,
    NdData,
    NdFactor,
    NdLqrBoxSettings,
    NdLqrBoxSettingsFull,
    NdLqrSolver,
    SOLN_INPUT,
    SOLN_ONLY,
    SOLN_LAMBDA,
    SOLN_STATE,
    device_count,
    exported_symbols,
    generate_synthetic,
    lib,
    library_path,
    pinned_empty,
)
