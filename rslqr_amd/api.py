"""ctypes mirror of include/ndlqr.h and include/ndlqr_hip.h.

Function names, argument order and return conventions are those of the C API (and therefore of
the reference's src/*.h); nothing numerical happens in Python. If the shared library is missing
it is built in-tree with hipcc (rslqr_amd.build); if that fails the import fails loudly -- there
is no Python or CPU fallback for the solver.
"""
import ctypes as C
import os
import re

import numpy as np

from . import build as _build

FLAG_STRICT_FP = 1
FLAG_GENERIC = 2
FLAG_PROFILE = 4
FLAG_KEEP_FACT = 8
FLAG_KEEP_RECORDS = 16
SOLN_LAMBDA, SOLN_STATE, SOLN_INPUT, SOLN_ONLY = 1, 2, 4, 8
# ndlqr_BatchGradients: bit o of sum_mask sums output o over the batch; GRAD_NAMES in the order of the bits / arguments
GRAD_A, GRAD_B, GRAD_Q, GRAD_R, GRAD_q, GRAD_r, GRAD_d, GRAD_x0 = 1, 2, 4, 8, 16, 32, 64, 128
GRAD_NAMES = ("A", "B", "Q", "R", "q", "r", "d", "x0")
# ndlqr_BatchGradientsDense: the same for the nine outputs of dense-cost mode, in the order of the dense initialiser
GRADD_A, GRADD_B, GRADD_Q, GRADD_H, GRADD_R, GRADD_q, GRADD_r, GRADD_d, GRADD_x0 = 1, 2, 4, 8, 16, 32, 64, 128, 256
GRAD_DENSE_NAMES = ("A", "B", "Q", "H", "R", "q", "r", "d", "x0")

ERR_INVALID = -1
ERR_NO_DEVICE = -2
ERR_NOT_SPD = -3

dp = C.POINTER(C.c_double)


class Matrix(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("data", dp)]

    def numpy(self):
        """Copy out as a (rows, cols) array (storage is column-major)."""
        flat = np.ctypeslib.as_array(self.data, (self.rows * self.cols,))
        return flat.reshape(self.cols, self.rows).T.copy()


class CholeskyInfo(C.Structure):
    _fields_ = [("uplo", C.c_char), ("success", C.c_int), ("lib", C.c_char), ("fact", C.c_void_p),
                ("is_freed", C.c_int)]


class LQRData(C.Structure):
    _fields_ = [("nstates", C.c_int), ("ninputs", C.c_int), ("Q", dp), ("R", dp), ("q", dp),
                ("r", dp), ("c", dp), ("A", dp), ("B", dp), ("d", dp)]


class LQRProblem(C.Structure):
    _fields_ = [("nhorizon", C.c_int), ("x0", dp), ("lqrdata", C.POINTER(C.POINTER(LQRData)))]


class UnitRange(C.Structure):
    _fields_ = [("start", C.c_int), ("stop", C.c_int)]


class BinaryNode(C.Structure):
    pass


BinaryNode._fields_ = [("idx", C.c_int), ("level", C.c_int), ("levelidx", C.c_int),
                       ("left_inds", UnitRange), ("right_inds", UnitRange),
                       ("parent", C.POINTER(BinaryNode)), ("left_child", C.POINTER(BinaryNode)),
                       ("right_child", C.POINTER(BinaryNode))]


class OrderedBinaryTree(C.Structure):
    _fields_ = [("root", C.POINTER(BinaryNode)), ("node_list", C.POINTER(BinaryNode)),
                ("num_elements", C.c_int), ("depth", C.c_int)]


class NdFactor(C.Structure):
    _fields_ = [("lambda_", Matrix), ("state", Matrix), ("input", Matrix)]


class NdData(C.Structure):
    _fields_ = [("nstates", C.c_int), ("ninputs", C.c_int), ("nsegments", C.c_int),
                ("depth", C.c_int), ("width", C.c_int), ("data", dp),
                ("factors", C.POINTER(NdFactor))]

    def numpy(self):
        """View of the whole slab (no copy)."""
        count = (self.nsegments + 1) * self.depth * (2 * self.nstates + self.ninputs) * self.width
        return np.ctypeslib.as_array(self.data, (count,))


class NdLqrCholeskyFactors(C.Structure):
    _fields_ = [("depth", C.c_int), ("nhorizon", C.c_int), ("cholinfo", C.POINTER(CholeskyInfo)),
                ("numfacts", C.c_int)]


class NdLqrProfile(C.Structure):
    _fields_ = [("t_total_ms", C.c_double), ("t_leaves_ms", C.c_double),
                ("t_products_ms", C.c_double), ("t_cholesky_ms", C.c_double),
                ("t_cholsolve_ms", C.c_double), ("t_shur_ms", C.c_double),
                ("num_threads", C.c_int)]


class NdLqrSolver(C.Structure):
    _fields_ = [("nstates", C.c_int), ("ninputs", C.c_int), ("nhorizon", C.c_int),
                ("depth", C.c_int), ("nvars", C.c_int), ("tree", OrderedBinaryTree),
                ("diagonals", C.POINTER(Matrix)), ("data", C.POINTER(NdData)),
                ("fact", C.POINTER(NdData)), ("soln", C.POINTER(NdData)),
                ("cholfacts", C.POINTER(NdLqrCholeskyFactors)), ("solve_time_ms", C.c_double),
                ("linalg_time_ms", C.c_double), ("profile", NdLqrProfile),
                ("num_threads", C.c_int), ("device_ctx", C.c_void_p),
                ("device_flags", C.c_uint), ("device_profiling", C.c_int), ("device_profiled", C.c_int),
                ("device_split", NdLqrProfile), ("mirror_fact", C.c_int)]


class NdLqrBoxSettings(C.Structure):
    """The seven fixed-penalty fields of the C NdLqrBoxSettings, at the size that struct had before the adaptive-penalty
    fields were appended: kept for code that builds or inspects it. The library calls take NdLqrBoxSettingsFull (ctypes
    refuses a pointer to this shorter struct: the C side reads all ten fields)."""
    _fields_ = [("rho", C.c_double), ("alpha", C.c_double), ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("max_iter", C.c_int), ("check_every", C.c_int), ("warm_start", C.c_int)]


class NdLqrBoxSettingsFull(C.Structure):
    """NdLqrBoxSettings of include/ndlqr.h as it is now: the seven fields above, then adapt_every, rho_min, rho_max
    (positional construction with the first seven leaves those zero: the fixed penalty)."""
    _fields_ = NdLqrBoxSettings._fields_ + [("adapt_every", C.c_int), ("rho_min", C.c_double), ("rho_max", C.c_double)]


BOUNDS_SHARED = 1

_LIB = None


class NdLqrPolishSettings(C.Structure):
    """NdLqrPolishSettings of include/ndlqr.h"""
    _fields_ = [("sigma", C.c_double), ("max_steps", C.c_int), ("max_rounds", C.c_int)]


def library_path():
    return _build.LIB


def exported_symbols():
    """Every function name declared in include/ndlqr.h and include/ndlqr_hip.h."""
    names = []
    for hdr in ("ndlqr.h", "ndlqr_hip.h"):
        text = open(os.path.join(_build.INCLUDE, hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"static inline[^{]*\{[^}]*\}", "", text)
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text):
            names.append(m.group(1))
    return sorted(set(names))


def lib():
    """Load (building if needed) librslqr_amd.so and declare the prototypes used from Python."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_build.LIB):
        _build.build()
    # NDLQR_LIBRARY: developer hook for instrumented builds of the same library (tools/segtime.py)
    L = C.CDLL(os.environ.get("NDLQR_LIBRARY", _build.LIB))
    vp, ci, cd, cu64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    sp = C.POINTER(NdLqrSolver)
    pp = C.POINTER(LQRProblem)
    ndp = C.POINTER(NdData)
    mp = C.POINTER(Matrix)

    def proto(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    proto("ndlqr_Version", C.c_char_p)
    proto("ndlqr_hip_device_count", ci)
    proto("ndlqr_hip_last_error", C.c_char_p)
    # problem containers
    proto("ndlqr_NewLQRData", C.POINTER(LQRData), ci, ci)
    proto("ndlqr_FreeLQRData", ci, C.POINTER(LQRData))
    proto("ndlqr_InitializeLQRData", ci, C.POINTER(LQRData), dp, dp, dp, dp, cd, dp, dp, dp)
    proto("ndlqr_CopyLQRData", ci, C.POINTER(LQRData), C.POINTER(LQRData))
    proto("ndlqr_NewLQRProblem", pp, ci, ci, ci)
    proto("ndlqr_InitializeLQRProblem", ci, pp, dp, C.POINTER(C.POINTER(LQRData)))
    proto("ndlqr_FreeLQRProblem", ci, pp)
    proto("ndlqr_ReadLQRProblemJSONFile", pp, C.c_char_p)
    proto("ndlqr_ReadLQRDataJSONFile", C.POINTER(LQRData), C.c_char_p)
    proto("ReadMatrixJSONFile", Matrix, C.c_char_p, C.c_char_p)
    proto("FreeMatrix", ci, mp)
    proto("ReadFile", ci, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(ci))
    proto("ndlqr_NewSyntheticLQRProblem", pp, ci, ci, ci, cu64)
    proto("ndlqr_GenerateSyntheticFlat", ci, ci, ci, ci, cu64, dp, dp, dp, dp, dp, dp, dp, dp)
    # tree / storage
    proto("ndlqr_BuildTree", OrderedBinaryTree, ci)
    proto("ndlqr_FreeTree", ci, C.POINTER(OrderedBinaryTree))
    proto("ndlqr_GetIndexFromLeaf", ci, C.POINTER(OrderedBinaryTree), ci, ci)
    proto("ndlqr_GetIndexLevel", ci, C.POINTER(OrderedBinaryTree), ci)
    proto("ndlqr_GetIndexAtLevel", ci, C.POINTER(OrderedBinaryTree), ci, ci)
    proto("ndlqr_NewNdData", ndp, ci, ci, ci, ci)
    proto("ndlqr_FreeNdData", ci, ndp)
    proto("ndlqr_ResetNdData", None, ndp)
    proto("ndlqr_GetNdFactor", ci, ndp, ci, ci, C.POINTER(C.POINTER(NdFactor)))
    proto("ndlqr_NewCholeskyFactors", C.POINTER(NdLqrCholeskyFactors), ci, ci)
    proto("ndlqr_FreeCholeskyFactors", ci, C.POINTER(NdLqrCholeskyFactors))
    proto("ndlqr_GetSFactorization", ci, C.POINTER(NdLqrCholeskyFactors), ci, ci,
          C.POINTER(C.POINTER(CholeskyInfo)))
    # solver
    proto("ndlqr_NewNdLqrSolver", sp, ci, ci, ci)
    proto("ndlqr_FreeNdLqrSolver", ci, sp)
    proto("ndlqr_InitializeWithLQRProblem", ci, pp, sp)
    proto("ndlqr_ResetSolver", None, sp)
    proto("ndlqr_GetNumVars", ci, sp)
    proto("ndlqr_SetNumThreads", ci, sp, ci)
    proto("ndlqr_GetNumThreads", ci, sp)
    proto("ndlqr_PrintSolveSummary", None, sp)
    proto("ndlqr_PrintSolveProfile", ci, sp)
    proto("ndlqr_GetProfile", NdLqrProfile, sp)
    proto("ndlqr_Solve", ci, sp)
    proto("ndlqr_GetSolution", Matrix, sp)
    proto("ndlqr_CopySolution", ci, sp, dp)
    proto("ndlqr_SyncFactorsToHost", ci, sp)
    proto("ndlqr_SetDeviceProfiling", ci, sp, ci)
    proto("ndlqr_SetDeviceFlags", ci, sp, C.c_uint)
    proto("ndlqr_SetFactorMirroring", ci, sp, ci)
    # stage functions
    proto("ndlqr_SolveLeaf", ci, sp, ci)
    proto("ndlqr_SolveLeaves", ci, sp)
    proto("ndlqr_FactorInnerProduct", ci, ndp, ndp, ci, ci, ci)
    proto("ndlqr_SolveCholeskyFactor", ci, ndp, C.POINTER(CholeskyInfo), ci, ci, ci)
    proto("ndlqr_UpdateShurFactor", ci, ndp, ndp, ci, ci, ci, ci, C.c_bool)
    proto("ndlqr_ShouldCalcLambda", C.c_bool, C.POINTER(OrderedBinaryTree), ci, ci)
    proto("ndlqr_ComputeShurCompliment", ci, sp, ci, ci, ci)
    # dense helpers
    proto("MatrixMultiply", None, mp, mp, mp, C.c_bool, C.c_bool, cd, cd)
    proto("MatrixCholeskyFactorize", ci, mp)
    proto("MatrixCholeskySolve", ci, mp, mp)
    proto("MatrixSymmetricMultiply", None, mp, mp, mp, cd, cd)
    proto("MatrixAddition", ci, mp, mp, cd)
    proto("MatrixCholeskyFactorizeWithInfo", ci, mp, C.POINTER(CholeskyInfo))
    proto("MatrixCholeskySolveWithInfo", ci, mp, mp, C.POINTER(CholeskyInfo))
    proto("MatrixCopyDiagonal", None, mp, mp)
    proto("clap_MatrixAddition", ci, mp, mp, cd)
    proto("clap_MatrixScale", ci, mp, cd)
    proto("clap_MatrixMultiply", ci, mp, mp, mp, C.c_bool, C.c_bool, cd, cd)
    proto("clap_MatrixTransposeMultiply", ci, mp, mp, mp)
    proto("clap_SymmetricMatrixMultiply", ci, mp, mp, mp, cd, cd)
    proto("clap_AddDiagonal", ci, mp, cd)
    proto("clap_CholeskyFactorize", ci, mp)
    proto("clap_CholeskySolve", ci, mp, mp)
    proto("clap_LowerTriBackSub", ci, mp, mp, C.c_bool)
    # batch
    proto("ndlqr_NewBatchSolver", vp, ci, ci, ci, ci, ci)
    proto("ndlqr_FreeBatchSolver", ci, vp)
    proto("ndlqr_BatchSetFlags", ci, vp, C.c_uint)
    proto("ndlqr_BatchGetFlags", C.c_uint, vp)
    proto("ndlqr_InitializeBatch", ci, vp, C.POINTER(pp), ci)
    proto("ndlqr_InitializeBatchFlat", ci, vp, dp, dp, dp, dp, dp, dp, dp, dp)
    proto("ndlqr_InitializeBatchSynthetic", ci, vp, cu64)
    proto("ndlqr_InitializeBatchFlatDense", ci, vp, dp, dp, dp, dp, dp, dp, dp, dp, dp)
    proto("ndlqr_BatchCostIsDense", ci, vp)
    proto("ndlqr_hip_download_cost_reduction", ci, vp, dp, dp, dp, dp, dp, dp, dp, dp, dp)
    proto("ndlqr_hip_cost_phase_ms", ci, vp, dp)
    proto("ndlqr_InitializeBatchFlatConstrained", ci, vp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ci, dp, dp, dp, dp, C.c_uint)
    proto("ndlqr_BatchIsConstrained", ci, vp)
    proto("ndlqr_BatchSetConstraintBounds", ci, vp, dp, dp, C.c_uint)
    proto("ndlqr_SolveBatchLinConstrained", ci, vp, C.POINTER(NdLqrBoxSettingsFull), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_BatchSetConstraintPenaltyAdaptation", ci, vp, ci, C.c_double, C.c_double)
    proto("ndlqr_CopyBatchConstraintPenalties", ci, vp, dp)
    proto("ndlqr_BatchSetConstraintInfeasibilityDetection", ci, vp, ci, cd)
    proto("ndlqr_CopyBatchConstraintInfeasibilityCertificate", ci, vp, dp, dp)
    proto("ndlqr_CopyBatchConstraintInfeasibilityMeasures", ci, vp, dp, C.POINTER(ci))
    proto("ndlqr_CopyBatchConstraintMultipliers", ci, vp, dp)
    proto("ndlqr_CopyBatchConstraintResiduals", ci, vp, dp)
    proto("ndlqr_hip_download_constraint_reduction", ci, vp, *([dp] * 14))
    proto("ndlqr_SolveBatchLinAdjoint", ci, vp, dp, C.POINTER(NdLqrBoxSettingsFull), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_BatchConstraintGradients", ci, vp, dp, dp, dp, dp, C.c_uint)
    proto("ndlqr_CopyBatchConstraintAdjointMultipliers", ci, vp, dp)
    proto("ndlqr_CopyBatchConstraintAdjointResiduals", ci, vp, dp)
    proto("ndlqr_CopyBatchConstraintCodes", ci, vp, C.c_void_p)
    proto("ndlqr_hip_download_constraint_codes", ci, vp, C.c_void_p, dp)
    proto("ndlqr_InitializeBatchFlatDevice", ci, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    proto("ndlqr_SolveBatch", ci, vp)
    proto("ndlqr_BatchSetRhsFlat", ci, vp, dp, dp, dp, dp)
    proto("ndlqr_SolveBatchRhsOnly", ci, vp)
    proto("ndlqr_SolveBatchMultiRhs", ci, vp, ci, dp, dp, dp, dp, dp)
    proto("ndlqr_SolveBatchMultiRhsSlices", ci, vp, ci, dp, dp, dp, dp, ci, ci, C.c_uint, dp)
    proto("ndlqr_SolveBatchAsync", ci, vp)
    proto("ndlqr_BatchStepAsync", ci, vp, dp, dp, dp, dp, dp)
    proto("ndlqr_BatchSynchronizePrevious", ci, vp)
    proto("ndlqr_BatchSetStepSelection", ci, vp, ci, ci, C.c_uint)
    proto("ndlqr_CopyBatchSolutionSlices", ci, vp, ci, ci, C.c_uint, dp)
    proto("ndlqr_SolveBatchSlicesAsync", ci, vp, ci, ci, C.c_uint, dp)
    proto("ndlqr_BatchStepAsyncDense", ci, vp, dp, dp, dp, dp, ci, ci, C.c_uint, dp)
    proto("ndlqr_SolveBatchSlicesAsyncDense", ci, vp, ci, ci, C.c_uint, dp)
    proto("ndlqr_CopyBatchSolutionSlicesDense", ci, vp, ci, ci, C.c_uint, dp)
    proto("ndlqr_hip_download_rhs_raw", ci, vp, dp)
    proto("ndlqr_hip_rhs_raw_doubles", C.c_size_t, vp)
    proto("ndlqr_BatchTimeShardTopDoubles", ci, vp, ci)
    proto("ndlqr_BatchTimeShardFactor", ci, vp, ci, ci)
    proto("ndlqr_BatchTimeShardExportTop", ci, vp, ci, vp)
    proto("ndlqr_BatchTimeShardImportTop", ci, vp, ci, vp)
    proto("ndlqr_BatchTimeShardFinish", ci, vp, ci, ci)
    proto("ndlqr_HostAlloc", vp, C.c_size_t)
    proto("ndlqr_HostFree", None, vp)
    proto("ndlqr_DeviceAlloc", vp, C.c_size_t)
    proto("ndlqr_DeviceFree", None, vp)
    proto("ndlqr_DeviceCopy", ci, vp, vp, C.c_size_t)
    proto("ndlqr_BatchSynchronize", ci, vp)
    proto("ndlqr_BatchNumVars", ci, vp)
    proto("ndlqr_BatchSize", ci, vp)
    proto("ndlqr_CopyBatchSolution", ci, vp, ci, dp)
    proto("ndlqr_CopyBatchSolutions", ci, vp, dp)
    proto("ndlqr_CopyBatchSolutionsDevice", ci, vp, vp)
    proto("ndlqr_CopyBatchFactors", ci, vp, ci, dp)
    proto("ndlqr_BatchCholeskyFailures", ci, vp)
    proto("ndlqr_CopyBatchCholeskyFailureCounts", ci, vp, C.POINTER(ci))
    proto("ndlqr_BatchKktResiduals", ci, vp, dp, dp)
    proto("ndlqr_BatchSolveTimeMs", cd, vp)
    proto("ndlqr_SolveBatchAdjoint", ci, vp, dp)
    proto("ndlqr_CopyBatchAdjoint", ci, vp, dp)
    proto("ndlqr_BatchGradients", ci, vp, C.c_uint, dp, dp, dp, dp, dp, dp, dp, dp)
    proto("ndlqr_BatchGradientsDense", ci, vp, C.c_uint, dp, dp, dp, dp, dp, dp, dp, dp, dp)
    proto("ndlqr_hip_gradients_dense_constants", ci, C.POINTER(C.c_int))
    proto("ndlqr_BatchFeedbackGains", ci, vp, ci, ci, dp, dp, dp, dp, C.POINTER(ci))
    proto("ndlqr_hip_feedback_gains_lds", C.c_size_t, ci, ci, ci)
    proto("ndlqr_BatchObjective", ci, vp, dp, dp)
    proto("ndlqr_hip_objective_constants", ci, C.POINTER(C.c_int))
    proto("ndlqr_RefineBatch", ci, vp, ci, C.POINTER(ci), dp, dp)
    proto("ndlqr_RefineBatchAdjoint", ci, vp, ci, C.POINTER(ci), dp, dp)
    proto("ndlqr_BatchKktResidualVector", ci, vp, dp)
    proto("ndlqr_hip_refine_phase_ms", ci, vp, dp)
    proto("ndlqr_BatchDeviceContext", vp, vp)
    proto("ndlqr_BatchSetBounds", ci, vp, C.c_uint, dp, dp, dp, dp)
    proto("ndlqr_SolveBatchBoxConstrained", ci, vp, C.POINTER(NdLqrBoxSettingsFull), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_CopyBatchBoundMultipliers", ci, vp, dp, dp)
    proto("ndlqr_CopyBatchBoxPenalties", ci, vp, dp)
    proto("ndlqr_CopyBatchBoxResiduals", ci, vp, dp)
    proto("ndlqr_CopyBatchBoxAdjointResiduals", ci, vp, dp)
    proto("ndlqr_BatchSetInfeasibilityDetection", ci, vp, ci, cd)
    proto("ndlqr_CopyBatchInfeasibilityCertificate", ci, vp, dp, dp, dp)
    proto("ndlqr_CopyBatchInfeasibilityMeasures", ci, vp, dp, C.POINTER(ci))
    proto("ndlqr_BatchSetBoxAcceleration", ci, vp, ci, cd, cd)
    proto("ndlqr_CopyBatchBoxAcceleration", ci, vp, C.POINTER(ci), C.POINTER(ci), dp, C.POINTER(ci))
    proto("ndlqr_SolveBatchBoxAdjoint", ci, vp, dp, C.POINTER(NdLqrBoxSettingsFull), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_BatchBoundGradients", ci, vp, C.c_uint, dp, dp, dp, dp)
    proto("ndlqr_PolishBatchBoxConstrained", ci, vp, C.POINTER(NdLqrPolishSettings), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_hip_download_polish_codes", ci, vp, C.POINTER(C.c_ubyte))
    proto("ndlqr_SolveBatchPolishedAdjoint", ci, vp, dp, C.POINTER(NdLqrPolishSettings), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_PolishBatchLinConstrained", ci, vp, C.POINTER(NdLqrPolishSettings), C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_CopyBatchConstraintPolishCodes", ci, vp, vp)
    proto("ndlqr_hip_polish_constrained", ci, vp, cd, ci, ci, C.POINTER(ci), C.POINTER(ci))
    proto("ndlqr_hip_constraint_polish_residual", ci, vp, dp, dp, C.POINTER(C.c_ubyte), dp, ci, dp, dp, dp)
    proto("ndlqr_hip_constraint_polish_phase_ms", ci, vp, dp, C.POINTER(ci))
    proto("ndlqr_hip_download_constraint_polish_state", ci, vp, dp, dp, dp, dp, C.POINTER(ci))
    proto("ndlqr_hip_factor_count", C.c_ulonglong, vp)
    # shim bits used by the benchmark
    proto("ndlqr_hip_set_stream", ci, vp, vp)
    proto("ndlqr_hip_get_stream", vp, vp)
    proto("ndlqr_hip_profile_slots", ci, vp)
    proto("ndlqr_hip_profile_get", ci, vp, ci, C.c_char_p, ci, dp, C.POINTER(ci))
    proto("ndlqr_hip_profile_reset", ci, vp)
    proto("ndlqr_hip_device_pointers", ci, vp, C.POINTER(vp))
    proto("ndlqr_hip_staged_io", ci, vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp))
    proto("ndlqr_hip_download_rhs_blocks", ci, vp, ci, dp)
    proto("ndlqr_hip_upload_inputs", ci, vp, ci, ci, dp, dp, dp)
    proto("ndlqr_hip_factors_valid", ci, vp)
    proto("ndlqr_hip_schedule", C.c_char_p, vp)
    if hasattr(L, "ndlqr_hip_compact_level1"):  # (an older build loaded through NDLQR_LIBRARY for an A/B has none)
        proto("ndlqr_hip_compact_level1", C.c_int, vp)
    if hasattr(L, "ndlqr_hip_level1_paired"):
        proto("ndlqr_hip_level1_paired", C.c_int, vp)
    if hasattr(L, "ndlqr_hip_bottom_lds16"):
        proto("ndlqr_hip_bottom_lds16", C.c_int, vp)
    if hasattr(L, "ndlqr_hip_top_chain"):
        proto("ndlqr_hip_top_chain", C.c_int, vp)
    proto("ndlqr_hip_set_pipeline_depth", ci, vp, ci)
    proto("ndlqr_hip_pipeline_depth", ci, vp)
    proto("ndlqr_hip_pack_solutions_device", ci, vp, vp)
    proto("ndlqr_hip_gemm", ci, ci, ci, ci, ci, ci, cd, dp, ci, dp, ci, cd, dp, ci)
    proto("ndlqr_hip_potrf_lower", ci, ci, dp, ci)
    proto("ndlqr_hip_potrs_lower", ci, ci, ci, dp, ci, dp, ci)
    proto("ndlqr_hip_trsv_lower", ci, ci, ci, dp, ci, dp, ci, ci)
    _LIB = L
    return L


def pinned_empty(shape):
    """float64 numpy array in pinned host memory (ndlqr_HostAlloc): H2D / D2H copies from / to it are
    asynchronous and run at the rate of the host link. Freed when the array is garbage-collected."""
    import weakref
    count = int(np.prod(shape))
    L = lib()
    ptr = L.ndlqr_HostAlloc(max(count, 1) * 8)
    if not ptr:
        raise MemoryError("ndlqr_HostAlloc(%d bytes) failed" % (count * 8))
    buf = (C.c_double * max(count, 1)).from_address(ptr)
    arr = np.ctypeslib.as_array(buf)[:count].reshape(shape)
    weakref.finalize(buf, L.ndlqr_HostFree, C.c_void_p(ptr))
    return arr


class DeviceArray:
    """float64 values of `shape` in device memory (ndlqr_DeviceAlloc): what BatchSolver.step_async takes for q, r, d, x0
    and soln when the loop around the solver lives on the GPU -- nothing crosses the host link then. set() / get() copy
    from / to numpy arrays synchronously (ndlqr_DeviceCopy); `ptr` is the raw address for other device code."""

    def __init__(self, shape):
        import weakref
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.size = int(np.prod(self.shape))
        L = lib()
        self.ptr = L.ndlqr_DeviceAlloc(max(self.size, 1) * 8)
        if not self.ptr:
            raise MemoryError("ndlqr_DeviceAlloc(%d bytes) failed" % (self.size * 8))
        weakref.finalize(self, L.ndlqr_DeviceFree, C.c_void_p(self.ptr))

    def set(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        assert arr.size == self.size
        if lib().ndlqr_DeviceCopy(C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), self.size * 8):
            raise RuntimeError("ndlqr_DeviceCopy failed")
        return self

    def get(self):
        out = np.empty(self.shape)
        if lib().ndlqr_DeviceCopy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), self.size * 8):
            raise RuntimeError("ndlqr_DeviceCopy failed")
        return out


def _call(L, name, *args, detail=True, ok=(0,)):
    """L.name(*args), checked: RuntimeError "name failed: code (the library's last error)" -- without the parenthesis for
    detail=False, the text of the early calls -- unless the return code is one of `ok`. Returns the code."""
    err = getattr(L, name)(*args)
    if err not in ok:
        raise RuntimeError("%s failed: %d (%s)" % (name, err, L.ndlqr_hip_last_error().decode()) if detail
                           else "%s failed: %d" % (name, err))
    return err


def device_count():
    return lib().ndlqr_hip_device_count()


def feedback_gains_lds(n, m, second=False):
    """Bytes of LDS the sweep of BatchSolver.feedback_gains needs at block size (n, m), with the second input buffer or
    without it (ndlqr_hip_feedback_gains_lds); a shape that needs more than 160 KB without it is refused."""
    return int(lib().ndlqr_hip_feedback_gains_lds(n, m, 1 if second else 0))


def objective_constants():
    """(knots of a workgroup's chunk, workgroup size) of the kernels behind BatchSolver.objective
    (ndlqr_hip_objective_constants): the tests size a horizon by them."""
    out = (C.c_int * 2)()
    if lib().ndlqr_hip_objective_constants(out):
        raise RuntimeError("ndlqr_hip_objective_constants failed")
    return int(out[0]), int(out[1])


def _ptr(a):
    return a.ctypes.data_as(dp)


def _any_ptr(a, size):
    """double* of a numpy array (float64, C-contiguous) or of device memory -- anything with `ptr` and `size` attributes,
    such as a DeviceArray -- holding `size` doubles."""
    if hasattr(a, "ptr"):
        if a.size != size:
            raise ValueError("expected %d doubles, got %d" % (size, a.size))
        return C.cast(C.c_void_p(int(a.ptr)), dp)
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.size == size):
        raise ValueError("expected a C-contiguous float64 array of %d doubles" % size)
    return _ptr(a)


def _doubles(a):
    """`a` itself if it is device memory (has `ptr`), else as a C-contiguous float64 numpy array."""
    return a if hasattr(a, "ptr") else np.ascontiguousarray(a, dtype=np.float64)


def _int_ptr(a, size):
    """int* of a numpy array (int32, C-contiguous) or of device memory -- anything with `ptr` -- holding `size` ints."""
    if hasattr(a, "ptr"):
        return C.cast(C.c_void_p(int(a.ptr)), C.POINTER(C.c_int))
    if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.size == size):
        raise ValueError("expected a C-contiguous int32 array of %d entries" % size)
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _stage(names, arrays, sizes, optional=("H",)):
    """(pointers, keep-alive list) of the caller's arrays for an initialiser: a numpy array (anything ascontiguousarray
    takes) of sizes[name] doubles, device memory (`ptr`, `size`), or None for the names in `optional`."""
    ptrs, keep = [], []
    for name, a in zip(names, arrays):
        if a is None:
            if name not in optional:
                raise ValueError("%s is missing (only %s may be None)" % (name, " and ".join(optional)))
            ptrs.append(None)
            continue
        if not hasattr(a, "ptr"):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != sizes[name]:
                raise ValueError("bad size for %s" % name)
            keep.append(a)
        ptrs.append(_any_ptr(a, sizes[name]))
    return ptrs, keep


def _stage_bounds(bounds, N, B):
    """(pointers, shared, keep-alive list) for the (bound, width, may be None) of `bounds`: a numpy bound of shape
    (width,), (N, width) -- shared -- or (B, N, width), or device memory of B * N * width doubles. The bounds are shared
    only if every given one is a host array with ndim <= 2."""
    host = [a if (a is None and may_be_none) or hasattr(a, "ptr") else np.asarray(a, dtype=np.float64)
            for a, _, may_be_none in bounds]
    shared = all(a is None or (not hasattr(a, "ptr") and a.ndim <= 2) for a in host)
    ptrs, keep = [], []
    for a, (_, k, _) in zip(host, bounds):
        if a is None:
            ptrs.append(None)
            continue
        if not hasattr(a, "ptr"):
            if a.shape not in ((k,), (N, k), (B, N, k)):
                raise ValueError("bounds of shape %s: expected (%d,), (%d, %d) or (%d, %d, %d)" % (a.shape, k, N, k, B, N, k))
            a = np.ascontiguousarray(np.broadcast_to(a, (N, k) if shared else (B, N, k)))
            keep.append(a)
        ptrs.append(_any_ptr(a, (1 if shared else B) * N * k))
    return ptrs, shared, keep


def generate_synthetic(n, m, N, seed):
    """ndlqr_GenerateSyntheticFlat -> dict of numpy arrays (A [N,n*n] col-major, ...)."""
    out = dict(A=np.zeros((N, n * n)), B=np.zeros((N, n * m)), Q=np.zeros((N, n)),
               R=np.zeros((N, m)), q=np.zeros((N, n)), r=np.zeros((N, m)), d=np.zeros((N, n)),
               x0=np.zeros(n))
    _call(lib(), "ndlqr_GenerateSyntheticFlat", n, m, N, seed, *[_ptr(a) for a in out.values()], detail=False)
    return out


def top_chain(solver):
    """True when the last solve of the BatchSolver `solver` eliminated the separators of its top tree levels as one
    block-tridiagonal chain per problem (ndlqr_hip_top_chain; NDLQR_TOP_CHAIN). The schedule name is the same either way."""
    return hasattr(solver.L, "ndlqr_hip_top_chain") and bool(solver.L.ndlqr_hip_top_chain(solver.ctx))


class BatchSolver:
    """numpy-friendly wrapper of NdLqrBatchSolver (include/ndlqr.h, batch API)."""

    def __init__(self, n, m, N, batch, device=-1, flags=0):
        self.L = lib()
        self.n, self.m, self.N, self.batch = n, m, N, batch
        self.h = self.L.ndlqr_NewBatchSolver(n, m, N, batch, device)
        if not self.h:
            raise RuntimeError("ndlqr_NewBatchSolver failed: %s" %
                               self.L.ndlqr_hip_last_error().decode())
        self.nvars = self.L.ndlqr_BatchNumVars(self.h)
        self._sel = None          # (knot0, nknots, blocks) of set_step_selection
        self._step_refs = []      # host arrays of the steps in flight (kept alive until they are synchronised)
        self._rows = 0            # constraint rows per knot of initialize_flat_constrained
        self._accel_mem = 0       # memory of set_box_acceleration
        if flags:
            self.set_flags(flags)

    def close(self):
        if getattr(self, "h", None):
            self.L.ndlqr_FreeBatchSolver(self.h)  # (waits for everything in flight)
            self.h = None
        self._step_refs = []

    __del__ = close

    def set_flags(self, flags):
        self.L.ndlqr_BatchSetFlags(self.h, flags)

    @property
    def ctx(self):
        return self.L.ndlqr_BatchDeviceContext(self.h)

    # ---- what the methods below share: the checked call, and one helper per family of calls that differ in the C symbol
    def _call(self, name, *args, **how):
        """_call on the solver's library: every method that raises on a refusal goes through here."""
        return _call(self.L, name, *args, **how)

    def _copy_out(self, name, shape, dtype=np.float64, dest=None, via_ctx=False):
        """The read-outs of one array: `name`(handle, or device context for via_ctx, destination). The destination is
        `dest` (float64: a numpy array or DeviceArray of prod(shape) doubles), or a new numpy array. Returns it."""
        if dest is None:
            dest = np.zeros(shape, dtype=dtype)
        ptr = _any_ptr(dest, int(np.prod(shape))) if dtype is np.float64 else dest.ctypes.data_as(C.POINTER(C.c_ubyte))
        self._call(name, self.ctx if via_ctx else self.h, ptr)
        return dest

    def _admm_solve(self, name, settings, g=None):
        """The ADMM solves: `name`(handle, [g,] settings, iters, status) with g [batch, nvars] for an adjoint. Returns
        (iters, status), int32 [batch]."""
        st = NdLqrBoxSettingsFull(*settings)
        iters = np.zeros(self.batch, dtype=np.int32)
        status = np.zeros(self.batch, dtype=np.int32)
        lead = () if g is None else (_any_ptr(g, self.batch * self.nvars),)
        self._call(name, self.h, *lead, C.byref(st), _int_ptr(iters, self.batch), _int_ptr(status, self.batch))
        return iters, status

    def _polish(self, name, settings, steps, status, g=None):
        """The polish calls: `name`(handle, [g,] settings, steps, status); steps, status: int32 destinations [batch] (numpy
        arrays or device memory with `ptr`), None: new numpy arrays. Returns (steps, status)."""
        st = NdLqrPolishSettings(*settings)
        if steps is None:
            steps = np.zeros(self.batch, dtype=np.int32)
        if status is None:
            status = np.zeros(self.batch, dtype=np.int32)
        lead = () if g is None else (_any_ptr(g, self.batch * self.nvars),)
        self._call(name, self.h, *lead, C.byref(st), _int_ptr(steps, self.batch), _int_ptr(status, self.batch))
        return steps, status

    def _measures(self, name, measures, iteration):
        """The infeasibility measures: `name`(handle, measures [batch, 4], iteration [batch] of int32)."""
        if measures is None:
            measures = np.zeros((self.batch, 4))
        if iteration is None:
            iteration = np.zeros(self.batch, dtype=np.int32)
        ip = _int_ptr(iteration, self.batch)
        self._call(name, self.h, _any_ptr(measures, 4 * self.batch), ip)
        return measures, iteration

    def _named_gradients(self, name, shapes, out, flag, flag_first, what):
        """The gradient read-outs: `name`(handle, [flag,] one pointer per key of `shapes` in its order, [flag]); out: dict
        of destinations under those keys (numpy arrays or DeviceArrays; a key left out is not computed), None: new numpy
        arrays for all of them. `what` names the keys in the message about unknown ones. Returns out."""
        if out is None:
            out = {k: np.zeros(sh) for k, sh in shapes.items()}
        unknown = set(out) - set(shapes)
        if unknown:
            raise ValueError("unknown %s names: %s" % (what, sorted(unknown)))
        ptrs = [None if out.get(k) is None else _any_ptr(out[k], int(np.prod(sh))) for k, sh in shapes.items()]
        self._call(name, self.h, *([flag] + ptrs if flag_first else ptrs + [flag]))
        return out

    def initialize_flat(self, A, B, Q, R, q, r, d, x0):
        n, m, N, bt = self.n, self.m, self.N, self.batch
        shapes = dict(A=(bt, N, n * n), B=(bt, N, n * m), Q=(bt, N, n), R=(bt, N, m),
                      q=(bt, N, n), r=(bt, N, m), d=(bt, N, n), x0=(bt, n))
        arrs = []
        for name, a in zip(("A", "B", "Q", "R", "q", "r", "d", "x0"), (A, B, Q, R, q, r, d, x0)):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != int(np.prod(shapes[name])):
                raise ValueError("bad size for %s" % name)
            arrs.append(a)
        self._call("ndlqr_InitializeBatchFlat", self.h, *[_ptr(a) for a in arrs], detail=False)

    def initialize_flat_device(self, *device_ptrs):
        """Eight device pointers (ints), flat reference layout: A, B, Q, R, q, r, d, x0."""
        self._call("ndlqr_InitializeBatchFlatDevice", self.h, *[C.c_void_p(int(p)) for p in device_ptrs], detail=False)

    def initialize_flat_dense(self, A, B, Q, H, R, q, r, d, x0):
        """ndlqr_InitializeBatchFlatDense: dense cost matrices Q [batch, N, n*n], R [batch, N, m*m] and the state-input
        cross term H [batch, N, n*m] (None: no cross term), column-major per knot like A and B; only the lower triangles of
        Q and R are read. The other arrays as for initialize_flat. Each array is a numpy array or device memory (anything
        with `ptr` and `size`, such as a DeviceArray). The solver is in dense-cost mode afterwards (cost_is_dense()): solve,
        solutions, set_rhs_flat + solve_rhs_only, solve_adjoint + adjoint work in the caller's variables; what has no
        dense-cost form refuses (include/ndlqr.h has the list)."""
        n, m, N, bt = self.n, self.m, self.N, self.batch
        sizes = dict(A=bt * N * n * n, B=bt * N * n * m, Q=bt * N * n * n, H=bt * N * n * m, R=bt * N * m * m,
                     q=bt * N * n, r=bt * N * m, d=bt * N * n, x0=bt * n)
        ptrs, keep = _stage(GRAD_DENSE_NAMES, (A, B, Q, H, R, q, r, d, x0), sizes)
        self._call("ndlqr_InitializeBatchFlatDense", self.h, *ptrs)

    def cost_is_dense(self):
        """ndlqr_BatchCostIsDense: True between initialize_flat_dense and the next diagonal initialiser."""
        return bool(self.L.ndlqr_BatchCostIsDense(self.h))

    def cost_phase_ms(self):
        """(factor + transform, S', S): device times in ms of the latest launches of the reduction's kernels under FLAG_PROFILE."""
        out = np.zeros(3)
        self.L.ndlqr_hip_cost_phase_ms(self.ctx, _ptr(out))
        return tuple(out)

    def cost_reduction(self):
        """ndlqr_hip_download_cost_reduction (read-out for the tests): dict of numpy arrays -- the records L [batch, N, n*n],
        LR [batch, N, m*m], G [batch, N, m*n] (column-major per knot) and the reduced unit-cost problem At, Bt, qt, rt, dt,
        x0t in the flat layout of initialize_flat. Raises outside dense-cost mode. qt, rt, dt, x0t are those of the latest
        initialize_flat_dense / set_rhs_flat: the steps of step_dense_async reduce straight into the device right-hand side
        (rhs_raw() shows it) and bypass these arrays."""
        n, m, N, bt = self.n, self.m, self.N, self.batch
        out = dict(L=np.zeros((bt, N, n * n)), LR=np.zeros((bt, N, m * m)), G=np.zeros((bt, N, m * n)),
                   At=np.zeros((bt, N, n * n)), Bt=np.zeros((bt, N, n * m)), qt=np.zeros((bt, N, n)), rt=np.zeros((bt, N, m)),
                   dt=np.zeros((bt, N, n)), x0t=np.zeros((bt, n)))
        self._call("ndlqr_hip_download_cost_reduction", self.ctx, *[_ptr(a) for a in out.values()])
        return out

    # ---- linear inequality constraints (include/ndlqr.h: ndlqr_InitializeBatchFlatConstrained)
    def initialize_flat_constrained(self, A, B, Q, H, R, q, r, d, x0, C_, D_, lo, hi):
        """ndlqr_InitializeBatchFlatConstrained: the nine arrays of initialize_flat_dense, then the constraint rows
        lo <= C x + D u <= hi per knot: C_ [batch, N, p*n], D_ [batch, N, p*m] column-major per knot (p is taken from C_'s
        size) and lo, hi of shape (p,), (N, p) -- one set for every problem -- or (batch, N, p); entries may be +-inf.
        Arrays are numpy arrays or device memory (`ptr`, `size`). Afterwards the solver is in constrained mode
        (is_constrained()): dense-cost mode with solve_constrained() available."""
        n, m, N, bt = self.n, self.m, self.N, self.batch
        csize = C_.size
        if csize % (bt * N * n):
            raise ValueError("bad size for C")
        p = csize // (bt * N * n)
        sizes = dict(A=bt * N * n * n, B=bt * N * n * m, Q=bt * N * n * n, H=bt * N * n * m, R=bt * N * m * m,
                     q=bt * N * n, r=bt * N * m, d=bt * N * n, x0=bt * n, C=bt * N * p * n, D=bt * N * p * m)
        ptrs, keep = _stage(GRAD_DENSE_NAMES + ("C", "D"), (A, B, Q, H, R, q, r, d, x0, C_, D_), sizes)
        bounds, shared, keep2 = _stage_bounds([(lo, p, False), (hi, p, False)], N, bt)
        self._call("ndlqr_InitializeBatchFlatConstrained", self.h, *ptrs[:9], p, *ptrs[9:], *bounds, BOUNDS_SHARED if shared else 0)
        self._rows = p  # (only now: a refused call leaves the context, and the shapes checked here, as they were)

    def is_constrained(self):
        """ndlqr_BatchIsConstrained: True between initialize_flat_constrained and the next other initialiser."""
        return bool(self.L.ndlqr_BatchIsConstrained(self.h))

    def set_constraint_bounds(self, lo, hi):
        """ndlqr_BatchSetConstraintBounds: new lo, hi (shapes as for initialize_flat_constrained). Raises on a refusal
        (lo > hi, NaN, not in constrained mode); the previous bounds then stay."""
        if not self._rows:
            raise RuntimeError("ndlqr_BatchSetConstraintBounds: initialize_flat_constrained first")
        bounds, shared, keep = _stage_bounds([(lo, self._rows, False), (hi, self._rows, False)], self.N, self.batch)
        self._call("ndlqr_BatchSetConstraintBounds", self.h, *bounds, BOUNDS_SHARED if shared else 0)

    def solve_constrained(self, rho=0.0, alpha=0.0, eps_abs=0.0, eps_rel=0.0, max_iter=0, check_every=0, warm_start=False,
                          adapt_every=0):
        """ndlqr_SolveBatchLinConstrained (0 = the library's default of the box solve for every setting; adapt_every > 0 is
        refused: the adaptive penalty of this solve is switched on by set_constraint_adaptation). Returns (iters, status) as numpy int arrays [batch]; status 1 = converged, 2 = max_iter reached, 3 = not
        finite, 4 = certified infeasible (only after set_constraint_infeasibility(every > 0)). solutions() afterwards gives [lambda, x, u] of the last re-solve. Raises on a nonzero return."""
        return self._admm_solve("ndlqr_SolveBatchLinConstrained", (rho, alpha, eps_abs, eps_rel, int(max_iter), int(check_every),
                                                                   1 if warm_start else 0, int(adapt_every), 0.0, 0.0))

    def set_constraint_adaptation(self, every=0, rho_min=0.0, rho_max=0.0):
        """ndlqr_BatchSetConstraintPenaltyAdaptation: every > 0 gives the solve_constrained() calls that follow the
        per-problem adaptive penalty, considered every that many iterations within [rho_min, rho_max] (0: the library's
        1e-6 and 1e6); every = 0 (the initial state): off. Raises on a refusal (a negative argument, rho_min > rho_max);
        the previous setting then stays."""
        self._call("ndlqr_BatchSetConstraintPenaltyAdaptation", self.h, int(every), float(rho_min), float(rho_max))

    def constraint_penalties(self, rho=None):
        """ndlqr_CopyBatchConstraintPenalties: rho [batch] of the last solve_constrained (what an adaptive solve ended
        with); `rho`: destination (numpy array or DeviceArray)."""
        return self._copy_out("ndlqr_CopyBatchConstraintPenalties", (self.batch,), dest=rho)

    def set_constraint_infeasibility(self, every=0, eps=0.0):
        """ndlqr_BatchSetConstraintInfeasibilityDetection: every > 0 lets the solve_constrained() calls that follow test
        every running problem for a primal infeasibility certificate at the iterations it >= 2, it % every == 0 (status 4;
        eps = 0: 1e-4); every = 0 (the initial state): off. Raises on a refusal (every < 0, eps negative or not finite);
        the previous setting then stays."""
        self._call("ndlqr_BatchSetConstraintInfeasibilityDetection", self.h, int(every), float(eps))

    def constraint_infeasibility_certificate(self, dlam=None, dmu=None):
        """ndlqr_CopyBatchConstraintInfeasibilityCertificate: (dlam [batch, N, n], dmu [batch, N, p]) of the last
        solve_constrained, which ran with detection on: the Farkas certificate of every status-4 problem, zero rows for
        the others; `dlam`, `dmu`: destinations (numpy arrays or DeviceArrays). Raises on a refusal."""
        n, N, B, p = self.n, self.N, self.batch, self._rows or 1
        if dlam is None:
            dlam = np.zeros((B, N, n))
        if dmu is None:
            dmu = np.zeros((B, N, p))
        self._call("ndlqr_CopyBatchConstraintInfeasibilityCertificate", self.h, _any_ptr(dlam, B * N * n), _any_ptr(dmu, B * N * p))
        return dlam, dmu

    def constraint_infeasibility_measures(self, measures=None, iteration=None):
        """ndlqr_CopyBatchConstraintInfeasibilityMeasures: (measures [batch, 4], iteration [batch]) of the last
        solve_constrained, which ran with detection on: ||e||_inf, ||dmu||_inf, the largest |dmu_i| toward an infinite
        bound and S as the latest check of every problem found them, and the iteration of that check (0 and a row of
        zeros: no check examined the problem). Arguments as for infeasibility_measures. Raises on a refusal."""
        return self._measures("ndlqr_CopyBatchConstraintInfeasibilityMeasures", measures, iteration)

    def constraint_multipliers(self):
        """ndlqr_CopyBatchConstraintMultipliers: mu = rho y, [batch, N, p]."""
        return self._copy_out("ndlqr_CopyBatchConstraintMultipliers", (self.batch, self.N, self._rows or 1))

    def constraint_residuals(self):
        """ndlqr_CopyBatchConstraintResiduals: [batch, 4] = r_prim | r_dual | s_prim | s_dual of the last constrained solve."""
        return self._copy_out("ndlqr_CopyBatchConstraintResiduals", (self.batch, 4))

    def constraint_reduction(self):
        """ndlqr_hip_download_constraint_reduction (read-out for the tests): dict of numpy arrays -- the shifted costs Qs, Hs,
        Rs, the shifted records L, LR, G and reduced problem At .. x0t (as cost_reduction gives the plain ones), and the
        iterates v, y [batch, N, p] of the latest constrained solve."""
        n, m, N, bt, p = self.n, self.m, self.N, self.batch, self._rows or 1
        out = dict(Qs=np.zeros((bt, N, n * n)), Hs=np.zeros((bt, N, n * m)), Rs=np.zeros((bt, N, m * m)),
                   L=np.zeros((bt, N, n * n)), LR=np.zeros((bt, N, m * m)), G=np.zeros((bt, N, m * n)),
                   At=np.zeros((bt, N, n * n)), Bt=np.zeros((bt, N, n * m)), qt=np.zeros((bt, N, n)), rt=np.zeros((bt, N, m)),
                   dt=np.zeros((bt, N, n)), x0t=np.zeros((bt, n)), v=np.zeros((bt, N, p)), y=np.zeros((bt, N, p)))
        self._call("ndlqr_hip_download_constraint_reduction", self.ctx, *[_ptr(a) for a in out.values()])
        return out

    # ---- gradients through the solve with linear inequality constraints (include/ndlqr.h: ndlqr_SolveBatchLinAdjoint,
    # ndlqr_BatchConstraintGradients)
    def solve_constrained_adjoint(self, g, alpha=0.0, eps_abs=0.0, eps_rel=0.0, max_iter=0, check_every=0):
        """ndlqr_SolveBatchLinAdjoint: the adjoint of the active-set system of the last solve_constrained for g = dL/dz*
        [batch, nvars] (numpy array or DeviceArray), on the forward's remembered shifted factorisation (its rho, a cold
        start; 0 = the library's default for every setting). Returns (iters, status) as numpy int arrays [batch]; status 1 =
        converged, 2 = max_iter reached, 3 = not finite (or the forward's was, or the forward certified the problem infeasible:
        not iterated, w = 0, zero gradients).
        Raises on a nonzero return. Afterwards adjoint() gives w in the caller's variables and constraint_gradients(),
        constraint_adjoint_multipliers(), constraint_adjoint_residuals() and constraint_codes() read the rest."""
        return self._admm_solve("ndlqr_SolveBatchLinAdjoint", (0.0, alpha, eps_abs, eps_rel, int(max_iter), int(check_every), 0),
                                _doubles(g))

    def constraint_gradients(self, summed=False, out=None):
        """ndlqr_BatchConstraintGradients: dict with keys C, D, lo, hi -> dL/d(C, D, lo, hi) of the last constrained
        adjoint: C [batch, N, p*n] and D [batch, N, p*m] column-major per knot like the inputs, lo, hi [batch, N, p]; or
        without the batch dimension, summed over the batch (NDLQR_BOUNDS_SHARED; two calls give the same bits). `out`:
        dict of destinations (numpy arrays or DeviceArrays); only those keys are computed. Default: numpy arrays for all
        four."""
        n, m, N, B, p = self.n, self.m, self.N, self.batch, self._rows or 1
        shapes = {k: ((N, w) if summed else (B, N, w)) for k, w in (("C", p * n), ("D", p * m), ("lo", p), ("hi", p))}
        return self._named_gradients("ndlqr_BatchConstraintGradients", shapes, out, BOUNDS_SHARED if summed else 0, False,
                                     "constraint gradient")

    def constraint_adjoint_multipliers(self):
        """ndlqr_CopyBatchConstraintAdjointMultipliers: nu = rho y of the last constrained adjoint, [batch, N, p] (zero
        outside the active set)."""
        return self._copy_out("ndlqr_CopyBatchConstraintAdjointMultipliers", (self.batch, self.N, self._rows or 1))

    def constraint_adjoint_residuals(self, resid=None):
        """ndlqr_CopyBatchConstraintAdjointResiduals: [batch, 4] = r_prim | r_dual | s_prim | s_dual of the last constrained
        adjoint (a row of zeros for a problem it did not iterate)."""
        return self._copy_out("ndlqr_CopyBatchConstraintAdjointResiduals", (self.batch, 4), dest=resid)

    def constraint_codes(self):
        """ndlqr_CopyBatchConstraintCodes: uint8 [batch, N, p] of the last constrained adjoint -- 0 unbounded, 1 bounded
        and inactive, 2 active at lo, 3 active at hi."""
        return self._copy_out("ndlqr_CopyBatchConstraintCodes", (self.batch, self.N, self._rows or 1), np.uint8)

    # ---- active-set polish of the solve with linear inequality constraints (include/ndlqr.h:
    # ndlqr_PolishBatchLinConstrained)
    def polish_constrained(self, sigma=0.0, max_steps=0, max_rounds=0, steps=None, status=None):
        """ndlqr_PolishBatchLinConstrained on the latest solve_constrained (0 = the library's default for every setting).
        steps / status: int32 destinations [batch] (numpy arrays or device memory with `ptr`); default: new numpy arrays.
        Returns (steps, status): the accepted steps, and 1 = polished, 2 = not polished (the ADMM solution, v, y stay), 3 =
        not finite. Raises on a nonzero return."""
        return self._polish("ndlqr_PolishBatchLinConstrained", (sigma, int(max_steps), int(max_rounds)), steps, status)

    def constraint_polish_codes(self):
        """ndlqr_CopyBatchConstraintPolishCodes: uint8 [batch, N, p] of the latest polish_constrained -- 0 unbounded, 1
        bounded and inactive, 2 active at lo, 3 active at hi."""
        return self._copy_out("ndlqr_CopyBatchConstraintPolishCodes", (self.batch, self.N, self._rows or 1), np.uint8)

    def constraint_polish_residual(self, z, mu, codes, sig, poison_pad=False):
        """ndlqr_hip_constraint_polish_residual (test hook): the residual kernel of the polish alone on z [batch, nvars], mu,
        codes [batch, N, p] and sigma_p [batch]; poison_pad: the pad entries and pad knots of the device's z hold NaN
        instead of zero. Returns (r [batch, nvars], rc [batch, N, p], norms [2, batch])."""
        p = self._rows or 1
        z = np.ascontiguousarray(z, dtype=np.float64)
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        sig = np.ascontiguousarray(sig, dtype=np.float64)
        assert z.shape == (self.batch, self.nvars) and mu.shape == codes.shape == (self.batch, self.N, p) and sig.shape == (self.batch,)
        r, rc, norms = np.zeros_like(z), np.zeros_like(mu), np.zeros((2, self.batch))
        self._call("ndlqr_hip_constraint_polish_residual", self.ctx, _ptr(z), _ptr(mu), codes.ctypes.data_as(C.POINTER(C.c_ubyte)),
                   _ptr(sig), 1 if poison_pad else 0, _ptr(r), _ptr(rc), _ptr(norms))
        return r, rc, norms

    def constraint_polish_phase_ms(self):
        """ndlqr_hip_constraint_polish_phase_ms: under FLAG_PROFILE, (ms [3], launches [3]) of the latest polish_constrained --
        residuals | S' + re-solves | updates."""
        ms, cnt = np.zeros(3), np.zeros(3, dtype=np.int32)
        self.L.ndlqr_hip_constraint_polish_phase_ms(self.ctx, _ptr(ms), cnt.ctypes.data_as(C.POINTER(C.c_int)))
        return ms, cnt

    def constraint_polish_state(self, max_steps=8):
        """ndlqr_hip_download_constraint_polish_state (test hook): dict of the latest polish_constrained -- zc [batch, nvars]
        and muc [batch, N, p], the candidate of its last formed step; norms [2, max_steps + 1, batch], the slots of its last
        round (max_steps: that of the call); sig [batch]; rounds, its factorisations."""
        p = self._rows or 1
        out = dict(zc=np.zeros((self.batch, self.nvars)), muc=np.zeros((self.batch, self.N, p)), sig=np.zeros(self.batch))
        norms = np.zeros(2 * 33 * self.batch)
        rounds = C.c_int(0)
        self._call("ndlqr_hip_download_constraint_polish_state", self.ctx, _ptr(out["zc"]), _ptr(out["muc"]), _ptr(norms),
                   _ptr(out["sig"]), C.byref(rounds))
        out["norms"] = norms[: 2 * (max_steps + 1) * self.batch].reshape(2, max_steps + 1, self.batch).copy()
        out["rounds"] = rounds.value
        return out

    def constraint_adjoint_iterate(self):
        """ndlqr_hip_download_constraint_codes (read-out for the tests): the constrained adjoint's own projected iterate
        v [batch, N, p] (0 on the fixed and the unbounded rows)."""
        out = np.zeros((self.batch, self.N, self._rows or 1))
        self._call("ndlqr_hip_download_constraint_codes", self.ctx, None, _ptr(out))
        return out

    def initialize_synthetic(self, seed0):
        self._call("ndlqr_InitializeBatchSynthetic", self.h, seed0, detail=False)

    def solve(self):
        return self.L.ndlqr_SolveBatch(self.h)

    def set_rhs_flat(self, q, r, d, x0):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (q, r, d, x0)]
        self._call("ndlqr_BatchSetRhsFlat", self.h, *[_ptr(a) for a in arrs], detail=False)

    def solve_rhs_only(self):
        """Solution sweep against the cached factorisation (needs FLAG_KEEP_FACT, or FLAG_KEEP_RECORDS
        in fast mode on a size-specialised shape, on the solve)."""
        return self.L.ndlqr_SolveBatchRhsOnly(self.h)

    def solve_multi_rhs(self, q, r, d, x0, out=None, selection=None):
        """nrhs sets of right-hand sides for the whole batch against the records kept by the last solve (FLAG_KEEP_RECORDS,
        level-per-launch schedule): q, d [nrhs][batch][N][n], r [nrhs][batch][N][m], x0 [nrhs][batch][n] ->
        solutions [nrhs][batch][nvars], or with selection = (knot0, nknots, blocks) that slice of every solution,
        [nrhs][batch][nknots][width] (ndlqr_SolveBatchMultiRhsSlices: nothing else is computed by the last launch).
        Blocking; solve_ms() afterwards = device time of the solve kernels alone."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (q, r, d, x0)]
        nrhs = arrs[3].shape[0]
        assert arrs[0].shape == (nrhs, self.batch, self.N, self.n) and arrs[1].shape == (nrhs, self.batch, self.N, self.m)
        assert arrs[2].shape == (nrhs, self.batch, self.N, self.n) and arrs[3].shape == (nrhs, self.batch, self.n)
        if selection is not None:
            k0, nk, blocks = selection
            if out is None:
                out = np.empty((nrhs, self.batch, nk, self.slice_width(blocks)))
            assert out.size == nrhs * self.batch * nk * self.slice_width(blocks)
            err = self.L.ndlqr_SolveBatchMultiRhsSlices(self.h, nrhs, *[_ptr(a) for a in arrs], k0, nk, blocks, _ptr(out))
        else:
            if out is None:
                out = np.empty((nrhs, self.batch, self.nvars))
            err = self.L.ndlqr_SolveBatchMultiRhs(self.h, nrhs, *[_ptr(a) for a in arrs], _ptr(out))
        if err:  # (not through _call: the message names the plain call for both)
            raise RuntimeError("ndlqr_SolveBatchMultiRhs failed: %d (%s)" % (err, self.L.ndlqr_hip_last_error().decode()))
        return out

    def solve_async(self):
        return self.L.ndlqr_SolveBatchAsync(self.h)

    def slice_width(self, blocks):
        return (self.n if blocks & SOLN_LAMBDA else 0) + (self.n if blocks & SOLN_STATE else 0) + \
               (self.m if blocks & SOLN_INPUT else 0)

    def set_step_selection(self, knot0=0, nknots=0, blocks=7):
        """ndlqr_BatchSetStepSelection: what step_async brings down -- knots [knot0, knot0 + nknots), blocks = SOLN_*
        mask, packed [batch, nknots, width]; nknots = 0: every solution [batch, nvars] (default). With SOLN_ONLY in the
        mask a step computes nothing but those knots (the rest of the solution is unavailable until the next complete
        solve)."""
        err = self.L.ndlqr_BatchSetStepSelection(self.h, knot0, nknots, blocks)
        if err:
            raise ValueError("ndlqr_BatchSetStepSelection(%d, %d, %d): %d" % (knot0, nknots, blocks, err))
        self._sel = (knot0, nknots, blocks) if nknots else None

    def solve_slices_async(self, knot0, nknots, blocks, out):
        """ndlqr_SolveBatchSlicesAsync: factor + solve of the resident problems, computing and delivering knots
        [knot0, knot0 + nknots) alone into `out` ([batch, nknots, width]: a pinned_empty array or a DeviceArray);
        complete after synchronize()."""
        size = self.batch * nknots * self.slice_width(blocks)
        assert out.size == size and (isinstance(out, DeviceArray) or (out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]))
        self._step_refs = self._step_refs[-1:] + [(out,)]
        ptr = C.cast(C.c_void_p(out.ptr), dp) if isinstance(out, DeviceArray) else _ptr(out)
        return self.L.ndlqr_SolveBatchSlicesAsync(self.h, knot0, nknots, blocks, ptr)

    def solution_slices(self, knot0, nknots, blocks, out=None):
        """ndlqr_CopyBatchSolutionSlices: [batch, nknots, width] of the latest solve."""
        if out is None:
            out = np.zeros((self.batch, nknots, self.slice_width(blocks)))
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.size == self.batch * nknots * self.slice_width(blocks)
        self._call("ndlqr_CopyBatchSolutionSlices", self.h, knot0, nknots, blocks, _ptr(out), detail=False)
        return out

    def step_async(self, q, r, d, x0, soln):
        """ndlqr_BatchStepAsync: new right-hand side up, factor + solve, solutions down into `soln` ([batch, nvars], or
        the slice chosen with set_step_selection), asynchronously. Use pinned_empty() arrays (pageable ones make the
        call block) or DeviceArray objects (no transfer at all) and leave them untouched until the step has been synchronised; the solver holds references to the
        arrays of the two steps that can be in flight, so that dropping one early does not free pinned memory the GPU
        is still reading or writing."""
        n, m, N, bt = self.n, self.m, self.N, self.batch
        out_size = bt * self.nvars if self._sel is None else bt * self._sel[1] * self.slice_width(self._sel[2])
        for a, size in ((q, bt * N * n), (r, bt * N * m), (d, bt * N * n), (x0, bt * n), (soln, out_size)):
            assert a is None or (a.size == size if isinstance(a, DeviceArray) else
                                 (a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.size == size))
        assert x0 is not None and soln is not None  # q, r, d may be None: unchanged
        ptr = lambda a: None if a is None else (C.cast(C.c_void_p(a.ptr), dp) if isinstance(a, DeviceArray) else _ptr(a))
        self._step_refs = self._step_refs[-1:] + [(q, r, d, x0, soln)]
        return self.L.ndlqr_BatchStepAsync(self.h, ptr(q), ptr(r), ptr(d), ptr(x0), ptr(soln))

    # ---- the step and the slices in dense-cost mode (include/ndlqr.h: ndlqr_BatchStepAsyncDense)
    def step_dense_async(self, q, r, d, x0, out, selection=None):
        """ndlqr_BatchStepAsyncDense: step_async for a dense-cost problem, in the caller's variables. q and r come together
        or are both None (unchanged), d may be None, x0 and out are required. selection = (knot0, nknots, blocks) delivers
        that slice, [batch, nknots, width] (with SOLN_ONLY in blocks nothing else is computed); None: every solution
        [batch, nvars]. Arrays as for step_async: pinned_empty() ones, DeviceArray objects, or pageable numpy arrays (the
        call then blocks); the solver holds references to those of the two steps that can be in flight. Returns the error
        code; ValueError for arrays of the wrong size, q without r, or a refusal of the library (its message)."""
        n, m, N, bt = self.n, self.m, self.N, self.batch
        if (q is None) != (r is None):
            raise ValueError("step_dense_async: q and r are replaced together or not at all")
        if x0 is None or out is None:
            raise ValueError("step_dense_async: x0 and out are required")
        k0, nk, blocks = (0, 0, 7) if selection is None else selection
        out_size = bt * self.nvars if nk == 0 else bt * nk * self.slice_width(blocks)
        ptrs = [None if a is None else _any_ptr(a, size) for a, size in
                ((q, bt * N * n), (r, bt * N * m), (d, bt * N * n), (x0, bt * n), (out, out_size))]
        self._step_refs = self._step_refs[-1:] + [(q, r, d, x0, out)]
        err = self.L.ndlqr_BatchStepAsyncDense(self.h, *ptrs[:4], k0, nk, blocks, ptrs[4])
        if err == ERR_INVALID:
            raise ValueError("ndlqr_BatchStepAsyncDense: %s" % self.L.ndlqr_hip_last_error().decode())
        return err

    def solve_slices_dense_async(self, knot0, nknots, blocks, out):
        """ndlqr_SolveBatchSlicesAsyncDense: solve_slices_async for a dense-cost problem -- the slice in the caller's
        variables into `out` ([batch, nknots, width]); complete after synchronize()."""
        ptr = _any_ptr(out, self.batch * max(nknots, 0) * self.slice_width(blocks))
        self._step_refs = self._step_refs[-1:] + [(out,)]
        err = self.L.ndlqr_SolveBatchSlicesAsyncDense(self.h, knot0, nknots, blocks, ptr)
        if err == ERR_INVALID:
            raise ValueError("ndlqr_SolveBatchSlicesAsyncDense: %s" % self.L.ndlqr_hip_last_error().decode())
        return err

    def solution_slices_dense(self, knot0, nknots, blocks, out=None):
        """ndlqr_CopyBatchSolutionSlicesDense: [batch, nknots, width] of the latest solve of a dense-cost problem, in the
        caller's variables."""
        if out is None:
            out = np.zeros((self.batch, max(nknots, 0), self.slice_width(blocks)))
        ptr = _any_ptr(out, self.batch * max(nknots, 0) * self.slice_width(blocks))
        self._call("ndlqr_CopyBatchSolutionSlicesDense", self.h, knot0, nknots, blocks, ptr)
        return out

    def rhs_raw(self):
        """ndlqr_hip_download_rhs_raw (read-out for the tests): the latest right-hand side as it lies on the device,
        [batch, doubles per problem] in the device's block sizes and horizon, pad rows and tail knots included. Waits for
        everything in flight. Every mode."""
        shape = (self.batch, int(self.L.ndlqr_hip_rhs_raw_doubles(self.ctx)) // self.batch)
        return self._copy_out("ndlqr_hip_download_rhs_raw", shape, via_ctx=True)

    # ---- time-axis sharding (one problem over G ranks; include/ndlqr_hip.h)
    def time_shard_top_doubles(self, G):
        return self.L.ndlqr_BatchTimeShardTopDoubles(self.h, G)

    def time_shard_factor(self, g, G):
        return self.L.ndlqr_BatchTimeShardFactor(self.h, g, G)

    def time_shard_export(self, G, ptr):
        """`ptr`: address (int) of host or device memory for time_shard_top_doubles(G) doubles."""
        return self.L.ndlqr_BatchTimeShardExportTop(self.h, G, C.c_void_p(int(ptr)))

    def time_shard_import(self, G, ptr):
        return self.L.ndlqr_BatchTimeShardImportTop(self.h, G, C.c_void_p(int(ptr)))

    def time_shard_finish(self, g, G):
        return self.L.ndlqr_BatchTimeShardFinish(self.h, g, G)

    def synchronize_previous(self):
        return self.L.ndlqr_BatchSynchronizePrevious(self.h)

    def synchronize(self):
        err = self.L.ndlqr_BatchSynchronize(self.h)
        self._step_refs = []
        return err

    def solve_ms(self):
        return self.L.ndlqr_BatchSolveTimeMs(self.h)

    def solution(self, p):
        out = np.zeros(self.nvars)
        self._call("ndlqr_CopyBatchSolution", self.h, p, _ptr(out), detail=False, ok=(self.nvars,))
        return out

    def kkt_residuals(self):
        """(res, bnorm): ||K z - b||_2 and ||b||_2 of every problem, evaluated on the device."""
        res = np.zeros(self.batch)
        bn = np.zeros(self.batch)
        self._call("ndlqr_BatchKktResiduals", self.h, _ptr(res), _ptr(bn), detail=False)
        return res, bn

    def solutions(self, out=None):
        """[batch, nvars] solutions of the latest solve; `out`: destination (e.g. a pinned_empty array)."""
        if out is None:
            out = np.zeros((self.batch, self.nvars))
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.size == self.batch * self.nvars
        self._call("ndlqr_CopyBatchSolutions", self.h, _ptr(out), detail=False, ok=(self.nvars,))
        return out

    # ---- adjoint solve and parameter gradients (include/ndlqr.h: ndlqr_SolveBatchAdjoint, ndlqr_BatchGradients)
    def solve_adjoint(self, g):
        """ndlqr_SolveBatchAdjoint: K w = g for g = dL/dz [batch, nvars] (numpy array or DeviceArray) against the
        factorisation the last solve kept (FLAG_KEEP_RECORDS or FLAG_KEEP_FACT). Returns the C return code (0, or -1 when
        there is no kept factorisation of the resident solution)."""
        return self.L.ndlqr_SolveBatchAdjoint(self.h, _any_ptr(_doubles(g), self.batch * self.nvars))

    def adjoint(self, out=None):
        """ndlqr_CopyBatchAdjoint: the adjoint solution w [batch, nvars] into `out` (numpy array or DeviceArray)."""
        if out is None:
            out = np.zeros((self.batch, self.nvars))
        self._call("ndlqr_CopyBatchAdjoint", self.h, _any_ptr(out, self.batch * self.nvars), ok=(self.nvars,))
        return out

    def gradient_shape(self, name, summed=False):
        """Shape of gradient `name` (GRAD_NAMES) in the flat layout, per problem or summed over the batch."""
        n, m, N = self.n, self.m, self.N
        per = dict(A=(N, n * n), B=(N, n * m), Q=(N, n), R=(N, m), q=(N, n), r=(N, m), d=(N, n), x0=(n,))[name]
        return per if summed else (self.batch,) + per

    def gradients(self, sum_mask=0, out=None):
        """ndlqr_BatchGradients: dict name -> dL/d(name) for the names of GRAD_NAMES, in the flat layout of
        initialize_flat (A, B column-major per knot); those whose bit is in sum_mask (GRAD_*) summed over the batch.
        `out`: dict of destinations (numpy arrays or DeviceArrays); only those names are computed. Default: numpy arrays
        for all eight."""
        shapes = {k: self.gradient_shape(k, bool(sum_mask & (1 << i))) for i, k in enumerate(GRAD_NAMES)}
        return self._named_gradients("ndlqr_BatchGradients", shapes, out, sum_mask, True, "gradient")

    def dense_gradient_shape(self, name, summed=False):
        """Shape of gradient `name` (GRAD_DENSE_NAMES) in the flat layout of initialize_flat_dense, per problem or summed
        over the batch."""
        n, m, N = self.n, self.m, self.N
        per = dict(A=(N, n * n), B=(N, n * m), Q=(N, n * n), H=(N, n * m), R=(N, m * m), q=(N, n), r=(N, m), d=(N, n),
                   x0=(n,))[name]
        return per if summed else (self.batch,) + per

    def gradients_dense(self, sum_mask=0, out=None):
        """ndlqr_BatchGradientsDense: dict name -> dL/d(name) for the names of GRAD_DENSE_NAMES in dense-cost mode, after
        solve_adjoint or -- on a constrained solution -- solve_constrained_adjoint, in the flat layout of
        initialize_flat_dense (matrices column-major per knot); those whose bit is in sum_mask (GRADD_*) summed over the
        batch. `out`: dict of destinations (numpy arrays or DeviceArrays); only those names are computed. Default: numpy
        arrays for all nine."""
        shapes = {k: self.dense_gradient_shape(k, bool(sum_mask & (1 << i))) for i, k in enumerate(GRAD_DENSE_NAMES)}
        return self._named_gradients("ndlqr_BatchGradientsDense", shapes, out, sum_mask, True, "gradient")

    # ---- feedback gains and cost-to-go matrices (include/ndlqr.h: ndlqr_BatchFeedbackGains)
    def feedback_gains(self, knot0=0, nknots=None, want=("K", "k", "P", "p"), out=None):
        """ndlqr_BatchFeedbackGains: u_k = K_k x_k + k_k and lambda_k = P_k x_k + p_k of the resident problems and the
        latest right-hand side, for the knots [knot0, knot0 + nknots) (nknots=None: to the end of the horizon). Returns a
        dict of numpy arrays in the math convention -- K [batch, nknots, m, n], k [batch, nknots, m], P [batch, nknots, n, n],
        p [batch, nknots, n], those named in `want` -- plus "failures", int32 [batch]. With `out`, a dict of pinned_empty
        arrays or DeviceArrays in the flat shapes of the C API (K [batch, nknots, m*n] column-major per knot, P
        [batch, nknots, n*n]), those are filled and returned instead (`want` is ignored). Raises RuntimeError with the
        library's message on a refusal. A pivot that was not positive does not raise: the dict comes back with
        failures[problem] > 0 for the problems concerned (their outputs are finite, not meaningful); MPC use:
        feedback_gains(0, 1, want=("K",))["K"][:, 0]."""
        n, m, bt = self.n, self.m, self.batch
        if nknots is None:
            nknots = self.N - knot0
        flat = dict(K=(bt, nknots, m * n), k=(bt, nknots, m), P=(bt, nknots, n * n), p=(bt, nknots, n))
        names = tuple(out) if out is not None else tuple(want)
        unknown = set(names) - set(flat)
        if unknown:
            raise ValueError("unknown output names: %s" % sorted(unknown))
        flat = {k: tuple(max(s, 0) for s in v) for k, v in flat.items()}  # (an empty range is the library's to refuse)
        res = dict(out) if out is not None else {k: np.zeros(flat[k]) for k in names}
        ptrs = [None if res.get(k) is None else _any_ptr(res[k], int(np.prod(flat[k]))) for k in ("K", "k", "P", "p")]
        failures = np.zeros(bt, dtype=np.int32)
        self._call("ndlqr_BatchFeedbackGains", self.h, int(knot0), int(nknots), *ptrs, _int_ptr(failures, bt), ok=(0, ERR_NOT_SPD))
        if out is None:
            for k in ("K", "P"):
                if k in res:
                    rows = m if k == "K" else n
                    res[k] = np.ascontiguousarray(res[k].reshape(bt, nknots, n, rows).transpose(0, 1, 3, 2))
        res["failures"] = failures
        return res

    # ---- objective values and stage costs (include/ndlqr.h: ndlqr_BatchObjective)
    def objective(self, stage=False, out=None):
        """ndlqr_BatchObjective: the value of the cost every problem minimised at its resident solution -- with the caller's
        costs (dense-cost mode: the caller's Q, H, R; after a constrained solve or polish: the unshifted cost at the
        delivered iterate) and the right-hand side that produced the solution. Returns {"J": [batch]} and, with
        stage=True, "stage": [batch, N], the stage costs l_k (J is their sum; the last knot has no input terms), as numpy
        arrays. With `out`, a dict of numpy arrays (pinned_empty ones included) or DeviceArrays under those names, those
        are filled and returned instead (`stage` is ignored: "stage" is computed when it is in `out`; "J" is required).
        Accumulated in double-double and rounded once; the bits do not depend on the flag mode, the memory of the outputs
        or whether the stage costs were asked for. Raises RuntimeError with the library's message on a refusal (no full
        resident solution, a time-axis shard)."""
        shapes = dict(J=(self.batch,), stage=(self.batch, self.N))
        if out is not None:
            unknown = set(out) - set(shapes)
            if unknown:
                raise ValueError("unknown output names: %s" % sorted(unknown))
            res = dict(out)
        else:
            res = {k: np.zeros(shapes[k]) for k in (("J", "stage") if stage else ("J",))}
        ptrs = [None if res.get(k) is None else _any_ptr(res[k], int(np.prod(shapes[k]))) for k in ("J", "stage")]
        self._call("ndlqr_BatchObjective", self.h, *ptrs)
        return res

    # ---- iterative refinement (include/ndlqr.h: ndlqr_RefineBatch, ndlqr_RefineBatchAdjoint, ndlqr_BatchKktResidualVector)
    def _refine(self, name, max_steps):
        steps = np.zeros(self.batch, dtype=np.int32)
        before, after = np.zeros(self.batch), np.zeros(self.batch)
        self._call(name, self.h, int(max_steps), _int_ptr(steps, self.batch), _ptr(before), _ptr(after))
        return steps, before, after

    def refine(self, max_steps=2):
        """ndlqr_RefineBatch: up to max_steps (1 .. 8) steps of iterative refinement of the resident solutions with a
        double-double residual, against the factorisation the last solve kept (FLAG_KEEP_RECORDS or FLAG_KEEP_FACT).
        Returns (steps, eta_before, eta_after), numpy arrays [batch]: the steps every problem took (a step counts while the
        residual norm fell at every step so far) and eta = ||r||_inf / max_i(|b_i| + sum_j |K_ij| |z_j|) before and after
        them. Raises on a refusal (no kept factorisation of the resident solution)."""
        return self._refine("ndlqr_RefineBatch", max_steps)

    def refine_adjoint(self, max_steps=2):
        """ndlqr_RefineBatchAdjoint: the same for w of the latest solve_adjoint against its g."""
        return self._refine("ndlqr_RefineBatchAdjoint", max_steps)

    def kkt_residual_vector(self, out=None):
        """ndlqr_BatchKktResidualVector: r = b - K z of the resident solutions, [batch, nvars] in the packing of solutions(),
        every row accumulated in double-double and rounded once; `out`: destination (numpy array or DeviceArray)."""
        return self._copy_out("ndlqr_BatchKktResidualVector", (self.batch, self.nvars), dest=out)

    def refine_phase_ms(self):
        """(residual, re-solve, commit) device times in ms of the latest refinement that ran under FLAG_PROFILE."""
        out = np.zeros(3)
        self.L.ndlqr_hip_refine_phase_ms(self.ctx, _ptr(out))
        return tuple(out)

    # ---- box-constrained solve (include/ndlqr.h: ndlqr_BatchSetBounds, ndlqr_SolveBatchBoxConstrained)
    def set_bounds(self, xlo=None, xhi=None, ulo=None, uhi=None):
        """ndlqr_BatchSetBounds. Each bound is None (unbounded), a numpy array of shape (n,) / (m,), (N, n) / (N, m) --
        one set for every problem, sent as NDLQR_BOUNDS_SHARED -- or (batch, N, n) / (batch, N, m), or a DeviceArray of
        batch * N * n (m) doubles. Entries may be +-inf. Raises on a refusal (lo > hi)."""
        n, m = self.n, self.m
        ptrs, shared, keep = _stage_bounds([(xlo, n, True), (xhi, n, True), (ulo, m, True), (uhi, m, True)], self.N, self.batch)
        self._call("ndlqr_BatchSetBounds", self.h, BOUNDS_SHARED if shared else 0, *ptrs)

    def solve_box(self, rho=0.0, alpha=0.0, eps_abs=0.0, eps_rel=0.0, max_iter=0, check_every=0, warm_start=False,
                  adapt_every=0, rho_min=0.0, rho_max=0.0):
        """ndlqr_SolveBatchBoxConstrained (0 = the library's default for every setting). adapt_every > 0: the per-problem
        adaptive penalty, considered every that many iterations and kept within [rho_min, rho_max]; 0: fixed rho. Returns
        (iters, status) as numpy int arrays [batch]; status 1 = converged, 2 = max_iter reached, 3 = not finite, 4 = primal
        infeasible with a certificate (only after set_box_infeasibility(every > 0)). Raises on a nonzero return."""
        return self._admm_solve("ndlqr_SolveBatchBoxConstrained", (rho, alpha, eps_abs, eps_rel, int(max_iter), int(check_every),
                                                                   1 if warm_start else 0, int(adapt_every), rho_min, rho_max))

    def set_box_infeasibility(self, every=0, eps=0.0):
        """ndlqr_BatchSetInfeasibilityDetection: every > 0 lets the constrained solves that follow test every running
        problem for a primal infeasibility certificate at the iterations it % every == 0 (status 4; eps = 0: 1e-4);
        every = 0 (the initial state): off. Raises on a refusal (every < 0, eps negative or not finite); the previous
        setting then stays."""
        self._call("ndlqr_BatchSetInfeasibilityDetection", self.h, int(every), float(eps))

    def infeasibility_certificate(self, dlam=None, dmu_x=None, dmu_u=None):
        """ndlqr_CopyBatchInfeasibilityCertificate: (dlam [batch, N, n], dmu_x [batch, N, n], dmu_u [batch, N, m]) of the
        last constrained solve, which ran with detection on: the Farkas certificate of every status-4 problem, zero rows
        for the others; `dlam`, `dmu_x`, `dmu_u`: destinations (numpy arrays or DeviceArrays). Raises on a refusal."""
        n, m, N, B = self.n, self.m, self.N, self.batch
        if dlam is None:
            dlam = np.zeros((B, N, n))
        if dmu_x is None:
            dmu_x = np.zeros((B, N, n))
        if dmu_u is None:
            dmu_u = np.zeros((B, N, m))
        self._call("ndlqr_CopyBatchInfeasibilityCertificate", self.h, _any_ptr(dlam, B * N * n), _any_ptr(dmu_x, B * N * n),
                   _any_ptr(dmu_u, B * N * m))
        return dlam, dmu_x, dmu_u

    def infeasibility_measures(self, measures=None, iteration=None):
        """ndlqr_CopyBatchInfeasibilityMeasures: (measures [batch, 4], iteration [batch]) of the last constrained solve,
        which ran with detection on: ||e||_inf, ||dmu||_inf, the largest |dmu_i| toward an infinite bound and S as the
        latest check of every problem found them, and the iteration of that check (0 and a row of zeros: no check examined
        the problem). `measures`: destination (numpy array or DeviceArray); `iteration`: a C-contiguous int32 numpy array,
        or anything with `ptr` addressing batch ints of device memory. Raises on a refusal."""
        return self._measures("ndlqr_CopyBatchInfeasibilityMeasures", measures, iteration)

    def set_box_acceleration(self, mem=0, safeguard=0.0, reg=0.0):
        """ndlqr_BatchSetBoxAcceleration: mem in 1 .. 16 lets the constrained solves that follow take safeguarded
        Anderson-accelerated steps from the last mem iterations (safeguard = 0: 1.0, reg = 0: 1e-10; 5 is the documented
        memory); mem = 0 (the initial state): off. Raises on a refusal (mem outside 0 .. 16, safeguard or reg negative or
        not finite); the previous setting then stays."""
        self._call("ndlqr_BatchSetBoxAcceleration", self.h, int(mem), float(safeguard), float(reg))
        self._accel_mem = int(mem)

    def box_acceleration(self):
        """ndlqr_CopyBatchBoxAcceleration: (accepted [batch], rejected [batch], gamma [batch, mem], columns [batch]) of
        the last constrained solve, which ran with acceleration on: the steps it took accelerated, the steps its
        safeguard rejected, and the coefficients and column count of every problem's latest accelerated step. Raises on
        a refusal."""
        B, mem = self.batch, self._accel_mem
        ints = [np.zeros(B, dtype=np.int32) for _ in range(3)]
        gamma = np.zeros((B, max(mem, 1)))
        ip = [_int_ptr(a, B) for a in ints]
        self._call("ndlqr_CopyBatchBoxAcceleration", self.h, ip[0], ip[1], _ptr(gamma), ip[2])
        return ints[0], ints[1], gamma[:, :mem], ints[2]

    def box_penalties(self, rho=None):
        """ndlqr_CopyBatchBoxPenalties: rho [batch] of the last constrained solve (what an adaptive solve ended with);
        `rho`: destination (numpy array or DeviceArray)."""
        return self._copy_out("ndlqr_CopyBatchBoxPenalties", (self.batch,), dest=rho)

    def box_residuals(self, resid=None):
        """ndlqr_CopyBatchBoxResiduals: [batch, 4] = r_prim | r_dual | s_prim | s_dual of the last constrained solve, the
        numbers of the convergence test as the last update of every problem found them (its freezing iteration, or
        max_iter for status 2); `resid`: destination (numpy array or DeviceArray). Raises on a refusal."""
        return self._copy_out("ndlqr_CopyBatchBoxResiduals", (self.batch, 4), dest=resid)

    def box_adjoint_residuals(self, resid=None):
        """ndlqr_CopyBatchBoxAdjointResiduals: the same of the last box adjoint (a row of zeros for a problem it did
        not iterate)."""
        return self._copy_out("ndlqr_CopyBatchBoxAdjointResiduals", (self.batch, 4), dest=resid)

    def bound_multipliers(self, mu_x=None, mu_u=None):
        """ndlqr_CopyBatchBoundMultipliers: (mu_x [batch, N, n], mu_u [batch, N, m]) = rho y of the last constrained solve;
        `mu_x`, `mu_u`: destinations (numpy arrays or DeviceArrays)."""
        n, m, N, B = self.n, self.m, self.N, self.batch
        if mu_x is None:
            mu_x = np.zeros((B, N, n))
        if mu_u is None:
            mu_u = np.zeros((B, N, m))
        self._call("ndlqr_CopyBatchBoundMultipliers", self.h, _any_ptr(mu_x, B * N * n), _any_ptr(mu_u, B * N * m))
        return mu_x, mu_u

    # ---- gradients through the box-constrained solve (include/ndlqr.h: ndlqr_SolveBatchBoxAdjoint,
    # ndlqr_BatchBoundGradients)
    def solve_box_adjoint(self, g, alpha=0.0, eps_abs=0.0, eps_rel=0.0, max_iter=0, check_every=0):
        """ndlqr_SolveBatchBoxAdjoint: the adjoint of the active-set system of the last constrained solve for g = dL/dz*
        [batch, nvars] (numpy array or DeviceArray), on the forward's kept shifted factorisation (its final penalties, a cold start;
        0 = the library's default for every setting). Returns (iters, status) as numpy int arrays [batch]; status 1 =
        converged, 2 = max_iter reached, 3 = not finite (or the forward's was), 4 = the forward certified the problem
        infeasible (not iterated: w = 0, zero gradients). Raises on a nonzero return. Afterwards
        adjoint() and gradients() read its w."""
        return self._admm_solve("ndlqr_SolveBatchBoxAdjoint", (0.0, alpha, eps_abs, eps_rel, int(max_iter), int(check_every), 0),
                                _doubles(g))

    def bound_gradients(self, summed=False, out=None):
        """ndlqr_BatchBoundGradients: dict with keys xlo, xhi, ulo, uhi -> dL/d(bound) of the last box adjoint, [batch, N, n]
        / [batch, N, m], or [N, n] / [N, m] summed over the batch (NDLQR_BOUNDS_SHARED). `out`: dict of destinations
        (numpy arrays or DeviceArrays); only those keys are computed. Default: numpy arrays for all four."""
        n, m, N, B = self.n, self.m, self.N, self.batch
        shapes = {k: ((N, w) if summed else (B, N, w)) for k, w in (("xlo", n), ("xhi", n), ("ulo", m), ("uhi", m))}
        return self._named_gradients("ndlqr_BatchBoundGradients", shapes, out, BOUNDS_SHARED if summed else 0, True, "bound")

    # ---- active-set polish (include/ndlqr.h: ndlqr_PolishBatchBoxConstrained)
    def polish_box(self, sigma=0.0, max_steps=0, max_rounds=0, steps=None, status=None):
        """ndlqr_PolishBatchBoxConstrained on the latest constrained solve (0 = the library's default for every setting).
        Returns (steps, status) as numpy int arrays [batch] (or the DeviceArray-like destinations given); status 1 =
        polished, 2 = not polished (the ADMM solution stays), 3 = not finite. Raises on a nonzero return."""
        return self._polish("ndlqr_PolishBatchBoxConstrained", (sigma, int(max_steps), int(max_rounds)), steps, status)

    def solve_polished_adjoint(self, g, max_steps=0, steps=None, status=None):
        """ndlqr_SolveBatchPolishedAdjoint: the adjoint of the polished active-set system for g = dL/dz* [batch, nvars]
        (numpy array or DeviceArray) on the polish's factorisation. Returns (steps, status); status 1 = solved, 2 / 3 = the
        polish status of a problem that was not polished (its w and nu are 0), or 2 = no step accepted. Raises on a nonzero
        return. Afterwards adjoint(), gradients() and bound_gradients() read its w and nu."""
        return self._polish("ndlqr_SolveBatchPolishedAdjoint", (0.0, int(max_steps), 0), steps, status, _doubles(g))

    def polish_codes(self):
        """developer / test hook: entry codes [batch, N, n+m] of the latest polish (0 unbounded, 1 free, 2 at the lower bound, 3 at the upper)"""
        return self._copy_out("ndlqr_hip_download_polish_codes", (self.batch, self.N, self.n + self.m), np.uint8, via_ctx=True)

    def factor_count(self):
        """factorisations this solver has launched (ndlqr_hip_factor_count; tests of the kept shifted factorisation)"""
        return int(self.L.ndlqr_hip_factor_count(self.ctx))

    def solutions_to_device(self, device_ptr):
        """[batch][nvars] packed solutions into device memory (asynchronous on the solver's stream)."""
        self._call("ndlqr_CopyBatchSolutionsDevice", self.h, C.c_void_p(int(device_ptr)), detail=False, ok=(self.nvars,))

    def upload_packed(self, AB, QR, rhs):
        """Raw H2D of inputs already in the device layout of include/ndlqr_hip.h (whole batch)."""
        self._call("ndlqr_hip_upload_inputs", self.ctx, 0, self.batch, _ptr(AB), _ptr(QR), _ptr(rhs), detail=False)

    def factors(self, p):
        if self.N & (self.N - 1):
            # (a padded horizon: the factor array is that of the device's tree, which the library does not hand out)
            raise RuntimeError("ndlqr_CopyBatchFactors: not available for a padded horizon (horizon %d is no power of two)"
                               % self.N)
        K = int(np.log2(self.N))
        out = np.zeros(self.N * K * (2 * self.n + self.m) * self.n)
        self._call("ndlqr_CopyBatchFactors", self.h, p, _ptr(out), detail=False)
        return out

    def cholesky_failures(self):
        return self.L.ndlqr_BatchCholeskyFailures(self.h)

    def cholesky_failure_counts(self):
        """int32 [batch]: how often the device flagged each problem. The words are the device's own, cumulative since the
        solver was created (or since the recovery of a solve that did not complete zeroed them): the failures of one solve
        are the difference between two calls."""
        out = np.zeros(self.batch, dtype=np.int32)
        self._call("ndlqr_CopyBatchCholeskyFailureCounts", self.h, _int_ptr(out, self.batch), detail=False)
        return out

    def profile(self):
        """{kernel name: (total ms, launches)} accumulated since the last reset."""
        out = {}
        for slot in range(self.L.ndlqr_hip_profile_slots(self.ctx)):
            name = C.create_string_buffer(64)
            ms, cnt = C.c_double(0), C.c_int(0)
            self.L.ndlqr_hip_profile_get(self.ctx, slot, name, 64, C.byref(ms), C.byref(cnt))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

    def schedule(self):
        """Name of the launch sequence the last solve used."""
        return self.L.ndlqr_hip_schedule(self.ctx).decode()

    def compact_level1(self):
        """True when the last solve kept only the packed Cholesky factor of the level-1 separators (NDLQR_COMPACT1)."""
        return hasattr(self.L, "ndlqr_hip_compact_level1") and bool(self.L.ndlqr_hip_compact_level1(self.ctx))

    def level1_paired(self):
        """True when the fused bottom launch of the last solve ran one Cholesky pass for the two level-1 separators of a
        workgroup (NDLQR_PAIR1)."""
        return hasattr(self.L, "ndlqr_hip_level1_paired") and bool(self.L.ndlqr_hip_level1_paired(self.ctx))

    def bottom_lds16(self):
        """True when that paired launch of the last solve ran in its 16 KB LDS layout (NDLQR_BOTTOM_LDS16); False: not
        applied."""
        return hasattr(self.L, "ndlqr_hip_bottom_lds16") and bool(self.L.ndlqr_hip_bottom_lds16(self.ctx))

    def set_pipeline_depth(self, depth):
        """1: stream-ordered solves; 2: consecutive asynchronous solves alternate between two buffer sets."""
        return self.L.ndlqr_hip_set_pipeline_depth(self.ctx, depth)

    def pipeline_depth(self):
        return self.L.ndlqr_hip_pipeline_depth(self.ctx)

    def profile_reset(self):
        self.L.ndlqr_hip_profile_reset(self.ctx)
