/*
 * ndlqr.h -- public C API of the MI355X-native nested-dissection LQR solver.
 *
 * Drop-in boundary for the `ndlqr_*` API of bjack205/rsLQR. Every declaration below names the
 * reference interface it replaces (file:line under /root/reference/src). Struct layouts of the
 * caller-visible types are kept field-for-field (callers poke at them directly, e.g.
 * `solver->soln->data`, `solver->nvars`, `solver->num_threads`, `solver->profile`).
 * One header carries the whole API; the per-module header names of the reference
 * (solver.h, solve.h, nested_dissection.h, ...) exist next to this file as one-line forwards.
 *
 * Where the work happens: everything numerical (leaf solves, separator inner products,
 * Cholesky, triangular solves, Schur updates, the dense Matrix* helpers) runs on the GPU
 * through the C-ABI shim declared in ndlqr_hip.h. There is no CPU fallback: with no HIP
 * device these entry points return NDLQR_ERR_NO_DEVICE (-2) and print to stderr.
 */
#ifndef NDLQR_H_
#define NDLQR_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h> /* (the reference's nested_dissection.h:15 pulls it in; callers rely on that: test/parallel_test.c:120) */

#ifdef __cplusplus
extern "C" {
#endif

#define NDLQR_OK 0
#define NDLQR_ERR_INVALID (-1)   /* reference convention: -1 on NULL / bad argument */
#define NDLQR_ERR_NO_DEVICE (-2) /* additive: no usable HIP device / HIP runtime error */
#define NDLQR_ERR_NOT_SPD (-3)   /* additive: a Cholesky pivot or a weight was not positive and finite on the device */

/* ------------------------------------------------------------------ matrix.h:71-75 */
typedef struct {
  int rows;
  int cols;
  double* data; /* column-major */
} Matrix;

Matrix NewMatrix(int rows, int cols);                       /* matrix.h:84 */
int MatrixSetConst(Matrix* mat, double val);                /* matrix.h:93 */
int FreeMatrix(Matrix* mat);                                /* matrix.h:104 */
int MatrixNumElements(const Matrix* mat);                   /* matrix.h:113 */
int MatrixGetLinearIndex(const Matrix* mat, int row, int col);
double* MatrixGetElement(const Matrix* mat, int row, int col);
double* MatrixGetElementTranspose(const Matrix* mat, int row, int col, bool istranposed);
int MatrixSetElement(Matrix* mat, int row, int col, double val);
int MatrixCopy(Matrix* dest, Matrix* src);
int MatrixCopyTranspose(Matrix* dest, Matrix* src);
int MatrixScaleByConst(Matrix* mat, double alpha);
double MatrixNormedDifference(Matrix* A, Matrix* B);
int MatrixFlatten(Matrix* mat);
int MatrixFlattenToRow(Matrix* mat);
int PrintMatrix(const Matrix* mat);
int PrintRowVector(const Matrix* mat);

/* ------------------------------------------------------------------ linalg.h:53-153 */
typedef struct {
  char uplo;    /* 'L' */
  int success;  /* 0 = factorisation succeeded */
  char lib;     /* 'H' = HIP device backend (reference: 'B','E','I') */
  void* fact;   /* unused (Eigen-only in the reference) */
  int is_freed;
} CholeskyInfo;

/* Backend selectors of the reference's header (src/linalg.h:17-39; callers print them,
 * test/sample_problem_test.c:172): none of its CPU backends exists here. */
static const int kUseMKL = 0;
static const int kUseEigen = 0;
static const int kUseClap = 0;
static const int kUseBLAS = 0;

enum MatrixLinearAlgebraLibrary { libBLAS = 0, libMKL = 1, libEigen = 2, libInternal = 3, libHIP = 4 };

CholeskyInfo DefaultCholeskyInfo(void);
void FreeFactorization(CholeskyInfo* cholinfo);
/* Dense helpers (linalg.h:83-153). Device-backed: operands are staged to HBM, the kernel of
 * ndlqr_hip.h runs, results are copied back. Meant for tests and small glue, not hot loops. */
int MatrixAddition(Matrix* A, Matrix* B, double alpha);
int MatrixCholeskyFactorize(Matrix* mat);
int MatrixCholeskyFactorizeWithInfo(Matrix* mat, CholeskyInfo* cholinfo);
int MatrixCholeskySolve(Matrix* A, Matrix* b);
int MatrixCholeskySolveWithInfo(Matrix* A, Matrix* b, CholeskyInfo* cholinfo);
void MatrixMultiply(Matrix* A, Matrix* B, Matrix* C, bool tA, bool tB, double alpha, double beta);
void MatrixSymmetricMultiply(Matrix* Asym, Matrix* B, Matrix* C, double alpha, double beta);
void MatrixCopyDiagonal(Matrix* dest, Matrix* src);
enum MatrixLinearAlgebraLibrary MatrixGetLinearAlgebraLibrary(void);
void MatrixPrintLinearAlgebraLibrary(void);
/* The names of the reference's internal backend (src/linalg_custom.h:44-159; its tests call them directly,
 * test/linalg_custom_test.c:11-208). Same argument meaning and return codes, same device kernels as the
 * Matrix* functions above. */
static const int clap_kCholeskySuccess = 0;
static const int clap_kCholeskyFail = -1;
int clap_MatrixAddition(Matrix* A, Matrix* B, double alpha);                 /* B += alpha A */
int clap_MatrixScale(Matrix* A, double alpha);                               /* A *= alpha */
int clap_MatrixMultiply(Matrix* A, Matrix* B, Matrix* C, bool tA, bool tB, double alpha, double beta);
int clap_MatrixTransposeMultiply(Matrix* A, Matrix* B, Matrix* C);           /* C = A' B */
int clap_SymmetricMatrixMultiply(Matrix* Asym, Matrix* B, Matrix* C, double alpha, double beta);
int clap_AddDiagonal(Matrix* A, double alpha);                               /* A += alpha I */
int clap_CholeskyFactorize(Matrix* A);                                       /* lower, in place; -1: pivot <= 0 */
int clap_CholeskySolve(Matrix* L, Matrix* b);                                /* b <- (L L')^-1 b */
int clap_LowerTriBackSub(Matrix* L, Matrix* b, bool istransposed);           /* b <- L^-1 b or L^-T b */

/* ------------------------------------------------------------------ utils.h / linalg_utils.h */
bool IsPowerOfTwo(int x);
static inline int PowerOfTwo(int x) { return 1 << x; }
int LogOfTwo(int x);
int ReadFile(const char* filename, char** out, int* len);
void MatrixLinAlgTimeStart(void);
void MatrixLinAlgTimeStop(void);
void MatrixLinAlgTimeReset(void);
double MatrixGetLinAlgTimeMilliseconds(void);

/* ------------------------------------------------------------------ lqr_data.h:54-132 */
/* One knot point: 0.5 x'Qx + q'x + 0.5 u'Ru + r'u + c ;  x+ = Ax + Bu + d.
 * Q and R are DIAGONALS (n and m entries). A (n x n), B (n x m) column-major.
 * Q is the base pointer of one allocation [Q R q r c A B d] (lqr_data.c:24-49). */
typedef struct {
  int nstates;
  int ninputs;
  double* Q;
  double* R;
  double* q;
  double* r;
  double* c;
  double* A;
  double* B;
  double* d;
} LQRData;

int ndlqr_InitializeLQRData(LQRData* lqrdata, double* Q, double* R, double* q, double* r,
                            double c, double* A, double* B, double* d);
LQRData* ndlqr_NewLQRData(int nstates, int ninputs);
int ndlqr_FreeLQRData(LQRData* lqrdata);
int ndlqr_CopyLQRData(LQRData* dest, LQRData* src);
Matrix ndlqr_GetA(LQRData* lqrdata);
Matrix ndlqr_GetB(LQRData* lqrdata);
Matrix ndlqr_Getd(LQRData* lqrdata);
Matrix ndlqr_GetQ(LQRData* lqrdata);
Matrix ndlqr_GetR(LQRData* lqrdata);
Matrix ndlqr_Getq(LQRData* lqrdata);
Matrix ndlqr_Getr(LQRData* lqrdata);
void ndlqr_PrintLQRData(LQRData* lqrdata);

/* ------------------------------------------------------------------ lqr_problem.h:31-68 */
typedef struct {
  int nhorizon;
  double* x0;
  LQRData** lqrdata;
} LQRProblem;

int ndlqr_InitializeLQRProblem(LQRProblem* lqrproblem, double* x0, LQRData** lqrdata);
LQRProblem* ndlqr_NewLQRProblem(int nstates, int ninputs, int nhorizon);
int ndlqr_FreeLQRProblem(LQRProblem* lqrprob);

/* ------------------------------------------------------------------ json_utils.h:46-76 */
/* Own parser (cJSON is not a dependency). 2-D arrays are arrays of columns; "index" is 1-based. */
LQRData* ndlqr_ReadLQRDataJSONFile(const char* filename);
LQRProblem* ndlqr_ReadLQRProblemJSONFile(const char* filename);
Matrix ReadMatrixJSONFile(const char* filename, const char* name);

/* ------------------------------------------------------------------ binary_tree.h:21-69 */
typedef struct {
  int start; /* inclusive */
  int stop;  /* inclusive for left/right_inds, as the reference fills them */
} UnitRange;

typedef struct BinaryNode_s BinaryNode;
struct BinaryNode_s {
  int idx;
  int level;
  int levelidx;
  UnitRange left_inds;
  UnitRange right_inds;
  BinaryNode* parent;
  BinaryNode* left_child;
  BinaryNode* right_child;
};

typedef struct {
  BinaryNode* root;
  BinaryNode* node_list;
  int num_elements;
  int depth;
} OrderedBinaryTree;

OrderedBinaryTree ndlqr_BuildTree(int nhorizon);
int ndlqr_FreeTree(OrderedBinaryTree* tree);
int ndlqr_GetIndexFromLeaf(const OrderedBinaryTree* tree, int leaf, int level);
int ndlqr_GetIndexLevel(const OrderedBinaryTree* tree, int index);
int ndlqr_GetIndexAtLevel(const OrderedBinaryTree* tree, int index, int level);

/* ------------------------------------------------------------------ nddata.h:40-145 */
typedef struct {
  Matrix lambda; /* (n, w) */
  Matrix state;  /* (n, w) */
  Matrix input;  /* (m, w) */
} NdFactor;

typedef struct {
  int nstates;
  int ninputs;
  int nsegments; /* nhorizon - 1 */
  int depth;
  int width;
  double* data;      /* host mirror, reference layout: block (k,level) at (k + N*level)*(2n+m)*w */
  NdFactor* factors;
} NdData;

Matrix ndlqr_GetLambdaFactor(NdFactor* factor);
Matrix ndlqr_GetStateFactor(NdFactor* factor);
Matrix ndlqr_GetInputFactor(NdFactor* factor);
NdData* ndlqr_NewNdData(int nstates, int ninputs, int nhorizon, int width);
int ndlqr_FreeNdData(NdData* nddata);
int ndlqr_GetNdFactor(NdData* nddata, int index, int level, NdFactor** factor);
void ndlqr_ResetNdData(NdData* nddata);

/* ------------------------------------------------------------------ cholesky_factors.h:30-92 */
typedef struct {
  int depth;
  int nhorizon;
  CholeskyInfo* cholinfo;
  int numfacts;
} NdLqrCholeskyFactors;

NdLqrCholeskyFactors* ndlqr_NewCholeskyFactors(int depth, int nhorizon);
int ndlqr_FreeCholeskyFactors(NdLqrCholeskyFactors* cholfacts);
int ndlqr_GetQFactorizon(NdLqrCholeskyFactors* cholfacts, int index, CholeskyInfo** cholfact);
int ndlqr_GetRFactorizon(NdLqrCholeskyFactors* cholfacts, int index, CholeskyInfo** cholfact);
int ndlqr_GetSFactorization(NdLqrCholeskyFactors* cholfacts, int leaf, int level,
                            CholeskyInfo** cholfact);

/* ------------------------------------------------------------------ solver.h:31-226 */
typedef struct {
  double t_total_ms;
  double t_leaves_ms;
  double t_products_ms;  /* device: separator kernels (products + Cholesky + solves fused) */
  double t_cholesky_ms;  /* device: always 0 (fused into the separator kernels) */
  double t_cholsolve_ms; /* device: always 0 (fused into the separator kernels) */
  double t_shur_ms;      /* device: Schur-update kernels + solution sweep */
  int num_threads;
} NdLqrProfile;

NdLqrProfile ndlqr_NewNdLqrProfile(void);
void ndlqr_ResetProfile(NdLqrProfile* prof);
void ndlqr_CopyProfile(NdLqrProfile* dest, NdLqrProfile* src);
void ndlqr_PrintProfile(NdLqrProfile* profile);
void ndlqr_CompareProfile(NdLqrProfile* base, NdLqrProfile* prof);

typedef struct {
  int nstates;
  int ninputs;
  int nhorizon;
  int depth;
  int nvars;
  OrderedBinaryTree tree;
  Matrix* diagonals; /* (nhorizon, 2): dense Q_k, R_k host mirrors */
  NdData* data;      /* host mirror of the KKT coupling blocks */
  NdData* fact;      /* host mirror of the factorisation (filled by ndlqr_SyncFactorsToHost, or by every ndlqr_Solve under ndlqr_SetFactorMirroring) */
  NdData* soln;      /* rhs in, solution out (always synced by ndlqr_Solve) */
  NdLqrCholeskyFactors* cholfacts;
  double solve_time_ms;
  double linalg_time_ms;
  NdLqrProfile profile;
  int num_threads;   /* accepted and reported; irrelevant on the device */
  /* ---- appended (not in the reference) ---- */
  void* device_ctx;  /* opaque: batch-of-1 device solver */
  unsigned device_flags;     /* NDLQR_FLAG_* used by ndlqr_Solve (ndlqr_SetDeviceFlags; default 0) */
  int device_profiling;      /* ndlqr_SetDeviceProfiling: -1 (default) first solve only, 1 every solve, 0 never */
  int device_profiled;       /* a profiled solve has filled the per-kernel buckets of `profile` */
  NdLqrProfile device_split; /* ... which are kept here for the solves that replay the captured graph */
  int mirror_fact;           /* ndlqr_SetFactorMirroring: ndlqr_Solve leaves the factorisation in `fact` like the reference */
} NdLqrSolver;

NdLqrSolver* ndlqr_NewNdLqrSolver(int nstates, int ninputs, int nhorizon);
int ndlqr_FreeNdLqrSolver(NdLqrSolver* solver);
int ndlqr_InitializeWithLQRProblem(const LQRProblem* lqrprob, NdLqrSolver* solver);
void ndlqr_ResetSolver(NdLqrSolver* solver);
void ndlqr_PrintSolveSummary(NdLqrSolver* solver);
int ndlqr_GetNumVars(NdLqrSolver* solver);
int ndlqr_SetNumThreads(NdLqrSolver* solver, int num_threads);
int ndlqr_GetNumThreads(NdLqrSolver* solver);
int ndlqr_PrintSolveProfile(NdLqrSolver* solver);
NdLqrProfile ndlqr_GetProfile(NdLqrSolver* solver);

/* ------------------------------------------------------------------ solve.h:37-72 */
/* Factor + substitute on the device. Returns 0; additionally NDLQR_ERR_NO_DEVICE /
 * NDLQR_ERR_NOT_SPD (the reference always returns 0, solve.c:189). */
int ndlqr_Solve(NdLqrSolver* solver);
Matrix ndlqr_GetSolution(NdLqrSolver* solver);
int ndlqr_CopySolution(NdLqrSolver* solver, double* soln);
/* additive: per-kernel HIP-event profiling of ndlqr_Solve (fills the buckets of solver->profile like the
 * reference's always-on profiler, src/solve.c:15-25,184-188). Default: the FIRST solve of a solver is profiled (eager
 * launches, an event pair per kernel); every later one replays one captured hipGraph -- copies up, launch chain, copy
 * down: a third of the wall time of a small solve -- and reports its own t_total_ms / solve_time_ms beside the
 * per-kernel split of the last profiled solve. on = 1: profile every solve; on = 0: never (buckets stay 0). */
int ndlqr_SetDeviceProfiling(NdLqrSolver* solver, int on);
/* additive: NDLQR_FLAG_* bits ndlqr_Solve runs with (default 0 = fast mode, solution only; the same
 * launch sequence ndlqr_SolveBatch times). NDLQR_FLAG_STRICT_FP reproduces the reference's default
 * build bit for bit, NDLQR_FLAG_KEEP_FACT materialises the factor array during every solve. */
int ndlqr_SetDeviceFlags(NdLqrSolver* solver, unsigned flags);
/* additive: copy the device factorisation into solver->fact->data (reference layout). Without
 * NDLQR_FLAG_KEEP_FACT on the solve the (still resident) problem is factored once more for it. */
int ndlqr_SyncFactorsToHost(NdLqrSolver* solver);
/* additive: on = 1 makes every ndlqr_Solve of this solver end the way the reference's does (src/solve.c:120-131,
 * src/nddata.h:83-93): with the complete factorisation in solver->fact->data -- the solve runs with
 * NDLQR_FLAG_KEEP_FACT and the factor array comes down with the solution (N K (2n+m) n doubles: 1.5 MB at (6,3,256)).
 * Default 0 (solution only; ndlqr_SyncFactorsToHost on demand), or 1 when the environment has
 * NDLQR_SOLVE_MIRRORS_FACT=1 at ndlqr_NewNdLqrSolver -- for callers that read solver->fact behind an unmodified
 * ndlqr_Solve. */
int ndlqr_SetFactorMirroring(NdLqrSolver* solver, int on);

/* ------------------------------------------------------------------ nested_dissection.h:39-147 */
/* Stage functions on the host mirrors; each runs its dense math through the device-backed
 * Matrix* helpers above (tests / debugging; the hot path is ndlqr_Solve / ndlqr_SolveBatch). */
int ndlqr_SolveLeaf(NdLqrSolver* solver, int index);
int ndlqr_SolveLeaves(NdLqrSolver* solver);
int ndlqr_FactorInnerProduct(NdData* data, NdData* fact, int index, int data_level,
                             int fact_level);
int ndlqr_SolveCholeskyFactor(NdData* fact, CholeskyInfo* cholinfo, int index, int level,
                              int upper_level);
bool ndlqr_ShouldCalcLambda(OrderedBinaryTree* tree, int index, int i);
int ndlqr_UpdateShurFactor(NdData* fact, NdData* soln, int index, int i, int level,
                           int upper_level, bool calc_lambda);
int ndlqr_ComputeShurCompliment(NdLqrSolver* solver, int index, int level, int upper_level);

/* ================================================================== additive: batch API */
/*
 * A batch of independent LQR problems of identical (nstates, ninputs, nhorizon) solved in one
 * launch sequence on one GPU (SURVEY.md 8b "New, additive"). ndlqr_Solve == batch of 1.
 *
 * Flat host layout accepted by ndlqr_InitializeBatchFlat, problem p at offset p*stride:
 *   A [batch][N][n*n] column-major, B [batch][N][n*m] column-major,
 *   Q,q,d [batch][N][n], R,r [batch][N][m], x0 [batch][n]
 * (every knot carries every field, like LQRData; A,B,R,r,d of the last knot are unused).
 */
typedef struct NdLqrBatchSolver NdLqrBatchSolver;

#define NDLQR_FLAG_STRICT_FP 1u   /* separate mul/add (no FMA): bit-reproduces the reference's
                                     default build; slower. Default: fused multiply-add. */
#define NDLQR_FLAG_GENERIC 2u     /* force the runtime-sized kernels even when a size-specialised
                                     variant exists (cross-check) */
#define NDLQR_FLAG_PROFILE 4u     /* bracket every kernel with HIP events */
#define NDLQR_FLAG_KEEP_FACT 8u   /* also materialise the complete factor array on the device (what
                                     the reference leaves in solver->fact); needed by
                                     ndlqr_CopyBatchFactors. Off: only the solution is produced. */

#define NDLQR_FLAG_KEEP_RECORDS 16u /* fast mode: keep what a right-hand-side re-solve needs (separator
                                     records + Cholesky factors, ~3.5 KB per knot at (12,4)) without
                                     materialising the factor array: ndlqr_SolveBatchRhsOnly works,
                                     ndlqr_CopyBatchFactors does not. Size-specialised shapes and every
                                     other one up to 128 states; beyond (the knot-based kernels) the factor
                                     array is kept instead, as with NDLQR_FLAG_KEEP_FACT. */
/* Reach of the modes by block size (runtime-sized kernels; the size-specialised instances of
 * rslqr_amd/csrc/small_instances.def support every mode): EVERY mode works for every block size the device memory holds
 * (round 4; tested up to (256,32)). What changes with the size is the speed: the default fast mode and
 * NDLQR_FLAG_KEEP_RECORDS run the separator-only schedule on the matrix cores up to 128 states (n + m + 4 staged columns
 * within the 160 KB of LDS; (128,32) and everything beyond: the knot-based kernels). NDLQR_FLAG_STRICT_FP and
 * NDLQR_FLAG_KEEP_FACT always run the knot-based kernels, whose separator kernel keeps S-bar and the whole right-hand-side
 * panel in LDS up to about 82 states (tile-filling block sizes, n a multiple of 16, up to 112) and in global memory beyond
 * (one scratch pair per level-0 separator, allocated by the first such solve; NDLQR_ERR_INVALID with
 * ndlqr_hip_last_error() = "global scratch ... does not fit" if the device is too small for the batch). The factor-based
 * rhs-only re-solve reads the factor where it lies beyond ~140 states. */

/* The batch solver takes ANY horizon nhorizon >= 2 (the drop-in ndlqr_NewNdLqrSolver keeps the reference's power of two).
 * A horizon that is no power of two runs padded to the next one on the device ("Padded horizon"):
 * decoupled unit knots behind the caller's, which solve to exactly zero, and the caller's last knot as an interior knot
 * with [A | B] = 0, R = 1, r = 0 -- A, B, R, r, d of the last knot are not part of the problem and are never read. Every
 * array of the API keeps the caller's shapes ([batch][nhorizon][..], nvars = (2n+m) nhorizon - m); the padding is exact;
 * a solve costs what the next power of two costs. Carried through: the four initialisers, ndlqr_SolveBatch / ...Async in
 * every flag mode, ndlqr_BatchSetRhsFlat + ndlqr_SolveBatchRhsOnly, ndlqr_BatchStepAsync, the step selection and the
 * slice functions (knots below nhorizon), ndlqr_CopyBatchSolution(s)(Device), ndlqr_BatchKktResiduals,
 * ndlqr_BatchKktResidualVector, ndlqr_SolveBatchAdjoint, ndlqr_CopyBatchAdjoint, ndlqr_BatchGradients,
 * ndlqr_BatchSetBounds, ndlqr_SolveBatchBoxConstrained (fixed and adaptive penalty), ndlqr_CopyBatchBoundMultipliers,
 * ndlqr_CopyBatchBoxPenalties, ndlqr_CopyBatchBoxResiduals, ndlqr_BatchObjective.
 * REFUSED at a padded horizon (NDLQR_ERR_INVALID, ndlqr_hip_last_error() names the horizon): ndlqr_SolveBatchMultiRhs(Slices),
 * ndlqr_RefineBatch(Adjoint), ndlqr_SolveBatchBoxAdjoint, ndlqr_BatchBoundGradients, ndlqr_CopyBatchBoxAdjointResiduals,
 * ndlqr_PolishBatchBoxConstrained, ndlqr_SolveBatchPolishedAdjoint, ndlqr_BatchSetInfeasibilityDetection (every > 0) and
 * its two getters, ndlqr_BatchSetBoxAcceleration (mem > 0) and ndlqr_CopyBatchBoxAcceleration, the ndlqr_BatchTimeShard*
 * functions, ndlqr_CopyBatchFactors, and of ndlqr_hip.h: ndlqr_hip_device_pointers, ndlqr_hip_staged_io,
 * ndlqr_hip_download_rhs_blocks, ndlqr_hip_download_polish_codes. */
NdLqrBatchSolver* ndlqr_NewBatchSolver(int nstates, int ninputs, int nhorizon, int batch,
                                       int device);
int ndlqr_FreeBatchSolver(NdLqrBatchSolver* bs);
int ndlqr_BatchSetFlags(NdLqrBatchSolver* bs, unsigned flags);
unsigned ndlqr_BatchGetFlags(const NdLqrBatchSolver* bs);
int ndlqr_InitializeBatch(NdLqrBatchSolver* bs, const LQRProblem* const* probs, int count);
int ndlqr_InitializeBatchFlat(NdLqrBatchSolver* bs, const double* A, const double* B,
                              const double* Q, const double* R, const double* q,
                              const double* r, const double* d, const double* x0);
/* Same flat layout, but DEVICE pointers (the problem is produced on the GPU): packed by a kernel
 * on the solver's stream, no host round trip. */
int ndlqr_InitializeBatchFlatDevice(NdLqrBatchSolver* bs, const double* dA, const double* dB,
                                    const double* dQ, const double* dR, const double* dq,
                                    const double* dr, const double* dd, const double* dx0);
/* Dense cost matrices and a state-input cross term: per knot the cost
 *   1/2 x'Q x + x'H u + 1/2 u'R u + q'x + r'u,   Q [batch][N][n*n], R [batch][N][m*m], H [batch][N][n*m]
 * column-major like A and B; H may be NULL (no cross term). Only the LOWER triangles of Q and R are read. Needs R_k > 0 and
 * Q_k - H_k R_k^-1 H_k' > 0 (the dense form of Q > 0, R > 0); H, R of the last knot are not part of the problem and, like
 * its A, B, r, d, are never read. Host or device pointers (this device's). The problem is reduced on the device to a
 * unit-cost problem of the same shape, which the solver's kernels solve as they are; every result comes back in the
 * caller's variables. A pivot of the reduction that is not positive is reported like one of the solver's own: the next
 * ndlqr_SolveBatch returns NDLQR_ERR_NOT_SPD and ndlqr_BatchCholeskyFailures counts it.
 * The solver is in dense-cost mode (ndlqr_BatchCostIsDense) until one of the diagonal initialisers above or below is
 * called. CARRIED THROUGH in that mode: ndlqr_SolveBatch and ndlqr_SolveBatchAsync + ndlqr_BatchSynchronize in every flag
 * mode, ndlqr_CopyBatchSolution(s)(Device), ndlqr_BatchSetRhsFlat + ndlqr_SolveBatchRhsOnly, ndlqr_SolveBatchAdjoint +
 * ndlqr_CopyBatchAdjoint + ndlqr_BatchGradientsDense (the nine dense-cost gradients, assembled on the device),
 * ndlqr_BatchCholeskyFailures, ndlqr_BatchSolveTimeMs, ndlqr_BatchObjective (the caller's Q, H, R: the unit-cost
 * objective of the reduced problem is the caller's), any horizon >= 2.
 * REFUSED (NDLQR_ERR_INVALID, ndlqr_hip_last_error() opens with the name of the function of ndlqr_hip.h behind the call):
 * ndlqr_BatchStepAsync, ndlqr_BatchSetStepSelection (a non-empty one), ndlqr_SolveBatchSlicesAsync,
 * ndlqr_CopyBatchSolutionSlices, ndlqr_SolveBatchMultiRhs(Slices), ndlqr_BatchGradients (the dense-cost gradients are
 * ndlqr_BatchGradientsDense's), ndlqr_RefineBatch(Adjoint), ndlqr_BatchKktResiduals,
 * ndlqr_BatchKktResidualVector (their rows are those of the reduced system), ndlqr_BatchSetBounds and every function of the
 * box-constrained solve, the ndlqr_BatchTimeShard* functions, ndlqr_CopyBatchFactors, and of ndlqr_hip.h
 * ndlqr_hip_device_pointers, ndlqr_hip_staged_io / ndlqr_hip_solve_staged, ndlqr_hip_download_rhs_blocks.
 * (The step and the slices of this mode come under names of their own: ndlqr_BatchStepAsyncDense,
 * ndlqr_SolveBatchSlicesAsyncDense, ndlqr_CopyBatchSolutionSlicesDense, below.) */
int ndlqr_InitializeBatchFlatDense(NdLqrBatchSolver* bs, const double* A, const double* B, const double* Q,
                                   const double* H, const double* R, const double* q, const double* r,
                                   const double* d, const double* x0);
int ndlqr_BatchCostIsDense(const NdLqrBatchSolver* bs); /* 1: dense-cost mode, 0: not */
/* General linear inequality constraints: per knot p >= 1 rows
 *   lo_k <= C_k x_k + D_k u_k <= hi_k,   C [batch][N][p*n], D [batch][N][p*m] column-major per knot like A and B,
 * lo, hi [P][N][p] with P = batch, or P = 1 with NDLQR_BOUNDS_SHARED in `flags`. Entries of lo, hi may be +-inf (a row with
 * both infinite is unbounded); D of the last knot is never loaded. The nine arrays before p are those of
 * ndlqr_InitializeBatchFlatDense (a diagonal cost is passed as a dense one); host or device pointers (this device's).
 *   ndlqr_InitializeBatchFlatConstrained puts the solver into dense-cost mode exactly as the dense initialiser does --
 *   ndlqr_SolveBatch, ndlqr_BatchSetRhsFlat + ndlqr_SolveBatchRhsOnly and ndlqr_SolveBatchAdjoint work as there and give the
 *   UNCONSTRAINED answers -- and retains A, B, Q, H, R, the right-hand side, C and D on the device (constrained mode,
 *   ndlqr_BatchIsConstrained). Every other initialiser leaves constrained mode.
 *   ndlqr_BatchSetConstraintBounds: new bounds without touching C, D or the factorisation; lo > hi or a NaN is refused
 *   before anything is replaced; a change of WHICH rows are bounded drops the remembered factorisation.
 *   ndlqr_SolveBatchLinConstrained: scaled ADMM on the rows (section 3.9 carried to w = C x + D u) with the fixed penalty
 *   s->rho; the settings rho, alpha, eps_abs, eps_rel, max_iter, check_every, warm_start are those of
 *   ndlqr_SolveBatchBoxConstrained with the same defaults (0, or s == NULL). The cost shifted by rho C'MC, rho C'MD, rho D'MD
 *   (M: the bounded rows) is reduced and factored once -- or not at all while rho, the flags, the inputs and the bounded
 *   pattern stay as they were (ndlqr_BatchSetRhsFlat keeps them) --, every iteration is one re-solve and one update
 *   kernel. iters / status [batch] (may be NULL): status 1 converged, 2 max_iter reached, 3 not finite, 4 certified
 *   infeasible (only with ndlqr_BatchSetConstraintInfeasibilityDetection, below). The solution that
 *   ndlqr_CopyBatchSolution(s) delivers afterwards is [lambda, x, u] of the last re-solve: the dynamics hold exactly, the
 *   rows hold to within r_prim. A plain solve afterwards gives what it gave before, bit for bit.
 *   ndlqr_BatchSetConstraintPenaltyAdaptation: every > 0 gives the constrained solves that follow
 *   the per-problem adaptive penalty of the box solve (section 3.11): at the iterations it % every == 0, it < max_iter,
 *   every running problem may move its penalty by a power of two within [rho_min, rho_max] (0: the library's 1e-6 and
 *   1e6) from its own residuals, keeping mu = rho y; the whole batch is then shifted, reduced and factored again, at most
 *   once per such iteration. every = 0, the initial state: off. Negative values or rho_min > rho_max return
 *   NDLQR_ERR_INVALID and the previous setting stays. The setting belongs to the solver: allowed in any mode, kept
 *   across initialisers. With it on, s->rho is the start of a cold solve; a solve with warm_start on a remembered
 *   factorisation starts from the penalties the previous one ended with, factors nothing and ignores s->rho. A solve
 *   with adaptation off reuses a remembered factorisation only while all its penalties are s->rho.
 *   ndlqr_CopyBatchConstraintPenalties: rho [batch] of the latest constrained solve (host or this device's memory);
 *   refused by name before a constrained solve.
 *   ndlqr_BatchSetConstraintInfeasibilityDetection: every > 0 lets the constrained solves that
 *   follow test every running problem, at the iterations it >= 2 with it % every == 0 and it <= max_iter, for a Farkas
 *   certificate that the dynamics and the rows have no common point: with dlam, dmu the differences of the multipliers
 *   (in the caller's variables) and of mu = rho y over that iteration, D = max |dmu|,
 *     e_x,k = -dlam_k + A_k' dlam_(k+1) + C_k' dmu_k,  e_u,k = B_k' dlam_(k+1) + D_k' dmu_k  (last knot: -dlam + C' dmu only),
 *     S = sum over bounded rows (hi max(dmu, 0) + lo min(dmu, 0)) - x0' dlam_0 - sum_k d_k' dlam_(k+1),
 *   a problem is certified when D > 0, max |e| <= eps D, S < -eps D, every dmu pointing to an infinite bound is at most
 *   eps D, and all of them are finite (a NaN never certifies). It then ends as status 4 with iters = that iteration, frozen
 *   like a converged one; its delivered solution is its last iterate (the dynamics hold, the rows do not), the batch ends
 *   when every problem is 1, 3 or 4. every = 0, the initial state: off -- nothing is allocated, copied or launched. eps = 0:
 *   1e-4. every < 0, or eps negative or not finite, returns NDLQR_ERR_INVALID and the previous setting stays. The setting
 *   belongs to the solver: allowed in any mode and for any horizon, kept across initialisers; it is this solve's own --
 *   ndlqr_BatchSetInfeasibilityDetection stays the box solve's. A warm-started solve starts a problem that ended as 4
 *   cold; ndlqr_SolveBatchLinAdjoint does not iterate it (w = 0, nu = 0, every gradient of it zero).
 *   ndlqr_CopyBatchConstraintInfeasibilityCertificate: dlam [batch][N][n], dmu [batch][N][p] of the problems that ended as
 *   4, zero rows for the others; either may be NULL, not both. ndlqr_CopyBatchConstraintInfeasibilityMeasures: measures
 *   [batch][4] = max |e| | D | the largest |dmu| toward an infinite bound | S of every problem's latest check and
 *   iteration [batch], the iteration it ran at (0: never examined); either may be NULL, not both. Host or this device's
 *   memory. Both refuse by name unless the resident solution is that of the latest constrained solve and detection was on
 *   for it, and outside constrained mode.
 *   ndlqr_CopyBatchConstraintMultipliers: mu = rho y, [batch][N][p] (mu > 0 at an upper, < 0 at a lower bound).
 *   ndlqr_CopyBatchConstraintResiduals: [batch][4] = r_prim | r_dual | sp | sd of every problem's last update, with the
 *   meaning of ndlqr_CopyBatchBoxResiduals: r_prim = max |w - v|, r_dual = rho max |[C D]'(v - v_prev)|,
 *   sp = max(max |w|, max |v|), sd = rho max |[C D]' y|.
 *   ndlqr_BatchObjective is carried through: after a constrained solve or its polish the caller's unshifted cost at the
 *   delivered iterate (from the retained Q, H, R, q, r), after a plain solve the unconstrained optimal value.
 * REFUSED by name (NDLQR_ERR_INVALID, ndlqr_hip_last_error()): s->adapt_every > 0 (that field, with rho_min and rho_max, is
 * the box solve's: ndlqr_BatchSetConstraintPenaltyAdaptation is this solve's switch); everything of the box
 * solve -- acceleration, its infeasibility detection (ndlqr_BatchSetInfeasibilityDetection and its two read-outs: this
 * solve has ndlqr_BatchSetConstraintInfeasibilityDetection), its polish (this solve has ndlqr_PolishBatchLinConstrained,
 * below), box adjoint and bound gradients -- as in dense-cost mode;
 * ndlqr_BatchStepAsync. ndlqr_SolveBatchAdjoint refuses after a constrained solve: its adjoint is
 * ndlqr_SolveBatchLinAdjoint (below). */
int ndlqr_InitializeBatchFlatConstrained(NdLqrBatchSolver* bs, const double* A, const double* B, const double* Q,
                                         const double* H, const double* R, const double* q, const double* r,
                                         const double* d, const double* x0, int p, const double* C, const double* D,
                                         const double* lo, const double* hi, unsigned flags);
int ndlqr_BatchIsConstrained(const NdLqrBatchSolver* bs); /* 1: constrained mode, 0: not */
int ndlqr_BatchSetConstraintBounds(NdLqrBatchSolver* bs, const double* lo, const double* hi, unsigned flags);
/* Seeded synthetic problems, problem p seeded with seed0 + p; generated on the
 * host, packed and uploaded. */
int ndlqr_InitializeBatchSynthetic(NdLqrBatchSolver* bs, uint64_t seed0);
int ndlqr_SolveBatch(NdLqrBatchSolver* bs);      /* launch + wait */
/* Factor / solve split (MPC re-solves): replace q, r, d, x0 (flat layout as above) and run only
 * the solution sweep against the factorisation cached by the last ndlqr_SolveBatch; needs
 * NDLQR_FLAG_KEEP_FACT (or, in fast mode up to 128 states, the lighter
 * NDLQR_FLAG_KEEP_RECORDS) to have been set for that solve. A, B, Q, R are those of that solve. */
int ndlqr_BatchSetRhsFlat(NdLqrBatchSolver* bs, const double* q, const double* r, const double* d,
                          const double* x0);
int ndlqr_SolveBatchRhsOnly(NdLqrBatchSolver* bs);
/* additive: nrhs sets of right-hand sides for the whole batch against the factorisation kept by the last ndlqr_SolveBatch
 * with NDLQR_FLAG_KEEP_RECORDS -- q, d [nrhs][batch][N][n], r [nrhs][batch][N][m], x0 [nrhs][batch][n] (the flat layout above
 * with a leading [nrhs]) in, solutions [nrhs][batch][nvars] out (host arrays; blocking). The reference solves one
 * right-hand side per factorisation (src/nddata.h:70-75); here e.g. ONE problem of (12,4,256) takes 1024 right-hand sides
 * (sampled initial states / cost offsets of one model) at the rate its right-hand sides and solutions move through the
 * HBM. Size-specialised shapes on the level-per-launch schedule (batch x N / 4 > 2048, or NDLQR_TREE=0 in the environment). */
int ndlqr_SolveBatchMultiRhs(NdLqrBatchSolver* bs, int nrhs, const double* q, const double* r, const double* d,
                             const double* x0, double* soln);
/* The same for a slice of every solution -- knots [knot0, knot0 + nknots), blocks = NDLQR_SOLN_* (below) ->
 * out [nrhs][batch][nknots][width]; only those knots are computed by the last launch and brought down. */
int ndlqr_SolveBatchMultiRhsSlices(NdLqrBatchSolver* bs, int nrhs, const double* q, const double* r, const double* d,
                                   const double* x0, int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_SolveBatchAsync(NdLqrBatchSolver* bs); /* enqueue on the solver's stream */
int ndlqr_BatchSynchronize(NdLqrBatchSolver* bs);
/* One MPC step, asynchronous: new q, r, d, x0 (flat host layout as above) up, factor + solve against the resident
 * A, B, Q, R, the solutions [batch][nvars] down into `soln` (the array ndlqr_CopyBatchSolutions fills); q, r, d may each
 * be NULL: that part of the right-hand side stays what its most recent writer -- ndlqr_InitializeBatch*,
 * ndlqr_BatchSetRhsFlat or an earlier step -- left (an MPC iteration often replaces x0 alone; full steps and x0-only
 * steps may be mixed freely: the library keeps track of which buffer set's copy is behind in what). Consecutive
 * steps alternate between the two buffer sets of the solve pipeline, so the transfers of one step run beside the
 * kernels of the other; `soln` of a step is complete after ndlqr_BatchSynchronize, or -- one step behind --
 * ndlqr_BatchSynchronizePrevious. Host arrays from ndlqr_HostAlloc (pinned) keep the copies asynchronous;
 * pageable memory works but blocks. What the reference does per MPC iteration with ndlqr_ResetSolver +
 * ndlqr_InitializeWithLQRProblem + ndlqr_Solve + ndlqr_CopySolution (src/solve.h:20-32).
 * With NDLQR_FLAG_KEEP_RECORDS (size-specialised shapes on the level-per-launch schedule): a step never changes A, B, Q,
 * R, so the first step factors and every further one is the right-hand-side re-solve on the kept records -- 0.51 instead
 * of 0.68 ms per step of 1024 x (12,4,256) with x0 up and u of knot 0 down -- until new inputs are uploaded; the steps
 * are then stream-ordered on one buffer set (results equal a full solve's to rounding, not bit for bit). */
int ndlqr_BatchStepAsync(NdLqrBatchSolver* bs, const double* q, const double* r, const double* d,
                         const double* x0, double* soln);
/* Waits for the step before the most recent one; NDLQR_ERR_NOT_SPD when a Cholesky pivot of that step (or an earlier,
 * unreported one) was not positive -- its `soln` is then not a solution. */
int ndlqr_BatchSynchronizePrevious(NdLqrBatchSolver* bs);
/* What a step brings down: knots [knot0, knot0 + nknots) of every problem, of each knot the blocks of `blocks`, in
 * the reference's order lambda, state, input -> soln = [batch][nknots][width], width = n per NDLQR_SOLN_LAMBDA /
 * NDLQR_SOLN_STATE + m for NDLQR_SOLN_INPUT. nknots = 0: back to every solution [batch][nvars] (the default; what
 * ndlqr_CopySolution hands back, src/solve.c:192-201). An MPC loop that applies u_0 asks for (0, 1, NDLQR_SOLN_INPUT):
 * 32 KB instead of 59 MB per 1024 problems of (12,4,256). ndlqr_CopyBatchSolutionSlices: the same slice of the most
 * recent solve, synchronously.
 * NDLQR_SOLN_ONLY (or-ed into `blocks`): the caller wants NOTHING but the selection, so a step may skip the part of the
 * back-substitution that produces the other knots -- (0, 1, NDLQR_SOLN_INPUT | NDLQR_SOLN_ONLY) is the MPC step that
 * computes u_0 alone: the forward pass over the whole horizon, the top-down sweep, and the eight knots around knot 0
 * instead of all N (0.63 -> 0.43 ms per 1024 x (12,4,256), 0.48 -> 0.30 with NDLQR_FLAG_KEEP_RECORDS). After such a step
 * the solver holds only that slice: ndlqr_CopyBatchSolutionSlices inside it works, everything that needs the whole
 * vector (ndlqr_CopyBatchSolution(s), ndlqr_BatchKKTResidual, the device-side pack) returns -1 until the next solve or
 * step without the bit. ((64,16,512) x 256: 11.6 -> 9.4 ms, 8.0 -> 5.5 with NDLQR_FLAG_KEEP_RECORDS.) The knot-based
 * kernels (strict mode, KEEP_FACT, beyond 128 states) compute everything regardless. */
#define NDLQR_SOLN_LAMBDA 1u
#define NDLQR_SOLN_STATE 2u
#define NDLQR_SOLN_INPUT 4u
#define NDLQR_SOLN_ONLY 8u
int ndlqr_BatchSetStepSelection(NdLqrBatchSolver* bs, int knot0, int nknots, unsigned blocks);
/* The same economy for a loop that replaces A, B, Q, R too (ndlqr_InitializeBatchFlat[Device] per iteration): factor +
 * solve of the resident problems, computing and delivering knots [knot0, knot0 + nknots) alone -- out =
 * [batch][nknots][width] in host, pinned or device memory; asynchronous like ndlqr_SolveBatchAsync (complete after
 * ndlqr_BatchSynchronize), and like a step with NDLQR_SOLN_ONLY it leaves nothing but that slice behind. */
int ndlqr_SolveBatchSlicesAsync(NdLqrBatchSolver* bs, int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_CopyBatchSolutionSlices(NdLqrBatchSolver* bs, int knot0, int nknots, unsigned blocks, double* out);
/* The MPC step and the slices of a DENSE-COST problem (ndlqr_InitializeBatchFlatDense), everything in the caller's
 * variables. ndlqr_BatchStepAsyncDense is ndlqr_BatchStepAsync for that mode: the right-hand side up, factor + solve (the
 * re-solve on kept records under NDLQR_FLAG_KEEP_RECORDS), the solutions down, asynchronously, two steps in flight, the
 * same memories (pinned, pageable -- which blocks --, the solver's device), ndlqr_BatchSynchronize(Previous) as for the
 * plain step. x0 and out are required; q and r are replaced TOGETHER or not at all (the reduced q needs both); d may be
 * NULL. What comes down is an argument, not the selection of ndlqr_BatchSetStepSelection: knots [knot0, knot0 + nknots),
 * blocks = NDLQR_SOLN_* -> out [batch][nknots][width] (u of the last knot: zero), or with nknots == 0 every solution
 * [batch][nvars]. An x0-only step for (0, 1, NDLQR_SOLN_INPUT | NDLQR_SOLN_ONLY) touches one knot per problem on the way up
 * and one on the way down. ndlqr_SolveBatchSlicesAsyncDense / ndlqr_CopyBatchSolutionSlicesDense: the dense-cost forms of
 * the two slice functions above. Each of the three refuses by name (NDLQR_ERR_INVALID; ndlqr_hip_last_error() opens with
 * the name of the function of ndlqr_hip.h behind it) outside dense-cost mode, in constrained mode, and for q without r. */
int ndlqr_BatchStepAsyncDense(NdLqrBatchSolver* bs, const double* q, const double* r, const double* d, const double* x0,
                              int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_SolveBatchSlicesAsyncDense(NdLqrBatchSolver* bs, int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_CopyBatchSolutionSlicesDense(NdLqrBatchSolver* bs, int knot0, int nknots, unsigned blocks, double* out);
/* Time-axis sharding: one problem (or a small batch) over G ranks, rank g on knots [g N / G, (g + 1) N / G) -- for jobs
 * with fewer problems than GPUs (details and limits: ndlqr_hip.h). Per solve, on every rank:
 * Factor -> ExportTop(buf) -> sum buf over the ranks -> ImportTop(buf) -> Finish -> ndlqr_BatchSynchronize. */
int ndlqr_BatchTimeShardTopDoubles(NdLqrBatchSolver* bs, int G);
int ndlqr_BatchTimeShardFactor(NdLqrBatchSolver* bs, int g, int G);
int ndlqr_BatchTimeShardExportTop(NdLqrBatchSolver* bs, int G, double* buf);
int ndlqr_BatchTimeShardImportTop(NdLqrBatchSolver* bs, int G, const double* buf);
int ndlqr_BatchTimeShardFinish(NdLqrBatchSolver* bs, int g, int G);
void* ndlqr_HostAlloc(size_t bytes); /* pinned host memory (NULL: no device / no memory) */
void ndlqr_HostFree(void* p);
/* Device memory, for loops that live on the GPU: ndlqr_BatchStepAsync takes q, r, d, x0 and soln in the solver's device
 * memory as they are (no transfer at all; any mix with host pointers works). ndlqr_DeviceCopy: synchronous, any direction. */
void* ndlqr_DeviceAlloc(size_t bytes);
void ndlqr_DeviceFree(void* p);
int ndlqr_DeviceCopy(void* dst, const void* src, size_t bytes);
int ndlqr_BatchNumVars(const NdLqrBatchSolver* bs);
int ndlqr_BatchSize(const NdLqrBatchSolver* bs);
int ndlqr_CopyBatchSolution(NdLqrBatchSolver* bs, int p, double* soln);    /* nvars doubles */
int ndlqr_CopyBatchSolutions(NdLqrBatchSolver* bs, double* soln);          /* batch*nvars */
/* the same [batch][nvars] array written to DEVICE memory by a kernel on the solver's stream
 * (asynchronous; e.g. the send buffer of an all_gather of the shards' solutions) */
int ndlqr_CopyBatchSolutionsDevice(NdLqrBatchSolver* bs, double* dsoln);
int ndlqr_CopyBatchFactors(NdLqrBatchSolver* bs, int p, double* fact);     /* reference layout */
int ndlqr_BatchCholeskyFailures(NdLqrBatchSolver* bs);
/* Which members failed: counts[b], b = 0 .. batch - 1, is the number of times the device flagged problem b (a block of
 * the top chain, one launch that stands for several tree levels, adds one count per level it stands for). The words
 * are cumulative since the solver was created (ndlqr_hip.h: ndlqr_hip_download_failure_counts), so the failures of one
 * solve are the difference between the counts after and before it; their sum over the batch grows by what
 * ndlqr_BatchCholeskyFailures reports for that solve. Waits for everything in flight. */
int ndlqr_CopyBatchCholeskyFailureCounts(NdLqrBatchSolver* bs, int* counts);
/* KKT residual ||K z - b||_2 and ||b||_2 of every problem's resident solution against its raw
 * data, evaluated on the device (batch doubles each; bnorm may be NULL). */
int ndlqr_BatchKktResiduals(NdLqrBatchSolver* bs, double* res, double* bnorm);
double ndlqr_BatchSolveTimeMs(const NdLqrBatchSolver* bs); /* HIP-event time of last solve */
/* additive: adjoint solve and parameter gradients (differentiable MPC, system identification). For a loss L(z) of the
 * resident solutions z and g = dL/dz ([batch][nvars], the packing of ndlqr_CopyBatchSolutions; host, pinned or the
 * solver's device memory), ndlqr_SolveBatchAdjoint solves K w = g against the kept factorisation (K is symmetric) and
 * ndlqr_BatchGradients assembles dL/d(A, B, Q, R, q, r, d, x0) from z and w on the device, in the flat layout of
 * ndlqr_InitializeBatchFlat (A, B column-major; Q, R diagonals; zero for A, B, R, r, d of the last knot).
 *   Reach: wherever ndlqr_SolveBatchRhsOnly works -- a solve with NDLQR_FLAG_KEEP_RECORDS (fast mode) or
 *   NDLQR_FLAG_KEEP_FACT (any mode; with NDLQR_FLAG_STRICT_FP the gradients are bit-reproducible from z and w).
 *   The primal state stays as it is: solutions, right-hand side, kept records and factors; a later
 *   ndlqr_CopyBatchSolutions, ndlqr_BatchKktResiduals, ndlqr_SolveBatchRhsOnly or step behaves as if the adjoint had
 *   never run. Any later solve, step or re-solve invalidates the adjoint, as does the upload of new inputs;
 *   ndlqr_BatchGradients / ndlqr_CopyBatchAdjoint then return NDLQR_ERR_INVALID. So do all three after a step that
 *   computed a slice alone (NDLQR_SOLN_ONLY), on a time-axis shard, and for device memory of another device.
 *   Outputs of ndlqr_BatchGradients: NULL = not computed; host or pinned memory (staged through HBM, one copy each) or the
 *   solver's device memory (written by the kernel). Bit o of sum_mask (NDLQR_GRAD_*): output o summed over the batch,
 *   deterministically -- [N][...] ([n] for x0) instead of [batch][N][...], at every block size the solver takes. The one
 *   refusal by size: z and w of two knots beyond the LDS of a workgroup (2n+m > 5120). All three calls block until their
 *   results are complete; ndlqr_BatchSolveTimeMs then reports the device time of the adjoint solve / the gradient kernels. */
#define NDLQR_GRAD_A 1u
#define NDLQR_GRAD_B 2u
#define NDLQR_GRAD_Q 4u
#define NDLQR_GRAD_R 8u
#define NDLQR_GRAD_q 16u
#define NDLQR_GRAD_r 32u
#define NDLQR_GRAD_d 64u
#define NDLQR_GRAD_x0 128u
int ndlqr_SolveBatchAdjoint(NdLqrBatchSolver* bs, const double* g);  /* K w = g against the kept factorisation */
int ndlqr_CopyBatchAdjoint(NdLqrBatchSolver* bs, double* w);         /* [batch][nvars]; returns nvars */
int ndlqr_BatchGradients(NdLqrBatchSolver* bs, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gR,
                         double* gq, double* gr, double* gd, double* gx0);
/* additive: the parameter gradients of dense-cost mode. ndlqr_BatchGradientsDense assembles
 * dL/d(A, B, Q, H, R, q, r, d, x0) on the device from exactly the z and w that ndlqr_CopyBatchSolutions and
 * ndlqr_CopyBatchAdjoint would deliver at that moment (both in the caller's variables), in the flat layout of
 * ndlqr_InitializeBatchFlatDense: gA, gQ [batch][N][n*n], gB, gH [batch][N][n*m], gR [batch][N][m*m], column-major per knot
 * ((i, j) at i + rows*j); gq, gd [batch][N][n], gr [batch][N][m], gx0 [batch][n]. With lam+ = lambda_(k+1), per knot
 *     gA(i,j) = -(w_lam+[i] z_x[j] + z_lam+[i] w_x[j])      gB(i,j) = -(w_lam+[i] z_u[j] + z_lam+[i] w_u[j])
 *     gH(i,j) = -(w_x[i] z_u[j] + z_x[i] w_u[j])
 *     gQ(i,j) = -1/2 (w_x[i] z_x[j] + z_x[i] w_x[j])        gR(i,j) = -1/2 (w_u[i] z_u[j] + z_u[i] w_u[j])
 *     gq = -w_x     gr = -w_u     gd = -w_lam+     gx0 = -w_lam0
 * A, B, H, R, r, d of the last knot are exactly zero. Both triangles of gQ and gR are written and (i,j), (j,i) carry the
 * same bits in every mode: the gradient in the space of symmetric matrices. With NDLQR_FLAG_STRICT_FP every matrix entry is
 * t1 = a*b (the w factor first), t2 = c*e, s = t1 + t2, -s (-0.5*s for Q, R) without contraction: bit-reproducible from z
 * and w; otherwise A, B and H are one fused multiply-add each.
 *   Reach: dense-cost mode after ndlqr_SolveBatchAdjoint (this includes constrained mode after a plain solve and adjoint:
 *   the unconstrained answers), and constrained mode after ndlqr_SolveBatchLinAdjoint of the resident constrained solution,
 *   where w is that of the active-set system and the same formulas hold; there a problem the adjoint did not iterate
 *   (status 3) gets exact zeros in every per-problem output and is left out of the batch sums, as in
 *   ndlqr_BatchConstraintGradients. Any horizon >= 2, every block size dense-cost mode accepts.
 *   Outputs and sum_mask (NDLQR_GRADD_*) as for ndlqr_BatchGradients: NULL = not computed; host, pinned or the solver's
 *   device memory; bit o: output o summed over the batch, deterministically (two calls give the same bits).
 *   Returns NDLQR_ERR_INVALID (ndlqr_hip_last_error() opens with ndlqr_hip_gradients_dense) outside dense-cost mode -- there
 *   ndlqr_BatchGradients is the call --, without an adjoint of the resident solution (any solve, re-solve, new inputs,
 *   ndlqr_BatchSetRhsFlat or ndlqr_BatchSetConstraintBounds since it was taken), for a partial or invalid solution, for mask
 *   bits beyond the ninth and for an output in the memory of another device.
 *   Nothing else moves: the resident solution and adjoint, the kept and remembered factorisations, v, y, mu and the warm
 *   start stay as they are, and nothing is factored. Blocking; ndlqr_BatchSolveTimeMs then reports the device time of the
 *   gradient kernels (the packing of z and w included). */
#define NDLQR_GRADD_A 1u
#define NDLQR_GRADD_B 2u
#define NDLQR_GRADD_Q 4u
#define NDLQR_GRADD_H 8u
#define NDLQR_GRADD_R 16u
#define NDLQR_GRADD_q 32u
#define NDLQR_GRADD_r 64u
#define NDLQR_GRADD_d 128u
#define NDLQR_GRADD_x0 256u
int ndlqr_BatchGradientsDense(NdLqrBatchSolver* bs, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gH,
                              double* gR, double* gq, double* gr, double* gd, double* gx0);
/* additive: feedback gains and cost-to-go matrices -- what an MPC loop applies between two solves
 * (u = u_0 + K_0 (x - x_0)), what a TVLQR tracking controller needs of every knot, and what an iLQR / SQP outer loop rolls
 * its line search out with. With P_(N-1) = Q_(N-1), p_(N-1) = q_(N-1), for k = N-2 .. 0 (the reference's Riccati recursion):
 *     g = P_(k+1) d_k + p_(k+1)
 *     M = [A_k | B_k]' P_(k+1) [A_k | B_k] + [[Q_k, H_k], [H_k', R_k]]      (Qxx | Qxu ; Qux | Quu)
 *     v = [q_k ; r_k] + [A_k | B_k]' g                                      (Qx ; Qu)
 *     Quu = L L',  W = L^-1 Qux,  w = L^-1 Qu
 *     K_k = -L^-T W     kff_k = -L^-T w     P_k = Qxx - W' W     p_k = Qx - W' w
 * so that u_k = K_k x_k + kff_k and lambda_k = P_k x_k + p_k on the optimal trajectory, in the signs of the solution vector
 * [lambda x u]. It delivers gains, not solutions: the time-parallel factorisation stays the only solver.
 *   Outputs for the knots [knot0, knot0 + nknots): K [batch][nknots][m*n], kff [batch][nknots][m], P [batch][nknots][n*n],
 *   p [batch][nknots][n]; matrices column-major per knot (K(j,i) at j + m*i). Any of them may be NULL (not computed), not
 *   all four; failures [batch] ints, may be NULL. Host, pinned or the solver's device memory. P is bit-symmetric. If knot
 *   N-1 is in the range its K, kff are exact zeros, its P = diag Q_(N-1) (dense-cost mode: Q_(N-1) as L L' of its factor)
 *   and p = q_(N-1).
 *   Reads the resident inputs and the latest right-hand side (ndlqr_BatchSetRhsFlat and the steps of ndlqr_BatchStepAsync
 *   included); in dense-cost mode it runs on the reduced problem and maps the result back, so the outputs are those of the
 *   caller's Q, H, R. Needs no solve before it and no flag; works in every flag mode (the same bits in all of them), at any
 *   horizon >= 2 and on every block size whose working set fits the LDS of a workgroup. Blocking.
 *   Returns NDLQR_OK; NDLQR_ERR_NOT_SPD if a pivot of some Quu was not > 0 (NaN included): the pivot is taken as 1 and
 *   counted in failures[problem], NOT in the solver's failure counts; all outputs are delivered, finite for finite input,
 *   and every healthy problem's are those of a healthy batch, bit for bit. NDLQR_ERR_INVALID (ndlqr_hip_last_error() opens
 *   with ndlqr_hip_feedback_gains) for a knot range outside [0, N), all outputs NULL, constrained (linear-inequality) mode
 *   -- the resident problem there is the rho-shifted one --, a time-axis shard, a block size beyond the LDS and an output in
 *   the memory of another device.
 *   Nothing else moves: the resident solution and what is known about it, the kept and remembered factorisations, the
 *   failure counts, the box / constraint / polish state stay as they are. ndlqr_BatchSolveTimeMs then reports the device
 *   time of the call's kernels. */
int ndlqr_BatchFeedbackGains(NdLqrBatchSolver* bs, int knot0, int nknots, double* K, double* kff, double* P, double* p,
                             int* failures);
/* additive: the value of the cost every problem minimised, at its resident solution -- what a line
 * search or a trust-region ratio of an iLQR / SQP outer loop divides by, what compares an ADMM iterate with its polish,
 * and the loss of a differentiable MPC layer (rslqr_amd.autograd.lqr_value):
 *     J = sum_{k<N} l_k,   l_k = 1/2 x_k'Q_k x_k + x_k'H_k u_k + 1/2 u_k'R_k u_k + q_k'x_k + r_k'u_k
 * with the last knot contributing 1/2 x'Q x + q'x alone (its H, R, r are never read) and no constant term.
 *   Outputs: J [batch]; stage [batch][nhorizon] = l_k, may be NULL. Host, pinned or the solver's device memory. Every
 *   product's rounding error is captured and every sum runs in double-double; J and every l_k are rounded once, and the
 *   bits depend on the solution and the inputs alone -- not on the flag mode, the memory of the outputs or whether stage was
 *   asked for.
 *   Evaluates the solution that ndlqr_CopyBatchSolutions would deliver against the right-hand side that produced it
 *   (ndlqr_BatchSetRhsFlat + ndlqr_SolveBatchRhsOnly and the steps of ndlqr_BatchStepAsync(Dense) on either buffer set
 *   included), with the caller's costs: in dense-cost mode the caller's Q, H, R; after ndlqr_SolveBatchBoxConstrained,
 *   ndlqr_SolveBatchLinConstrained or their polish the UNSHIFTED cost at the delivered iterate. A right-hand side replaced
 *   without a solve behind it is evaluated as it stands, at the old solution. Works in every flag mode, at any horizon
 *   >= 2 and every block size. Blocking.
 *   NDLQR_ERR_INVALID (ndlqr_hip_last_error() opens with ndlqr_hip_objective) for J NULL, before the first solve, after a
 *   failed constrained solve or a step that computed a slice alone (NDLQR_SOLN_ONLY) -- until the next full solve --, on a
 *   time-axis shard and for an output in the memory of another device.
 *   Nothing else moves: the resident solution and what is known about it, the kept and remembered factorisations, the
 *   adjoint, the failure counts, the box / constraint / polish state stay as they are. ndlqr_BatchSolveTimeMs then reports
 *   the device time of the call's kernels. */
int ndlqr_BatchObjective(NdLqrBatchSolver* bs, double* J, double* stage);
/* additive: iterative refinement of a batch solve with a double-double residual, for callers who need more than the
 * solve paths deliver on ill-conditioned inputs. ndlqr_RefineBatch evaluates r = b - K z of the resident solutions with
 * every row accumulated in double-double and rounded once, re-solves K delta = r against the kept factorisation, and
 * stores z + delta (fp64) for every problem whose residual norm ||r||_inf went down -- up to max_steps times (1 .. 8), with
 * no host read-back between the steps. Step s of a problem is accepted iff its residual norm fell strictly at every step
 * up to s (false for NaN; a rejection is permanent): a problem's residual never grows, one that cannot be improved keeps its
 * solution bit for bit, and NaN or inf data take 0 steps.
 *   Outputs, each [batch] and each may be NULL (host, pinned or the solver's device memory): steps taken; eta = ||r||_inf /
 *   max_i(|b_i| + sum_j |K_ij| |z_j|) before and after them.
 *   Reach: wherever ndlqr_SolveBatchRhsOnly works -- a solve with NDLQR_FLAG_KEEP_RECORDS (fast mode) or
 *   NDLQR_FLAG_KEEP_FACT (any mode). NDLQR_ERR_INVALID without a kept factorisation of the resident inputs (also after a
 *   constrained solve or the upload of new inputs), after a step that computed a slice alone (NDLQR_SOLN_ONLY), on a
 *   time-axis shard, for max_steps outside 1 .. 8 and for device memory of another device.
 *   State: the refined solution is a new resident solution -- ndlqr_CopyBatchSolutions, ndlqr_BatchKktResiduals and the
 *   device pack see it, and an earlier adjoint is invalidated. The kept records and factors, the inputs, the right-hand side
 *   and the flags stay bit for bit as found: a later ndlqr_SolveBatchRhsOnly equals one without the refinement.
 * ndlqr_RefineBatchAdjoint does the same for w of the latest ndlqr_SolveBatchAdjoint against its g; it changes w alone,
 * needs a valid plain adjoint and refuses the adjoint of a constrained solve.
 * ndlqr_BatchKktResidualVector delivers r = b - K z, [batch][nvars] in the packing of ndlqr_CopyBatchSolutions, evaluated
 * in double-double; it needs no kept factorisation and refuses where ndlqr_BatchKktResiduals does.
 * All three block; ndlqr_BatchSolveTimeMs then reports the device time of the whole call. */
int ndlqr_RefineBatch(NdLqrBatchSolver* bs, int max_steps, int* steps, double* eta_before, double* eta_after);
int ndlqr_RefineBatchAdjoint(NdLqrBatchSolver* bs, int max_steps, int* steps, double* eta_before, double* eta_after);
int ndlqr_BatchKktResidualVector(NdLqrBatchSolver* bs, double* r);
/* additive: box-constrained batch solve (MPC with actuator and state limits). For every problem of the batch, the resident
 * LQR problem plus the bounds xlo_k <= x_k <= xhi_k (k = 1 .. N-1) and ulo_k <= u_k <= uhi_k (k = 0 .. N-2), solved by
 * scaled ADMM with over-relaxation and a fixed penalty rho (OSQP-style) on the kept factorisation:
 *   ndlqr_BatchSetBounds: xlo, xhi [batch][N][n], ulo, uhi [batch][N][m] in the flat layout of ndlqr_InitializeBatchFlat
 *   ([N][..], one set for every problem, with NDLQR_BOUNDS_SHARED); NULL = unbounded; entries may be +-INFINITY. Bounds on
 *   x of knot 0 (x0 is fixed) and on u of the last knot (it has no input) are ignored. lo > hi (or NaN) for an entry that
 *   is used: NDLQR_ERR_INVALID, and the previous bounds stay. Host, pinned or the solver's device memory.
 *   ndlqr_SolveBatchBoxConstrained: factors Q + rho M_x, R + rho M_u (M: the bounded entries) once -- or not at all while rho,
 *   the finite / infinite pattern of the bounds and A, B, Q, R are those of the previous constrained solve: an MPC loop of
 *   ndlqr_BatchSetRhsFlat + this call pays only the iterations -- then iterates one right-hand-side re-solve and one
 *   element-wise update kernel per iteration. iters[p], status[p] (each may be NULL; host or the solver's device memory):
 *   iterations taken; 1 = converged, 2 = max_iter reached, the last iterate is returned (not an error; without
 *   infeasibility detection, below, an infeasible problem ends so), 3 = the iterate is not finite (NaN or inf in the
 *   problem's data): stopped, not a solution, 4 = primal infeasible, a certificate was found (only with
 *   ndlqr_BatchSetInfeasibilityDetection; the last iterate is returned, as for 2). A non-positive pivot of the shifted factorisation (Q or R <= 0 on an unbounded entry,
 *   as ndlqr_SolveBatch refuses it) returns NDLQR_ERR_NOT_SPD before any iteration; after that, and after any other
 *   error once the factorisation ran, the solution getters refuse until the next solve. A warm start keeps v, y of the
 *   entries bounded now (y of the others is zeroed). Blocking. Converged when, over the bounded entries of the problem,
 *       ||z - v||_inf <= eps_abs + eps_rel max(||z||_inf, ||v||_inf)   and   rho ||v - v_prev||_inf <= eps_abs + eps_rel ||rho y||_inf
 *   (z: the re-solve, v: its projection onto the bounds, y: the scaled dual); a converged problem is frozen.
 *   The resident solution becomes the constrained one: ndlqr_CopyBatchSolution(s), slices and the device pack hand back
 *   [lambda, x, u] with x, u the projected iterate (the bounds hold exactly) and lambda from the last re-solve.
 *   ndlqr_BatchKktResiduals keeps its meaning -- the unconstrained KKT system --, so after a constrained solve it measures
 *   about ||mu||. The resident A, B, Q, R, q, r, d, x0 are unchanged, but the kept records / factors are those of the
 *   shifted matrix: ndlqr_SolveBatchRhsOnly, the multi-rhs solves and the adjoint return NDLQR_ERR_INVALID until the next
 *   ndlqr_SolveBatch. Reach: wherever a kept factorisation exists (NDLQR_FLAG_KEEP_RECORDS is or-ed in for its own
 *   factorisation in fast mode, NDLQR_FLAG_KEEP_FACT in strict mode), padded shapes included; strict mode is
 *   bit-reproducible (DESIGN.md section 3.9 gives the operation order).
 *   ndlqr_CopyBatchBoundMultipliers: mu = rho y, mu_x [batch][N][n], mu_u [batch][N][m] (either may be NULL): >= 0 where the
 *   upper bound is active, <= 0 at the lower one, 0 inside; z solves the unconstrained problem with q + mu_x, r + mu_u.
 *   Adaptive penalty (adapt_every > 0): rho is per problem, started at the settings' rho. At every
 *   adapt_every-th iteration a running problem takes k = (ilogb(r_prim / s_prim) - ilogb(r_dual / s_dual)) / 2, clamped to
 *   [-6, 6] (r: its residuals, s: the scales of the convergence test above), and for k != 0 moves to rho 2^k within
 *   [rho_min, rho_max], y scaled so that mu = rho y stays; the batch is factored again in every round in which a problem
 *   moved. With warm_start, while the remembered factorisation applies (same pattern, A, B, Q, R and flags), the solve
 *   starts from the penalties the previous one ended with and factors nothing -- the settings' rho is ignored, an MPC
 *   loop keeps what it learnt; otherwise every problem starts at the settings' rho. A fixed-rho solve reuses a
 *   remembered factorisation only when all its penalties are that rho. iters and status keep their meaning.
 *   adapt_every < 0 or rho_min > rho_max: NDLQR_ERR_INVALID. ndlqr_CopyBatchBoxPenalties: rho [batch] of the latest
 *   constrained solve (host, pinned or the solver's device memory).
 *   ndlqr_CopyBatchBoxResiduals: the four numbers of the convergence test above as every problem's last update found
 *   them, resid [batch][4] = r_prim | r_dual | s_prim | s_dual with r_prim = ||z - v||_inf, r_dual = rho ||v - v_prev||_inf,
 *   s_prim = max(||z||_inf, ||v||_inf), s_dual = rho ||y||_inf over the bounded entries (host, pinned or the solver's device
 *   memory). A row holds the values of the last update the problem took part in: the iteration at which it was frozen for
 *   status 1, 3 and 4 (a NaN or an infinity is stored as it is), iteration max_iter for status 2; they are stored before
 *   the decision, with the penalty the iteration ran with. A problem without a bounded entry converges at iteration 1
 *   and has a row of zeros. With them a caller whose problem ended as 2 sees how far it was from the tolerance.
 *   NDLQR_ERR_INVALID unless the resident solution is that of a constrained solve with the current bounds (as
 *   ndlqr_SolveBatchBoxAdjoint: no solve, step, re-solve or ndlqr_BatchSetBounds since).
 *   ndlqr_CopyBatchBoxAdjointResiduals: the same four numbers of the latest ndlqr_SolveBatchBoxAdjoint (below), whose
 *   iteration has the same test; a problem that the box adjoint does not iterate (forward status 3 or 4) has a row of
 *   zeros. NDLQR_ERR_INVALID unless there is a box adjoint of the resident solution (as ndlqr_BatchBoundGradients). */
typedef struct {
  double rho;       /* penalty; 0 -> 0.1 */
  double alpha;     /* over-relaxation in (0, 2); 0 -> 1.6 */
  double eps_abs;   /* 0 -> 1e-6 */
  double eps_rel;   /* 0 -> 1e-6 */
  int max_iter;     /* 0 -> 4000 */
  int check_every;  /* host looks at the convergence count every this many iterations; 0 -> 10 */
  int warm_start;   /* start from v, y of the previous constrained solve (same bounds pattern) */
  int adapt_every;  /* per-problem adaptive penalty, considered every this many iterations; 0 -> fixed rho */
  double rho_min;   /* clamp of the adaptive penalty; 0 -> 1e-6 */
  double rho_max;   /* 0 -> 1e6 */
} NdLqrBoxSettings; /* zero-initialised = all defaults; NULL = all defaults */
#define NDLQR_BOUNDS_SHARED 1u /* bounds arrays are [N][..], one set for every problem */
int ndlqr_BatchSetBounds(NdLqrBatchSolver* bs, unsigned flags, const double* xlo, const double* xhi, const double* ulo,
                         const double* uhi);
int ndlqr_SolveBatchBoxConstrained(NdLqrBatchSolver* bs, const NdLqrBoxSettings* s, int* iters, int* status);
int ndlqr_CopyBatchBoundMultipliers(NdLqrBatchSolver* bs, double* mu_x, double* mu_u);
int ndlqr_CopyBatchBoxPenalties(NdLqrBatchSolver* bs, double* rho);
int ndlqr_CopyBatchBoxResiduals(NdLqrBatchSolver* bs, double* resid);
int ndlqr_CopyBatchBoxAdjointResiduals(NdLqrBatchSolver* bs, double* resid);
/* the constrained solve of ndlqr_InitializeBatchFlatConstrained (above) and its read-outs */
int ndlqr_SolveBatchLinConstrained(NdLqrBatchSolver* bs, const NdLqrBoxSettings* s, int* iters, int* status);
int ndlqr_BatchSetConstraintPenaltyAdaptation(NdLqrBatchSolver* bs, int every, double rho_min, double rho_max);
int ndlqr_CopyBatchConstraintPenalties(NdLqrBatchSolver* bs, double* rho);
int ndlqr_BatchSetConstraintInfeasibilityDetection(NdLqrBatchSolver* bs, int every, double eps);
int ndlqr_CopyBatchConstraintInfeasibilityCertificate(NdLqrBatchSolver* bs, double* dlam, double* dmu);
int ndlqr_CopyBatchConstraintInfeasibilityMeasures(NdLqrBatchSolver* bs, double* measures, int* iteration);
int ndlqr_CopyBatchConstraintMultipliers(NdLqrBatchSolver* bs, double* mu);
int ndlqr_CopyBatchConstraintResiduals(NdLqrBatchSolver* bs, double* resid);
/* additive: primal infeasibility detection in the box-constrained solve. State bounds make
 * infeasibility an ordinary event in MPC; without detection such a problem keeps the whole batch iterating to max_iter.
 *   ndlqr_BatchSetInfeasibilityDetection: every == 0 (the initial state) = off: no call changes a bit of its result.
 *   every > 0: ndlqr_SolveBatchBoxConstrained tests every running problem at the iterations it >= 2 with it % every == 0;
 *   eps == 0 -> 1e-4 (OSQP's eps_prim_inf). every < 0, or eps negative or not finite: NDLQR_ERR_INVALID and the previous
 *   setting stays. The setting belongs to the solver and holds for every later constrained solve.
 *   The test: with dlam = lambda^it - lambda^(it-1) (the multipliers of two consecutive re-solves) and
 *   dmu = rho^it y^it - rho^(it-1) y^(it-1) on the bounded entries (in units of mu, so across a change of the adaptive
 *   penalty too), let
 *       e_x,k = -dlam_k + A_k' dlam_(k+1) + dmu_x,k,   e_u,k = B_k' dlam_(k+1) + dmu_u,k   (no A', B' term at k = N-1),
 *       S = sum over the bounded entries of (hi_i max(dmu_i, 0) + lo_i min(dmu_i, 0)) - x0' dlam_0 - sum_k d_k' dlam_(k+1).
 *   Every (x, u) that satisfies the dynamics and the bounds has e'(x, u) <= S, so e = 0 with S < 0 proves that there is
 *   none. The problem is certified when ||dmu||_inf > 0, ||e||_inf <= eps ||dmu||_inf, S < -eps ||dmu||_inf, and every
 *   entry whose dmu_i points to an infinite bound has |dmu_i| <= eps ||dmu||_inf (it then counts 0 in S); a non-finite
 *   value anywhere means no certificate. A certified problem ends with status 4 and is frozen as a converged one is: it
 *   leaves the running count, so the batch ends when every problem has a status of 1, 3 or 4, or at max_iter. Its resident
 *   solution is its last iterate, as for status 2. The problems iterate independently: detection changes nothing for the
 *   others.
 *   ndlqr_CopyBatchInfeasibilityCertificate: dlam [batch][N][n], dmu_x [batch][N][n], dmu_u [batch][N][m] in the flat
 *   layout of ndlqr_CopyBatchBoundMultipliers (each may be NULL, not all; host, pinned or the solver's device memory);
 *   the rows of every problem whose status is not 4 are zero. NDLQR_ERR_INVALID unless the resident solution is that of
 *   the latest constrained solve and detection was on for it.
 *   ndlqr_CopyBatchInfeasibilityMeasures: the four numbers of every problem's latest check, measures [batch][4] =
 *   ||e||_inf | ||dmu||_inf | max |dmu_i| over the entries pointing to an infinite bound | S, and the iteration of that
 *   check, iteration [batch] (either may be NULL, not both; host, pinned or the solver's device memory). They are stored
 *   before the decision, for certified and running problems alike, a NaN among them as it is; a problem that no check
 *   examined (frozen before the first one) has iteration 0 and a row of zeros. The same refusals as
 *   ndlqr_CopyBatchInfeasibilityCertificate. With them a caller sees how far a running problem is from a certificate --
 *   ||e||_inf / ||dmu||_inf and -S / ||dmu||_inf against eps -- when choosing eps.
 *   Downstream, for a status-4 problem: ndlqr_PolishBatchBoxConstrained reports 2 and leaves it bit for bit;
 *   ndlqr_SolveBatchBoxAdjoint does not iterate it, reports 4 and gives w = 0, nu = 0 (zero gradients);
 *   ndlqr_SolveBatchPolishedAdjoint follows the polish status; a warm-started next solve starts that problem cold
 *   (v = y = 0: its y has diverged and is not a starting point). */
int ndlqr_BatchSetInfeasibilityDetection(NdLqrBatchSolver* bs, int every, double eps);
int ndlqr_CopyBatchInfeasibilityCertificate(NdLqrBatchSolver* bs, double* dlam, double* dmu_x, double* dmu_u);
int ndlqr_CopyBatchInfeasibilityMeasures(NdLqrBatchSolver* bs, double* measures, int* iteration);
/* additive: safeguarded Anderson acceleration of the box-constrained solve. The cost of a
 * constrained solve is its number of iterations; the ADMM is a fixed-point iteration in w = v + y over a problem's
 * bounded entries, and type-II Anderson acceleration extrapolates it from the last mem iterations.
 *   ndlqr_BatchSetBoxAcceleration: mem == 0 (the initial state) = off: no call changes a bit of any result, nothing is
 *   allocated and no other kernel is launched. mem in 1 .. 16: the memory (5 is the documented choice). safeguard == 0 ->
 *   1.0, reg == 0 -> 1e-10. mem < 0 or > 16, or safeguard or reg negative or not finite: NDLQR_ERR_INVALID and the
 *   previous setting stays. The setting belongs to the solver and holds for every later constrained solve (not for
 *   ndlqr_SolveBatchBoxAdjoint, whose ADMM is not accelerated).
 *   The rule, per problem and iteration, with t = alpha z + (1 - alpha) v + y the plain successor of w = v + y and
 *   g = t - (v + y): convergence, NaN and status are evaluated as without acceleration, on v+ = clip(t),
 *   y+ = (y + zh) - v+, before anything else, and a converged problem freezes with them. If the iteration started from an
 *   accelerated iterate and |g|_2 > safeguard |g_prev|_2, the step is rejected: v, y go back to the plain v+, y+ that the
 *   step before saved, the history is cleared, and the next step is plain. Otherwise (t, g) joins a ring of mem + 1
 *   entries; with c >= 1 columns dG = [g_(i+1) - g_i], dT = [t_(i+1) - t_i], gamma solves
 *   (dG'dG + reg tr(dG'dG) / c I) gamma = dG'g by Cholesky and w+ = t - dT gamma gives v = clip(w+), y = w+ - v. A pivot
 *   that is not positive, or a gamma or w+ that is not finite: the plain step, the history cleared. A problem whose
 *   adaptive penalty moves takes the plain step and clears its history. Warm and cold starts begin with an empty history.
 *   With ndlqr_BatchSetInfeasibilityDetection on, the iteration before a check and the check iteration take plain steps.
 *   The ring is scratch of one solve: polish, adjoints, multipliers, penalties and warm starts see v, y, rho and status
 *   as before. Results are the same from run to run (no floating-point atomics).
 *   ndlqr_CopyBatchBoxAcceleration: of the latest constrained solve, accepted and rejected [batch] (steps taken
 *   accelerated; steps rejected by the safeguard), gamma [batch][mem] (the coefficients of every problem's latest
 *   accelerated step, oldest column first, zero beyond its column count) and columns [batch] (that count). Any may be
 *   NULL, not all; host, pinned or the solver's device memory. NDLQR_ERR_INVALID unless the resident solution is that of
 *   the latest constrained solve and acceleration was on for it. */
int ndlqr_BatchSetBoxAcceleration(NdLqrBatchSolver* bs, int mem, double safeguard, double reg);
int ndlqr_CopyBatchBoxAcceleration(NdLqrBatchSolver* bs, int* accepted, int* rejected, double* gamma, int* columns);
/* additive: gradients through the box-constrained solve (differentiable MPC with actuator and state limits). After
 * ndlqr_SolveBatchBoxConstrained, for a loss L(z*) of the constrained solutions and g = dL/dz* (as for
 * ndlqr_SolveBatchAdjoint), ndlqr_SolveBatchBoxAdjoint solves the adjoint of the active-set system
 *     K w + E_A' nu = g,   E_A w = 0
 * (A: the bounded entries whose projected iterate lies exactly on a bound; E_A picks them) by the same ADMM on the
 * forward's kept shifted factorisation -- the penalties the forward ended with, cold start, nothing factored, nothing
 * adapted. The settings' rho, warm_start, adapt_every, rho_min and rho_max are ignored; alpha, eps_abs, eps_rel, max_iter and check_every (0: the defaults of the forward) apply, and iters / status
 * report as for the forward. A problem whose forward ended as 3 or 4 is not iterated and reports that status (4: w = 0,
 * nu = 0). Afterwards
 * ndlqr_CopyBatchAdjoint returns w and ndlqr_BatchGradients dL/d(A, B, Q, R, q, r, d, x0) at the constrained solution,
 * as after ndlqr_SolveBatchAdjoint. ndlqr_BatchBoundGradients returns dL/dc_A = nu: entry i goes to dL/dhi_i when the
 * forward's iterate sits on hi_i (lo_i == hi_i included), to dL/dlo_i when it sits on lo_i, 0 everywhere else; flat
 * layout [batch][N][n] / [batch][N][m], or summed over the batch ([N][..], deterministic) with NDLQR_BOUNDS_SHARED; a
 * NULL output is not computed; host, pinned or the solver's device memory. Where the active constraints are degenerate
 * (their rows of the KKT system are linearly dependent), nu is not unique and the bound gradients are one of many.
 *   Nothing of the forward changes: resident solution, v and y (the next warm start), mu, the remembered shifted
 *   factorisation; ndlqr_SolveBatchAdjoint and the plain re-solves still refuse. The box adjoint returns
 *   NDLQR_ERR_INVALID unless the resident solution is that of the latest constrained solve -- no solve, step, re-solve,
 *   input upload or ndlqr_BatchSetBounds since --, and any later solve invalidates it (as the plain adjoint). Blocking. */
int ndlqr_SolveBatchBoxAdjoint(NdLqrBatchSolver* bs, const double* g, const NdLqrBoxSettings* s, int* iters, int* status);
int ndlqr_BatchBoundGradients(NdLqrBatchSolver* bs, unsigned flags, double* gxlo, double* gxhi, double* gulo, double* guhi);
/* additive: gradients through the solve with linear inequality constraints (differentiable MPC
 * with rate limits, polytopic state sets, state-dependent input limits, and any box on a dense-cost problem). After
 * ndlqr_SolveBatchLinConstrained, for a loss L(z*) of the constrained solutions and g = dL/dz* [batch][nvars] (as for
 * ndlqr_SolveBatchAdjoint), ndlqr_SolveBatchLinAdjoint solves the adjoint of the active-set system
 *     K w + G_A' nu = g,   G_A w = 0        (G = [C D]; the last knot: C alone)
 * (A: the bounded rows whose projected iterate lies exactly on a bound) by the same ADMM on the forward's remembered
 * shifted reduction and factorisation -- its rho, its bounded pattern, a cold start, nothing factored. The settings' rho,
 * warm_start and adapt_every are ignored; alpha, eps_abs, eps_rel, max_iter and check_every (0: the defaults of the
 * forward) apply, and iters / status report as for the forward. A problem whose forward ended as 3 is not iterated and
 * reports 3 (w = 0, nu = 0, zero constraint gradients). Afterwards
 *   ndlqr_CopyBatchAdjoint returns w in the caller's variables, from which dL/d(A, B, Q, H, R, q, r, d, x0) follow as the
 *   outer products of z* and w (ndlqr_BatchGradientsDense assembles them on the device; ndlqr_BatchGradients stays refused
 *   in dense-cost mode);
 *   ndlqr_BatchConstraintGradients returns dL/dC [P][N][p*n] and dL/dD [P][N][p*m] (column-major per knot like C, D): row r
 *   of knot k is -(mu_r w_x' + nu_r x_k') and -(mu_r w_u' + nu_r u_k'), exactly zero outside A and for D of the last knot;
 *   and dL/dlo, dL/dhi [P][N][p]: nu_r goes to dL/dhi when the forward's iterate sits on hi (lo == hi included), to dL/dlo
 *   when it sits on lo, 0 everywhere else. P = batch, or 1 with NDLQR_BOUNDS_SHARED in `flags`: summed over the batch,
 *   deterministically (two calls give the same bits). A NULL output is not computed;
 *   ndlqr_CopyBatchConstraintAdjointMultipliers: nu [batch][N][p], with mu's sign convention;
 *   ndlqr_CopyBatchConstraintAdjointResiduals: [batch][4] of the adjoint's last updates, as ndlqr_CopyBatchConstraintResiduals
 *   (a row of zeros for a problem that was not iterated);
 *   ndlqr_CopyBatchConstraintCodes: one byte per row [batch][N][p]: 0 unbounded, 1 bounded and inactive, 2 active at lo,
 *   3 active at hi.
 * Outputs: host, pinned or the solver's device memory. Where the active rows are degenerate, nu is one of many.
 *   Nothing of the forward changes: resident solution, v and y (the next warm start), mu, its residuals, the remembered
 *   factorisation (ndlqr_hip_factor_count does not move). The adjoint refuses by name (NDLQR_ERR_INVALID,
 *   ndlqr_hip_last_error()) unless the resident solution is that of the latest constrained solve -- no solve, new inputs,
 *   ndlqr_BatchSetRhsFlat or ndlqr_BatchSetConstraintBounds since --, and the four read-outs unless the latest
 *   constrained adjoint belongs to the resident solution (a plain ndlqr_SolveBatchAdjoint never feeds them). Blocking. */
int ndlqr_SolveBatchLinAdjoint(NdLqrBatchSolver* bs, const double* g, const NdLqrBoxSettings* s, int* iters, int* status);
int ndlqr_BatchConstraintGradients(NdLqrBatchSolver* bs, double* gC, double* gD, double* glo, double* ghi, unsigned flags);
int ndlqr_CopyBatchConstraintAdjointMultipliers(NdLqrBatchSolver* bs, double* nu);
int ndlqr_CopyBatchConstraintAdjointResiduals(NdLqrBatchSolver* bs, double* resid);
int ndlqr_CopyBatchConstraintCodes(NdLqrBatchSolver* bs, unsigned char* codes);
/* additive: active-set polish of the latest constrained solve. ADMM run to a loose tolerance has
 * usually found the active set A; the constrained solution then solves K z + E_A' mu = b, E_A z = c_A, and
 * ndlqr_PolishBatchBoxConstrained solves that system directly: it reads A off the iterate (an entry is active at hi when
 * v == hi and y > 0, or lo == hi; at lo when v == lo and y < 0: exact comparisons), factors Q, R + sigma_p on the entries
 * of A once (sigma_p = sigma x the largest entry of diag Q, R of problem p), and takes up to max_steps steps of
 *     r = (b - E_A' mu) - K z  in double-double,   re-solve of r,   z += delta,   mu_A += sigma_p delta_A,   z_A = c_A exactly,
 * a step counting only while the residual norm fell at every step so far (the rule of ndlqr_RefineBatch). Each problem's
 * last accepted iterate is then validated -- mu >= 0 at an upper bound, <= 0 at a lower one, lo <= z <= hi on the free
 * bounded entries, all exact --; where that fails and rounds remain, wrong-signed entries are released, entries outside
 * their box are fixed at the violated bound, and the batch is shifted and factored again (at most max_rounds times).
 * steps[p], status[p] (each may be NULL; host, pinned or the solver's device memory): the accepted steps; 1 = polished: the
 * resident solution is the polished [lambda, x, u] -- every bound holds exactly, active entries sit on their bound bit
 * for bit --, ndlqr_CopyBatchBoundMultipliers returns the polished mu, and v, y of the next warm start are the polished
 * point; 2 = not polished (no accepted step, or the set was still invalid after the last round) and 3 = not finite (or the
 * constrained solve's status was 3): solution, v, y and mu stay bit for bit what the constrained solve left.
 *   Returns NDLQR_ERR_INVALID unless the resident solution is that of the latest ndlqr_SolveBatchBoxConstrained (no solve,
 *   step, re-solve, polish, input upload or ndlqr_BatchSetBounds since). A polish counts as a new solution; it replaces the
 *   remembered ADMM factorisation by its own, so the next constrained solve factors once and ndlqr_SolveBatchBoxAdjoint
 *   refuses; the plain re-solves, the multi-rhs solves and the plain adjoint refuse until the next ndlqr_SolveBatch, as
 *   after the constrained solve. The resident A, B, Q, R, q, r, d, x0 are unchanged on every exit. A non-positive pivot
 *   returns NDLQR_ERR_NOT_SPD with nothing remembered and no resident solution, as for the constrained solve. Strict mode
 *   is bit-reproducible (DESIGN.md section 3.13 gives the operation order). Blocking; ndlqr_BatchSolveTimeMs then reports
 *   the device time of the whole call. */
#define NDLQR_POLISH_DEFAULT_SIGMA 1e8
typedef struct {
  double sigma;    /* penalty on active entries relative to the problem's largest diag(Q,R) entry; 0 -> NDLQR_POLISH_DEFAULT_SIGMA */
  int max_steps;   /* 0 -> 8; at most 32 */
  int max_rounds;  /* active-set correction rounds, each at most one refactorisation; 0 -> 3 */
} NdLqrPolishSettings;  /* NULL / zero-initialised = defaults */
int ndlqr_PolishBatchBoxConstrained(NdLqrBatchSolver* bs, const NdLqrPolishSettings* s, int* steps, int* status);
/* additive: the adjoint of the polished solution. After a polish, for g = dL/dz* as for ndlqr_SolveBatchAdjoint,
 * ndlqr_SolveBatchPolishedAdjoint solves K w + E_A' nu = g, E_A w = 0 on the polish's final active set and its remembered
 * factorisation by the loop of the polish -- right-hand side g, c = 0, start w = nu = 0, up to max_steps steps under the
 * same acceptance rule; nothing is factored, no rounds; sigma and max_rounds of the settings are ignored. steps[p],
 * status[p]: 1 = solved; a problem whose polish status is not 1 reports that status (2 or 3) and gets w = 0, nu = 0; 2 also
 * when no step was accepted. Afterwards ndlqr_CopyBatchAdjoint and ndlqr_BatchGradients work as after the box adjoint,
 * and ndlqr_BatchBoundGradients returns nu split by the polish codes (same layouts, same deterministic batch sums).
 * NDLQR_ERR_INVALID unless the resident solution is that of the latest polish and its factorisation is still remembered
 * (no solve, step, re-solve, input upload or ndlqr_BatchSetBounds since). g, steps, status: host, pinned or the solver's
 * device memory. Nothing of the polish changes. Blocking; ndlqr_BatchSolveTimeMs reports the device time of the call. */
int ndlqr_SolveBatchPolishedAdjoint(NdLqrBatchSolver* bs, const double* g, const NdLqrPolishSettings* s, int* steps, int* status);
/* additive: active-set polish of the latest solve with linear inequality constraints: section
 * 3.13's polish carried from entries to rows. With G_k = [C_k D_k] (C alone at the last knot), A the active rows and c
 * the bound each is active at, the constrained solution solves K z + G_A' mu = b, G_A z = c_A in the caller's variables.
 * ndlqr_PolishBatchLinConstrained reads A off the iterate of the latest ndlqr_SolveBatchLinConstrained (a row is active
 * at hi when v == hi and y > 0, or lo == hi; at lo when v == lo and y < 0: exact comparisons; mu = rho_p y there), shifts
 * the costs by sigma_p G_A' G_A (sigma_p = sigma x the largest entry of diag Q, R of problem p / the largest squared norm
 * of its bounded rows of [C D]), reduces and factors them once per round, and takes up to max_steps steps of
 *     r_z = b - K z - G_A' mu,  r_c = c_A - G_A z,   K^ delta = r_z + sigma_p G_A' r_c,   z += delta,
 *     mu_A += sigma_p (G_A delta - r_c),
 * a step counting only while max(|r_z|, |r_c|) fell at every step so far (the rule of ndlqr_RefineBatch). Each problem's
 * last accepted iterate is then validated -- mu >= 0 at an upper bound, <= 0 at a lower one, lo <= C x + D u <= hi on the
 * inactive bounded rows, all exact --; where that fails and rounds remain, wrong-signed rows are released, violated rows
 * are fixed at the violated bound, and the batch is shifted, reduced and factored again (at most max_rounds times).
 * steps[p], status[p] (each may be NULL; host, pinned or the solver's device memory): the accepted steps; 1 = polished: the
 * resident solution is the polished [lambda, x, u], ndlqr_CopyBatchConstraintMultipliers returns the polished mu, and v
 * (the rows clipped to their bounds) and y = mu / rho_p of the next warm start are the polished point; 2 = not polished
 * (no accepted step, the set still invalid after the last round, or the constrained solve certified the problem
 * infeasible) and 3 = not finite (or the constrained solve's status was 3): solution, v, y and mu stay bit for bit what
 * the constrained solve left. UNLIKE the box polish an active row cannot be put onto its bound by assignment: the active
 * rows hold to the floor of the residual (the final |r_c|), not bit for bit.
 *   Returns NDLQR_ERR_INVALID (by name, ndlqr_hip_last_error()) unless the resident solution is that of the latest
 *   ndlqr_SolveBatchLinConstrained (no solve, polish, input upload, ndlqr_BatchSetRhsFlat or
 *   ndlqr_BatchSetConstraintBounds since), outside constrained mode, for steps / status in another device's memory, and
 *   when a kernel would stage more than the LDS of a workgroup (the message has the bytes). A polish counts as a new
 *   solution; it takes over the shifted-cost, record and reduced-problem buffers of the constrained solve and drops its
 *   factorisation: ndlqr_hip_factor_count moves by one per round, the next ndlqr_SolveBatchLinConstrained reduces and
 *   factors once (with warm_start from the polished v, y), and ndlqr_SolveBatchLinAdjoint and
 *   ndlqr_BatchConstraintGradients refuse until then. A plain ndlqr_SolveBatch afterwards gives the bits it gave before.
 *   A non-positive pivot returns NDLQR_ERR_NOT_SPD with nothing remembered and the solutions of the constrained solve back
 *   in place. The residual (rows accumulated in double-double, rounded once) is the same bits in strict and default mode. NULL / zero settings: max_steps 8, max_rounds 3,
 *   sigma NDLQR_LIN_POLISH_DEFAULT_SIGMA. Blocking; ndlqr_BatchSolveTimeMs then reports the device time of the whole call.
 * ndlqr_CopyBatchConstraintPolishCodes: the row codes of the latest polish, uint8 [batch][N][p] (0 unbounded, 1 bounded
 * and inactive, 2 active at lo, 3 active at hi; host or the solver's device memory); refused by name unless the resident
 * solution is that of a polish. */
#define NDLQR_LIN_POLISH_DEFAULT_SIGMA 1e8
int ndlqr_PolishBatchLinConstrained(NdLqrBatchSolver* bs, const NdLqrPolishSettings* s, int* steps, int* status);
int ndlqr_CopyBatchConstraintPolishCodes(NdLqrBatchSolver* bs, unsigned char* codes);
void* ndlqr_BatchDeviceContext(NdLqrBatchSolver* bs);      /* NdlqrHipCtx* (ndlqr_hip.h) */

/* Seeded synthetic problem generator (host, bit-reproducible). */
int ndlqr_GenerateSyntheticFlat(int nstates, int ninputs, int nhorizon, uint64_t seed, double* A,
                                double* B, double* Q, double* R, double* q, double* r, double* d,
                                double* x0);
LQRProblem* ndlqr_NewSyntheticLQRProblem(int nstates, int ninputs, int nhorizon, uint64_t seed);

const char* ndlqr_Version(void);

#ifdef __cplusplus
}
#endif
#endif /* NDLQR_H_ */
