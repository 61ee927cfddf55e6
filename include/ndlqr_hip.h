/*
 * ndlqr_hip.h -- thin C-ABI shim between the plain-C host library and the HIP kernels.
 *
 * Plain pointers and sizes only. This is the device boundary that SURVEY.md (section 1) inserts
 * between the reference's L2 driver (src/solve.c) and its L1/L0 numerics
 * (src/nested_dissection.c, src/linalg_custom.c): everything behind these calls runs on
 * gfx950. Implemented in rslqr_amd/csrc: the context, the solve pipeline and the downloads in ndlqr_hip.hip, each
 * optional feature in a unit of its own (hip_grad.hip: adjoint and gradients, hip_box.hip: bounds, ADMM, polish,
 * hip_refine.hip, hip_cost.hip: dense costs, hip_lin.hip: linear inequality constraints, hip_lin_polish.hip: their active-set polish, hip_dense.hip: the Matrix* helpers).
 *
 * Device data model (all fp64):
 *   inputs  AB  [batch][N][n][n+m]   row i of knot k = [A_k(i,:) | B_k(i,:)]   (A,B row-major)
 *           QR  [batch][N][n+m]      diag(Q_k) then diag(R_k)
 *           rhs [batch][N][2n+m]     initial right-hand side, already negated like
 *                                    src/solver.c:188-190: knot k = [-(x0 | d_{k-1}); -q_k; -r_k]
 *                                    (kept untouched by the solve, so solves can be repeated)
 *   state   F   [batch][K][N][2n+m][n]  factor block (level p, knot k), ROW-major; rows
 *                                       0..n-1 lambda, n..2n-1 state, 2n..2n+m-1 input.
 *                                       (reference: column-major sub-blocks, src/nddata.c:40-53)
 *           z   [batch][N][2n+m]     rhs in / solution out, same order as the reference
 *           info[batch+1]            non-positive Cholesky pivots per problem, batch total last (cumulative
 *                                    over solves; ndlqr_hip_cholesky_failures reports those since the last
 *                                    synchronisation)
 */
#ifndef NDLQR_HIP_H_
#define NDLQR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct NdlqrHipCtx NdlqrHipCtx;

int ndlqr_hip_device_count(void);
const char* ndlqr_hip_last_error(void);

/* replaces the allocation half of ndlqr_NewNdLqrSolver (src/solver.c:61-96) for a batch.
 * nhorizon: any value >= 2. One that is no power of two runs padded to the next one on the device (the horizon padding is
 * not optional: NDLQR_CREATE_NO_PAD and NDLQR_NO_PAD govern the block size only); the functions below keep the caller's
 * horizon in every array they take or fill, or refuse (include/ndlqr.h, at ndlqr_NewBatchSolver, has the list). */
NdlqrHipCtx* ndlqr_hip_create(int nstates, int ninputs, int nhorizon, int batch, int device);
/* ... with creation options: NDLQR_CREATE_NO_PAD keeps the caller's block size on the device (a block size without
 * a size-specialised instance otherwise runs zero-padded inside one, with another array layout: raw device pointers
 * -- ndlqr_hip_device_pointers -- need the caller's own). The environment variable NDLQR_NO_PAD=1 does the same for
 * every context of the process. */
#define NDLQR_CREATE_NO_PAD 1u
NdlqrHipCtx* ndlqr_hip_create_ex(int nstates, int ninputs, int nhorizon, int batch, int device, unsigned create_flags);
void ndlqr_hip_destroy(NdlqrHipCtx* ctx);
int ndlqr_hip_set_flags(NdlqrHipCtx* ctx, unsigned flags); /* NDLQR_FLAG_* of ndlqr.h */
unsigned ndlqr_hip_get_flags(const NdlqrHipCtx* ctx);
/* Use an externally owned hipStream_t (e.g. torch's current stream); NULL = own stream. */
int ndlqr_hip_set_stream(NdlqrHipCtx* ctx, void* hip_stream);
void* ndlqr_hip_get_stream(NdlqrHipCtx* ctx);

/* H2D of packed inputs for problems [p0, p0+count) (host layout = device layout above).
 * Replaces the data movement of ndlqr_InitializeWithLQRProblem (src/solver.c:122-194); the
 * zero-padded KKT `data` array is never materialised (kernels read A,B,Q,R and the rhs directly). */
int ndlqr_hip_upload_inputs(NdlqrHipCtx* ctx, int p0, int count, const double* AB,
                            const double* QR, const double* rhs);
/* The same packing done ON the device from flat arrays that already live in HBM (reference
 * layout: A [batch][N][n*n] and B [batch][N][n*m] column-major, Q,q,d [batch][N][n], R,r [batch][N][m],
 * x0 [batch][n]); asynchronous on the context's stream. The caller orders the pack kernel behind
 * whatever produced the inputs: synchronise the producer stream first, or make it the context's
 * stream with ndlqr_hip_set_stream. Invalidates a cached factorisation / cached records. */
int ndlqr_hip_pack_flat_device(NdlqrHipCtx* ctx, const double* A, const double* B, const double* Q,
                               const double* R, const double* q, const double* r, const double* d,
                               const double* x0);
/* Dense cost matrices and state-input cross terms (ndlqr.h: ndlqr_InitializeBatchFlatDense). The
 * dense-cost problem -- Q [batch][N][n*n], R [batch][N][m*m], H [batch][N][n*m] (may be NULL: zero), column-major like A and
 * B, of which only the LOWER triangles of Q and R are read; the other arrays as for ndlqr_hip_pack_flat_device -- is reduced
 * on the device to a unit-cost problem of the same shape (kernels_cost.hpp), which goes through ndlqr_hip_pack_flat_device
 * like a caller's. Every array: host, pinned or this device's memory. A, B, H, R, r, d of the last knot are never loaded.
 * The context is in dense-cost mode from then on, until ndlqr_hip_upload_inputs or ndlqr_hip_pack_flat_device is called.
 * A pivot that is not positive in R_k or in Q_k - H_k R_k^-1 H_k' counts like one of the solver's own Cholesky: the next
 * synchronisation reports it (ndlqr_hip_cholesky_failures). Block sizes whose working set per knot in cost_transform
 * -- 3 n^2 + 2 n m + m^2 doubles and the padding -- exceeds the LDS of a workgroup are refused by name.
 * CARRIED THROUGH in dense-cost mode, every result in the caller's variables: ndlqr_hip_solve_async /
 * ndlqr_hip_synchronize in every flag mode, ndlqr_hip_download_solutions, ndlqr_hip_pack_solutions_device,
 * ndlqr_hip_set_rhs_dense + ndlqr_hip_solve_rhs_async, ndlqr_hip_solve_adjoint + ndlqr_hip_download_adjoint,
 * ndlqr_hip_cholesky_failures, ndlqr_hip_last_solve_ms, any horizon >= 2.
 * REFUSED in dense-cost mode (NDLQR_ERR_INVALID; ndlqr_hip_last_error() opens with the function's name): ndlqr_hip_step_async,
 * ndlqr_hip_solve_slices_async, ndlqr_hip_set_step_selection (a non-empty one), ndlqr_hip_download_selection,
 * ndlqr_hip_solve_multi_rhs(_slices), ndlqr_hip_gradients, ndlqr_hip_refine, ndlqr_hip_kkt_residual,
 * ndlqr_hip_kkt_residual_vector (their rows are those of the reduced system), ndlqr_hip_set_bounds and everything on the box
 * solve (ndlqr_hip_solve_box(_ex), ndlqr_hip_solve_box_adjoint, ndlqr_hip_bound_gradients, ndlqr_hip_polish_box,
 * ndlqr_hip_solve_polished_adjoint, ndlqr_hip_set_box_infeasibility / ndlqr_hip_set_box_acceleration when switching on, and
 * the box downloads), the ndlqr_hip_time_shard_* functions, ndlqr_hip_download_factors, ndlqr_hip_download_rhs_blocks,
 * ndlqr_hip_device_pointers, ndlqr_hip_staged_io and ndlqr_hip_solve_staged. (The step and the slices have dense-cost
 * forms under names of their own: ndlqr_hip_step_dense_async, ndlqr_hip_solve_slices_dense_async,
 * ndlqr_hip_download_selection_dense.)
 * ndlqr_hip_set_rhs_dense: a new flat right-hand side q, r, d, x0 in the caller's variables (same memories).
 * ndlqr_hip_download_cost_reduction (read-out for the tests): the records L [batch][N][n*n], LR [batch][N][m*m], G
 * [batch][N][m*n] (column-major; the triangles with zeros above; LR = 1, G = 0 at the last knot) and the reduced problem in
 * the flat layout, At, Bt, qt, rt, dt [batch][N][..], x0t [batch][n], into HOST memory; any pointer may be NULL. */
int ndlqr_hip_init_dense(NdlqrHipCtx* ctx, const double* A, const double* B, const double* Q, const double* H,
                         const double* R, const double* q, const double* r, const double* d, const double* x0);
int ndlqr_hip_cost_is_dense(const NdlqrHipCtx* ctx);
/* Under NDLQR_FLAG_PROFILE: device time (HIP events, ms) of the latest cost_factor + cost_transform | cost_apply_t (S') |
 * cost_apply (S), 3 doubles; a profiled call waits for its kernels. Without the flag nothing is recorded. */
int ndlqr_hip_cost_phase_ms(NdlqrHipCtx* ctx, double* out3);
int ndlqr_hip_set_rhs_dense(NdlqrHipCtx* ctx, const double* q, const double* r, const double* d, const double* x0);
int ndlqr_hip_download_cost_reduction(NdlqrHipCtx* ctx, double* L, double* LR, double* G, double* At, double* Bt,
                                      double* qt, double* rt, double* dt, double* x0t);
/* General linear inequality constraints lo_k <= C_k x_k + D_k u_k <= hi_k (ndlqr.h: ndlqr_InitializeBatchFlatConstrained;
 * DESIGN.md section 3.17). ndlqr_hip_init_constrained takes the nine arrays of ndlqr_hip_init_dense and p >= 1 rows per
 * knot, C [batch][N][p*n], D [batch][N][p*m] (column-major per knot; D of the last knot is never loaded), lo, hi [P][N][p]
 * with P = batch, or 1 when `shared`; entries of lo, hi may be +-inf. Host or this device's memory. It retains A, B, Q, H,
 * R, the right-hand side, C and D on the device and leaves the context in dense-cost mode exactly as ndlqr_hip_init_dense
 * does -- constrained mode (ndlqr_hip_is_constrained) is dense-cost mode with constraints; ndlqr_hip_init_dense,
 * ndlqr_hip_pack_flat_device and ndlqr_hip_upload_inputs leave it.
 * ndlqr_hip_set_constraint_bounds: new lo, hi; refuses lo > hi or NaN before anything is replaced; a new bounded pattern
 * drops the remembered shifted factorisation.
 * ndlqr_hip_solve_constrained: scaled ADMM with the penalty rho (arguments and statuses of ndlqr_hip_solve_box;
 * adapt_every > 0 is refused: the argument is the box settings', the adaptive penalty of this solve is switched on by
 * ndlqr_hip_set_constraint_adaptation); the
 * resident solution afterwards is [lambda, x, u] of the last re-solve in the caller's variables.
 * ndlqr_hip_set_constraint_adaptation: every > 0 lets the solves that follow move every running
 * problem's penalty at the iterations it % every == 0, it < max_iter, within [rho_min, rho_max] (0 < rho_min <= rho_max);
 * every = 0: off. Any mode; no initialiser resets it. ndlqr_hip_download_constraint_penalties: rho [batch] of the latest
 * constrained solve.
 * ndlqr_hip_download_constraint_multipliers: mu = rho[b] y [batch][N][p]; ndlqr_hip_download_constraint_residuals: [batch][4]
 * as ndlqr_hip_download_box_residuals. ndlqr_hip_download_constraint_reduction (read-out for the tests, HOST memory, any
 * pointer may be NULL): the shifted costs Qs [batch][N][n*n], Hs [batch][N][n*m], Rs [batch][N][m*m], the shifted records and
 * reduced problem as ndlqr_hip_download_cost_reduction gives the plain ones, and the iterates v, y [batch][N][p].
 * Every refusal opens ndlqr_hip_last_error() with the function's name. */
int ndlqr_hip_init_constrained(NdlqrHipCtx* ctx, const double* A, const double* B, const double* Q, const double* H,
                               const double* R, const double* q, const double* r, const double* d, const double* x0, int p,
                               const double* C, const double* D, const double* lo, const double* hi, int shared);
int ndlqr_hip_is_constrained(const NdlqrHipCtx* ctx);
int ndlqr_hip_set_constraint_bounds(NdlqrHipCtx* ctx, const double* lo, const double* hi, int shared);
int ndlqr_hip_solve_constrained(NdlqrHipCtx* ctx, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                                int check_every, int warm_start, int adapt_every, int* iters, int* status);
int ndlqr_hip_set_constraint_adaptation(NdlqrHipCtx* ctx, int every, double rho_min, double rho_max);
int ndlqr_hip_download_constraint_penalties(NdlqrHipCtx* ctx, double* rho);
/* Infeasibility detection of that solve (ndlqr.h: ndlqr_BatchSetConstraintInfeasibilityDetection):
 * every > 0 lets the constrained solves that follow test every running problem for a Farkas certificate at the iterations
 * it >= 2, it % every == 0 (status 4); eps > 0 and finite. every = 0: off. Any mode, any horizon; no initialiser resets it.
 * The read-outs -- dlam [batch][N][n] and dmu [batch][N][p] (either may be NULL; zero rows for a problem that is not 4),
 * measures [batch][4] = ||e||_inf | D | the maximum toward an infinite bound | S and the iteration [batch] of every
 * problem's latest check -- go to host memory or this device's and refuse by name unless the resident solution is that
 * of the latest constrained solve and detection was on for it. */
int ndlqr_hip_set_constraint_infeasibility(NdlqrHipCtx* ctx, int every, double eps);
int ndlqr_hip_download_constraint_infeasibility_certificate(NdlqrHipCtx* ctx, double* dlam, double* dmu);
int ndlqr_hip_download_constraint_infeasibility_measures(NdlqrHipCtx* ctx, double* measures, int* iteration);
int ndlqr_hip_download_constraint_multipliers(NdlqrHipCtx* ctx, double* mu);
int ndlqr_hip_download_constraint_residuals(NdlqrHipCtx* ctx, double* resid);
int ndlqr_hip_download_constraint_reduction(NdlqrHipCtx* ctx, double* Qs, double* Hs, double* Rs, double* L, double* LR,
                                            double* G, double* At, double* Bt, double* qt, double* rt, double* dt, double* x0t,
                                            double* v, double* y);
/* Gradients through the solve with linear inequality constraints (ndlqr.h: ndlqr_SolveBatchLinAdjoint,
 * ndlqr_BatchConstraintGradients). ndlqr_hip_solve_constrained_adjoint: the adjoint of the
 * active-set system for g = dL/dz* [batch][nvars] by the forward's ADMM on its remembered shifted reduction and
 * factorisation (its penalties rho [batch] as it ended with them, a cold start, nothing factored, nothing adapted); refuses unless the resident solution is that of the latest
 * ndlqr_hip_solve_constrained with its right-hand side and bounds. Afterwards ndlqr_hip_download_adjoint returns w.
 * ndlqr_hip_constraint_gradients: dL/dC [P][N][p*n], dL/dD [P][N][p*m] (column-major per knot), dL/dlo, dL/dhi [P][N][p]
 * with P = batch, or 1 when `summed` (deterministic batch sums); each may be NULL.
 * ndlqr_hip_download_constraint_adjoint_multipliers: nu [batch][N][p].
 * ndlqr_hip_download_constraint_adjoint_residuals: [batch][4] of the adjoint's last updates.
 * ndlqr_hip_download_constraint_codes: the row codes [batch][N][p] bytes (0 unbounded, 1 free, 2 at lo, 3 at hi) and,
 * for the tests, the adjoint's own v [batch][N][p] into HOST memory (either may be NULL).
 * The gradients and the three read-outs refuse unless the latest constrained adjoint is that of the resident solution.
 * Outputs: host or this device's memory. */
int ndlqr_hip_solve_constrained_adjoint(NdlqrHipCtx* ctx, const double* g, double alpha, double eps_abs, double eps_rel,
                                        int max_iter, int check_every, int* iters, int* status);
int ndlqr_hip_constraint_gradients(NdlqrHipCtx* ctx, int summed, double* gC, double* gD, double* glo, double* ghi);
int ndlqr_hip_download_constraint_adjoint_multipliers(NdlqrHipCtx* ctx, double* nu);
int ndlqr_hip_download_constraint_adjoint_residuals(NdlqrHipCtx* ctx, double* resid);
int ndlqr_hip_download_constraint_codes(NdlqrHipCtx* ctx, unsigned char* codes, double* v);
/* Active-set polish of the latest solve with linear inequality constraints (ndlqr.h: ndlqr_PolishBatchLinConstrained;
 * DESIGN.md section 3.23). ndlqr_hip_polish_constrained takes the resolved settings (sigma > 0, 1 <= max_steps <= 32,
 * max_rounds >= 0) and blocks; steps / status [batch] may be NULL (host, pinned or this device's memory).
 * ndlqr_hip_download_constraint_polish_codes: the row codes of the latest polish, [batch][N][p] bytes (0 unbounded, 1
 * bounded and inactive, 2 active at lo, 3 active at hi), into host memory or this device's. */
int ndlqr_hip_polish_constrained(NdlqrHipCtx* ctx, double sigma, int max_steps, int max_rounds, int* steps, int* status);
int ndlqr_hip_download_constraint_polish_codes(NdlqrHipCtx* ctx, unsigned char* codes);
/* developer / test hooks, not for production use (HOST memory, blocking copies and repacks on the host; any output may be
 * NULL). ndlqr_hip_constraint_polish_residual: the residual kernel of the polish alone, in constrained mode, on given z
 * [batch][nvars] (packed, the caller's variables), mu [batch][N][p], row codes [batch][N][p] bytes and sigma_p [batch]: r
 * [batch][nvars] = r_z + sigma_p G_A' r_c, rc [batch][N][p] = c_A - G_A z, norms [2][batch] = max(|r_z|, |r_c|) | |r_c|;
 * poison_pad != 0 puts NaN instead of zero into the pad entries and pad knots of the device's copy of z.
 * It overwrites the state a polish left (its read-outs refuse afterwards).
 * ndlqr_hip_download_constraint_polish_state: of the latest polish the candidate zc [batch][nvars], muc [batch][N][p] of
 * its last formed step, the norm slots of its last round [2][max_steps + 1][batch] (the front of a buffer of
 * 2 x 33 x batch doubles, which `norms` must hold), sigma_p [batch] and the number of its factorisations. */
int ndlqr_hip_constraint_polish_residual(NdlqrHipCtx* ctx, const double* z, const double* mu, const unsigned char* codes,
                                         const double* sig, int poison_pad, double* r, double* rc, double* norms);
int ndlqr_hip_download_constraint_polish_state(NdlqrHipCtx* ctx, double* zc, double* muc, double* norms, double* sig,
                                               int* rounds);
/* Under NDLQR_FLAG_PROFILE: the device time of the latest polish spent in lin_polish_residual | lin_polish_apply_t + the
 * re-solve | lin_polish_update (out3, ms), and how many of each were added up (launches3, may be NULL). */
int ndlqr_hip_constraint_polish_phase_ms(NdlqrHipCtx* ctx, double* out3, int* launches3);
/* Device pointers for zero-copy producers (order: AB, QR, rhs, F, z). Allocates the factor array and
 * sets the pipeline depth to 1, so that z is THE solution buffer from then on. */
int ndlqr_hip_device_pointers(NdlqrHipCtx* ctx, void** out5);

/* ndlqr_Solve (src/solve.c:38-190) for the whole batch: leaf kernel + one kernel per tree level
 * (inner products, Cholesky, triangular solves, Schur updates, rhs sweep fused). Async on the
 * context's stream; HIP events bracket the sequence. */
int ndlqr_hip_solve_async(NdlqrHipCtx* ctx);
int ndlqr_hip_synchronize(NdlqrHipCtx* ctx);
/* One-shot solve from / into pinned host staging owned by the context -- what the drop-in ndlqr_Solve (host memory in,
 * host memory out on every call, src/solve.c:38-201) runs: ndlqr_hip_staged_io hands out the staging (AB, QR, rhs in
 * the packed layout above but in the CALLER's block size, z = [batch][N][2n+m] coming back), the caller packs into
 * it, ndlqr_hip_solve_staged replays one captured graph -- the three copies up, the launch chain, the copy down --
 * and waits for it: one launch and one synchronisation per call. Stream-ordered (pipeline depth 1 from the first
 * call on). Returns like ndlqr_hip_synchronize; ndlqr_hip_cholesky_failures tells about pivots. */
int ndlqr_hip_staged_io(NdlqrHipCtx* ctx, double** AB, double** QR, double** rhs, double** z);
int ndlqr_hip_solve_staged(NdlqrHipCtx* ctx);
/* Solve pipeline. Depth 2 (default; NDLQR_PIPELINE): consecutive ndlqr_hip_solve_async calls of one
 * context alternate between two sets of output buffers (records, accumulators, solution), each on its
 * own stream, so that a solve starts while the previous one is still in its thinly populated upper tree
 * levels / its HBM-bound back-substitution. Every solve is complete; ndlqr_hip_synchronize waits for all
 * of them and the download functions return the most recent one. Applies to the schedules that keep
 * nothing but the solution (no factor array, no kept records, no per-kernel events, own stream); depth 1
 * = strictly stream-ordered solves. Inputs must not be replaced while solves are in flight: the upload /
 * pack functions wait for them first. */
int ndlqr_hip_set_pipeline_depth(NdlqrHipCtx* ctx, int depth);
int ndlqr_hip_pipeline_depth(const NdlqrHipCtx* ctx);
/* Factor / solve split: new right-hand side(s) against the factorisation cached by the last
 * ndlqr_hip_solve_async with NDLQR_FLAG_KEEP_FACT (the reference's solution sweep,
 * src/solve.c:137-182, alone). rhs layout as in ndlqr_hip_upload_inputs. */
int ndlqr_hip_upload_rhs(NdlqrHipCtx* ctx, int p0, int count, const double* rhs);
int ndlqr_hip_solve_rhs_async(NdlqrHipCtx* ctx);
double ndlqr_hip_last_solve_ms(NdlqrHipCtx* ctx); /* valid after synchronize */
/* Adjoint solve and parameter gradients (ndlqr.h: ndlqr_SolveBatchAdjoint, ndlqr_BatchGradients). The adjoint K w = g is
 * the re-solve of ndlqr_hip_solve_rhs_async (kept records, else the factor array) with g packed into an adjoint
 * right-hand side, into an adjoint solution array of its own: [batch][N][2n+m] each, allocated on first use. Blocking. */
int ndlqr_hip_solve_adjoint(NdlqrHipCtx* ctx, const double* g);
int ndlqr_hip_download_adjoint(NdlqrHipCtx* ctx, double* w); /* [batch][nvars]: host, pinned or this device's memory */
int ndlqr_hip_gradients(NdlqrHipCtx* ctx, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gR, double* gq,
                        double* gr, double* gd, double* gx0);
/* ... in dense-cost mode (ndlqr.h: ndlqr_BatchGradientsDense): the nine gradients from packed
 * copies of z and w in the caller's variables, after ndlqr_hip_solve_adjoint or -- the resident solution that of a
 * constrained solve -- ndlqr_hip_solve_constrained_adjoint. Every refusal opens with the function's name. Blocking.
 * ndlqr_hip_gradients_dense_constants: out2[0] the workgroups the split of a batch sum aims at, out2[1] the knots of a
 * chunk at most (for the tests, which size a batch by them). */
int ndlqr_hip_gradients_dense(NdlqrHipCtx* ctx, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gH, double* gR,
                              double* gq, double* gr, double* gd, double* gx0);
int ndlqr_hip_gradients_dense_constants(int* out2);
/* Feedback gains and cost-to-go matrices of the resident problems (ndlqr.h: ndlqr_BatchFeedbackGains has the contract;
 * DESIGN.md section 3.22): the backward recursion of one workgroup per problem on the device inputs and the latest
 * right-hand side, for the knots [knot0, knot0 + nknots). K [batch][nknots][m*n], kff [batch][nknots][m],
 * P [batch][nknots][n*n], p [batch][nknots][n], fails [batch] (int): each may be NULL (not all of the four doubles); host,
 * pinned or this device's memory. Every refusal opens with the function's name. Blocking.
 * ndlqr_hip_feedback_gains_lds: the bytes of LDS its sweep needs at (n, m), with the second input buffer or without it
 * (for the tests and tools, which pick shapes by it). */
int ndlqr_hip_feedback_gains(NdlqrHipCtx* ctx, int knot0, int nknots, double* K, double* kff, double* P, double* p, int* fails);
size_t ndlqr_hip_feedback_gains_lds(int n, int m, int second);
/* The objective value of every problem at its resident solution and its stage costs (ndlqr.h: ndlqr_BatchObjective has the
 * contract). J [batch]; stage [batch][N], may be NULL; host, pinned or this device's memory (the
 * kernel writes this device's memory, host memory is staged, another device's is refused). Blocking: everything in flight
 * is waited for, the kernels run on the stream of the buffer set that holds the latest solution and read the right-hand
 * side of that set -- the one that produced it. A read-out: z, what is known about it, the kept and remembered
 * factorisations, the adjoint, the failure words and the box / constraint / polish state stay as they are; only
 * ndlqr_hip_last_solve_ms moves. NDLQR_ERR_INVALID, the message opening with ndlqr_hip_objective: J NULL, no full valid
 * resident solution (none yet, a failed constrained solve, a NDLQR_SOLN_ONLY step), a time-axis shard, an output in
 * another device's memory, a block size whose chunk does not fit the LDS of a workgroup (the bytes are named).
 * ndlqr_hip_objective_constants: out2[0] the knots of a workgroup's chunk, out2[1] the workgroup size (for the tests,
 * which size a horizon by them). */
int ndlqr_hip_objective(NdlqrHipCtx* ctx, double* J, double* stage);
int ndlqr_hip_objective_constants(int* out2);
/* Iterative refinement with a double-double residual (ndlqr.h: ndlqr_RefineBatch, ndlqr_RefineBatchAdjoint,
 * ndlqr_BatchKktResidualVector). which = 0: the resident solution against the resident right-hand
 * side; 1: w of the latest plain adjoint against its packed g. max_steps in [1, 8]. steps [batch] (int), eta_before,
 * eta_after [batch]: each may be NULL; host, pinned or this device's memory. Blocking. ndlqr_hip_refine_phase_ms: device
 * time of the residual kernels | re-solves | commits of the latest refinement that ran under NDLQR_FLAG_PROFILE (3
 * doubles). ndlqr_hip_kkt_residual_vector: r = b - K z of the resident solution, [batch][nvars] in the packing of
 * ndlqr_hip_download_solutions, every row accumulated in double-double (host, pinned or this device's memory). */
int ndlqr_hip_refine(NdlqrHipCtx* ctx, int which, int max_steps, int* steps, double* eta_before, double* eta_after);
int ndlqr_hip_refine_phase_ms(NdlqrHipCtx* ctx, double* out3);
int ndlqr_hip_kkt_residual_vector(NdlqrHipCtx* ctx, double* r);
/* Box-constrained solve by scaled ADMM on the kept factorisation (ndlqr.h: ndlqr_BatchSetBounds,
 * ndlqr_SolveBatchBoxConstrained, ndlqr_CopyBatchBoundMultipliers). Bounds in the flat layout,
 * [batch][N][n] / [batch][N][m], or [N][..] once for every problem when `shared`; NULL = unbounded; host, pinned or this
 * device's memory. ndlqr_hip_solve_box takes the resolved settings (no zero defaults here) and blocks; iters / status
 * [batch] may be NULL. Multipliers mu = rho_p y in the flat layout (rho_p: the penalty of problem p). ndlqr_hip_factor_count: factorisations launched by
 * this context so far (tests: a constrained solve that reuses the remembered shifted factorisation launches none). */
int ndlqr_hip_set_bounds(NdlqrHipCtx* ctx, int shared, const double* xlo, const double* xhi, const double* ulo,
                         const double* uhi);
int ndlqr_hip_solve_box(NdlqrHipCtx* ctx, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                        int check_every, int warm_start, int* iters, int* status);
/* ndlqr_hip_solve_box_ex: the same with a per-problem adaptive penalty: adapt_every > 0 lets
 * every running problem move its rho by a power of two at every adapt_every-th iteration, within [rho_min, rho_max]
 * (resolved: 0 < rho_min <= rho_max), and the batch is factored again whenever one did; adapt_every == 0 is
 * ndlqr_hip_solve_box. ndlqr_hip_download_box_penalties: rho [batch] of the latest constrained solve (host, pinned or
 * this device's memory). ndlqr_hip_download_box_residuals, ndlqr_hip_download_box_adjoint_residuals: resid [batch][4] =
 * r_prim | r_dual | s_prim | s_dual of every problem's last update in the latest constrained solve / box adjoint (ndlqr.h:
 * ndlqr_CopyBatchBoxResiduals, ndlqr_CopyBatchBoxAdjointResiduals), same destinations; they refuse unless the resident
 * solution is that of a constrained solve / has a box adjoint. */
int ndlqr_hip_solve_box_ex(NdlqrHipCtx* ctx, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                           int check_every, int warm_start, int* iters, int* status, int adapt_every, double rho_min,
                           double rho_max);
int ndlqr_hip_download_box_penalties(NdlqrHipCtx* ctx, double* rho);
int ndlqr_hip_download_box_residuals(NdlqrHipCtx* ctx, double* resid);
int ndlqr_hip_download_box_adjoint_residuals(NdlqrHipCtx* ctx, double* resid);
/* Infeasibility detection of the constrained solve (ndlqr.h: ndlqr_BatchSetInfeasibilityDetection,
 * ndlqr_CopyBatchInfeasibilityCertificate). ndlqr_hip_set_box_infeasibility takes the resolved
 * setting (every >= 0, 0: off; eps > 0 and finite) for the solves that follow. ndlqr_hip_download_infeasibility_certificate:
 * dlam [batch][N][n], dmu_x [batch][N][n], dmu_u [batch][N][m] of the latest constrained solve (each may be NULL; host,
 * pinned or this device's memory); zero rows for every problem that did not end as 4.
 * ndlqr_hip_download_infeasibility_measures: measures [batch][4], iteration [batch] of every problem's latest check
 * (ndlqr.h: ndlqr_CopyBatchInfeasibilityMeasures), with the same refusals and destinations. */
int ndlqr_hip_set_box_infeasibility(NdlqrHipCtx* ctx, int every, double eps);
int ndlqr_hip_download_infeasibility_certificate(NdlqrHipCtx* ctx, double* dlam, double* dmu_x, double* dmu_u);
int ndlqr_hip_download_infeasibility_measures(NdlqrHipCtx* ctx, double* measures, int* iteration);
/* Anderson acceleration of the constrained solve (ndlqr.h: ndlqr_BatchSetBoxAcceleration, ndlqr_CopyBatchBoxAcceleration;
 * DESIGN.md section 3.15). ndlqr_hip_set_box_acceleration takes the resolved setting (mem 0 .. 16, 0: off; safeguard and
 * reg > 0 and finite) for the solves that follow. ndlqr_hip_download_box_acceleration: accepted, rejected, columns [batch]
 * and gamma [batch][mem] of the latest constrained solve, which ran with acceleration on (each may be null, not all;
 * host, pinned or this device's memory); refuses as ndlqr_hip_download_infeasibility_measures does. */
int ndlqr_hip_set_box_acceleration(NdlqrHipCtx* ctx, int mem, double safeguard, double reg);
int ndlqr_hip_download_box_acceleration(NdlqrHipCtx* ctx, int* accepted, int* rejected, double* gamma, int* columns);
int ndlqr_hip_download_bound_multipliers(NdlqrHipCtx* ctx, double* mu_x, double* mu_u);
unsigned long long ndlqr_hip_factor_count(const NdlqrHipCtx* ctx);
/* Gradients through the box-constrained solve (ndlqr.h: ndlqr_SolveBatchBoxAdjoint, ndlqr_BatchBoundGradients;
 * DESIGN.md section 3.10). ndlqr_hip_solve_box_adjoint takes the resolved settings (the forward's final penalties, a cold start) and
 * blocks; g as for ndlqr_hip_solve_adjoint, iters / status [batch] may be NULL. Afterwards ndlqr_hip_download_adjoint and
 * ndlqr_hip_gradients read its w as they read a plain adjoint. ndlqr_hip_bound_gradients: dL/d(xlo, xhi, ulo, uhi) in the
 * flat layout, per problem or (summed) over the batch, [N][n] / [N][m]; NULL = not computed. */
int ndlqr_hip_solve_box_adjoint(NdlqrHipCtx* ctx, const double* g, double alpha, double eps_abs, double eps_rel, int max_iter,
                                int check_every, int* iters, int* status);
int ndlqr_hip_bound_gradients(NdlqrHipCtx* ctx, int summed, double* gxlo, double* gxhi, double* gulo, double* guhi);
/* Active-set polish of the latest constrained solve (ndlqr.h: ndlqr_PolishBatchBoxConstrained).
 * ndlqr_hip_polish_box takes the resolved settings (sigma > 0, 1 <= max_steps <= 32, max_rounds >= 0) and blocks; steps /
 * status [batch] may be NULL (host, pinned or this device's memory). ndlqr_hip_download_polish_codes: the entry codes of
 * the latest polish, [batch][N][n+m] bytes into host memory (0 unbounded, 1 free, 2 at the lower bound, 3 at the upper). */
int ndlqr_hip_polish_box(NdlqrHipCtx* ctx, double sigma, int max_steps, int max_rounds, int* steps, int* status);
/* ... and its adjoint on the remembered polish factorisation (ndlqr.h: ndlqr_SolveBatchPolishedAdjoint): g as for
 * ndlqr_hip_solve_adjoint (host, pinned or this device's memory), 1 <= max_steps <= 32; blocks. Afterwards
 * ndlqr_hip_download_adjoint, ndlqr_hip_gradients and ndlqr_hip_bound_gradients read its w and nu. */
int ndlqr_hip_solve_polished_adjoint(NdlqrHipCtx* ctx, const double* g, int max_steps, int* steps, int* status);
/* developer / test hook, not for production use (a blocking copy and a repack on the host): the entry codes */
int ndlqr_hip_download_polish_codes(NdlqrHipCtx* ctx, unsigned char* codes);
/* Several right-hand sides per problem against one kept factorisation each (the reference's NdData holds a single
 * right-hand side, src/nddata.h:70-75): nrhs sets of right-hand sides for the whole batch, flat HOST arrays in the layout of
 * ndlqr_BatchSetRhsFlat with a leading [nrhs] -- q, d [nrhs][batch][N][n], r [nrhs][batch][N][m], x0 [nrhs][batch][n] --,
 * solutions [nrhs][batch][nvars] into soln. Needs the records of a solve with NDLQR_FLAG_KEEP_RECORDS on a size-specialised
 * shape in the level-per-launch form (batch x N / 4 > 2048 or NDLQR_TREE=0), else NDLQR_ERR_INVALID. Blocking;
 * ndlqr_hip_last_solve_ms then reports the device time of the solve kernels alone. */
int ndlqr_hip_solve_multi_rhs(NdlqrHipCtx* ctx, int nrhs, const double* q, const double* r, const double* d,
                              const double* x0, double* soln);
/* ... of which only knots [knot0, knot0 + nknots), blocks `blocks` (NDLQR_SOLN_*) are computed and brought down:
 * out = [nrhs][batch][nknots][width] (u of knot 0 for a thousand sampled initial states of one model: 32 KB instead of 59 MB) */
int ndlqr_hip_solve_multi_rhs_slices(NdlqrHipCtx* ctx, int nrhs, const double* q, const double* r, const double* d,
                                     const double* x0, int knot0, int nknots, unsigned blocks, double* out);

/* One MPC step, asynchronous: a new right-hand side up (flat host arrays in the reference's layout: q, d
 * [batch][N][n], r [batch][N][m], x0 [batch][n] -- what ndlqr_InitializeWithLQRProblem reads from the problem,
 * src/solver.c:141-190), packed and negated by a kernel, factor + solve, the solutions [batch][nvars] (the layout of
 * ndlqr_hip_download_solutions, src/solve.c:192-201) down into `soln`. q, r, d may each be NULL: that part of the
 * right-hand side stays what its most recent writer left -- an upload, the device-side packing or an earlier step (an
 * MPC iteration often replaces x0 alone). There is ONE logical right-hand side; each buffer set of the pipeline has a
 * copy, and a solve or step that lands on a set whose copy is behind in a part it does not itself replace first
 * copies that part over (only a change of flow does: full steps followed by x0-only steps, a plain solve behind
 * steps). Everything is ordered on the stream of the
 * step's buffer set, so with the two-deep pipeline the copies of one step run beside the kernels of the other. Give
 * pinned host memory (ndlqr_hip_host_alloc): copies from / to pageable memory are staged by the runtime and block.
 * Pointers into THIS device's memory are taken as they are -- the pack kernels read q, r, d, x0 and write `soln` there
 * directly, nothing crosses the host link: the step of a loop whose states and inputs live on the GPU.
 * `soln` of a step is complete after ndlqr_hip_synchronize (every step) or, one step behind,
 * ndlqr_hip_synchronize_previous (the step before the most recent one; NDLQR_ERR_NOT_SPD when that step met a
 * non-positive pivot). */
int ndlqr_hip_step_async(NdlqrHipCtx* ctx, const double* q, const double* r, const double* d, const double* x0,
                         double* soln);
int ndlqr_hip_synchronize_previous(NdlqrHipCtx* ctx);
/* What a step brings down (ndlqr.h: ndlqr_BatchSetStepSelection) / the same slice of the latest solve, synchronously. */
int ndlqr_hip_set_step_selection(NdlqrHipCtx* ctx, int knot0, int nknots, unsigned blocks);
/* Factor + solve of the resident problems delivering a slice alone (ndlqr.h: ndlqr_SolveBatchSlicesAsync). */
int ndlqr_hip_solve_slices_async(NdlqrHipCtx* ctx, int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_hip_download_selection(NdlqrHipCtx* ctx, int knot0, int nknots, unsigned blocks, double* out);
/* The same three for a DENSE-COST problem (ndlqr_hip_init_dense; DESIGN.md section 3.16, "The asynchronous step"), all in
 * the caller's variables. ndlqr_hip_step_dense_async is ndlqr_hip_step_async with S' on the way up and S on the way down,
 * each by one kernel between the caller's arrays and the device layout on the step's stream (cost_pack_rhs,
 * cost_deliver_slice): x0 and `out` are required, q and r are replaced together or not at all (q~ = L^-1 (q - G' r) needs
 * both), d may be NULL; an x0-only step touches one knot per problem. The slice is an argument: knots
 * [knot0, knot0 + nknots), blocks = NDLQR_SOLN_* (with NDLQR_SOLN_ONLY nothing but those knots is computed), out
 * [batch][nknots][width]; nknots == 0: the whole vectors [batch][nvars]. u is computed from both reduced blocks whether or
 * not the state block is selected; u of the last knot comes out as zero. Memories, the two steps in flight,
 * ndlqr_hip_synchronize / ndlqr_hip_synchronize_previous and the re-solve under NDLQR_FLAG_KEEP_RECORDS are those of the
 * plain step. ndlqr_hip_solve_slices_dense_async / ndlqr_hip_download_selection_dense: the twins of the two slice functions.
 * All three refuse by name (NDLQR_ERR_INVALID, the message opens with the function's name) outside dense-cost mode, in
 * constrained mode (ndlqr_hip_init_constrained), on a time-axis shard, for another device's memory and for a slice that is
 * none. ndlqr_hip_download_cost_reduction keeps reporting the reduced right-hand side of the latest initialiser /
 * ndlqr_hip_set_rhs_dense: steps write the device right-hand side directly. */
int ndlqr_hip_step_dense_async(NdlqrHipCtx* ctx, const double* q, const double* r, const double* d, const double* x0,
                               int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_hip_solve_slices_dense_async(NdlqrHipCtx* ctx, int knot0, int nknots, unsigned blocks, double* out);
int ndlqr_hip_download_selection_dense(NdlqrHipCtx* ctx, int knot0, int nknots, unsigned blocks, double* out);
/* Read-out for the tests, every mode: the latest right-hand side as it lies on the device -- [batch][N'][2 n' + m'] in the
 * device's block sizes and horizon, pad rows and tail knots included, ndlqr_hip_rhs_raw_doubles of them -- into HOST
 * memory. Waits for everything in flight and brings the current buffer set's copy up to date first. */
int ndlqr_hip_download_rhs_raw(NdlqrHipCtx* ctx, double* out);
size_t ndlqr_hip_rhs_raw_doubles(const NdlqrHipCtx* ctx);
/* Time-axis sharding: ONE problem (or a small batch) solved by G ranks, each working on a chunk of
 * N / G consecutive knots of the horizon -- for jobs with fewer problems than GPUs; the batch axis stays the sharding
 * unit otherwise. Every rank holds the whole problem's inputs (upload as usual) and runs, for its chunk g:
 *     ndlqr_hip_time_shard_factor(ctx, g, G)      bottom kernel + the tree levels inside the chunk (asynchronous)
 *     ndlqr_hip_time_shard_export(ctx, G, buf)    the G - 1 accumulator slots between the chunks, packed
 *                                                 [G - 1][batch][slot] (ndlqr_hip_time_shard_top_doubles); waits
 *     -- the caller sums `buf` over the ranks: one all-reduce (RCCL over xGMI when every rank has its own GPU) --
 *     ndlqr_hip_time_shard_import(ctx, G, buf)
 *     ndlqr_hip_time_shard_finish(ctx, g, G)      the top log2(G) levels (redundantly on every rank: no multipliers
 *                                                 travel back), top-down sweep, back-substitution of the chunk
 * followed by ndlqr_hip_synchronize. The solution array then holds the knots [g N / G, (g + 1) N / G) of every problem
 * (ndlqr_hip_download_solutions hands back whole vectors: the other knots are stale). buf: host or device memory.
 * Default fast mode, size-specialised block sizes with a matrix-core instance, G a power of two, N / G >= 16,
 * N <= 64 K / (8 n) knots. The loop being split: src/solve.c:68-134 (factor), :137-182 (solve). */
int ndlqr_hip_time_shard_top_doubles(NdlqrHipCtx* ctx, int G);
int ndlqr_hip_time_shard_factor(NdlqrHipCtx* ctx, int g, int G);
int ndlqr_hip_time_shard_export(NdlqrHipCtx* ctx, int G, double* buf);
int ndlqr_hip_time_shard_import(NdlqrHipCtx* ctx, int G, const double* buf);
int ndlqr_hip_time_shard_finish(NdlqrHipCtx* ctx, int g, int G);
/* Pinned host memory for the transfer functions (hipHostMalloc): copies from / to it are asynchronous and run at the
 * rate of the host link. NULL when no device / no memory. */
void* ndlqr_hip_host_alloc(size_t bytes);
void ndlqr_hip_host_free(void* p);
/* device memory of the current device / a synchronous copy between any two of host, pinned and device memory: for
 * callers without HIP headers whose MPC loop lives on the GPU (ndlqr_hip_step_async takes device pointers) */
void* ndlqr_hip_device_alloc(size_t bytes);
void ndlqr_hip_device_free(void* p);
int ndlqr_hip_copy(void* dst, const void* src, size_t bytes);

/* D2H. soln: count*nvars doubles, nvars = (2n+m)N - m (src/solve.c:192-201).
 * fact: one problem, converted to the reference's NdData layout, N*K*(2n+m)*n doubles. */
int ndlqr_hip_download_solutions(NdlqrHipCtx* ctx, int p0, int count, double* soln);
int ndlqr_hip_download_rhs_blocks(NdlqrHipCtx* ctx, int p, double* z_full); /* N*(2n+m) */
int ndlqr_hip_download_factors(NdlqrHipCtx* ctx, int p, double* fact); /* needs NDLQR_FLAG_KEEP_FACT */
int ndlqr_hip_factors_valid(const NdlqrHipCtx* ctx); /* 1: the device holds the factor array of the last solve */
/* Solutions of the whole batch packed as [batch][nvars] into DEVICE memory `dst` (e.g. the send
 * buffer of an RCCL all_gather of the shards' solutions), by a kernel on the context's stream. */
int ndlqr_hip_pack_solutions_device(NdlqrHipCtx* ctx, double* dst);
/* Residual of the resident solution against the raw problem, per problem, computed on the device:
 * res[b] = ||K z - b||_2, bnorm[b] = ||b||_2 (bnorm may be NULL); the rows are those of the
 * reference's KKT system (src/solver.c:122-194). batch doubles each. */
int ndlqr_hip_kkt_residual(NdlqrHipCtx* ctx, double* res, double* bnorm);
int ndlqr_hip_cholesky_failures(NdlqrHipCtx* ctx);
/* The per-problem failure words, counts[0 .. batch): how often a kernel flagged problem b (a weight that is not
 * positive where the weights are staged, a Cholesky pivot that is not positive and finite). The words are the device's
 * own: CUMULATIVE since the context was created, or since the recovery of a solve that did not launch or complete zeroed
 * them -- take the difference between two calls for the count of the solves between them. One problem may be flagged
 * several times by one solve (at the separator that meets the bad data and at its ancestors; a block of the top chain,
 * which stands for several tree levels in one launch, adds one count per level it stands for). Waits for everything in
 * flight; does not change what ndlqr_hip_cholesky_failures reports. */
int ndlqr_hip_download_failure_counts(NdlqrHipCtx* ctx, int* counts);
/* Name of the launch sequence the last solve used (for reports): "reduced", "reduced-fused2" (the (12,4) instance; NDLQR_FUSE2=1/0), "reduced-tree",
 * "reduced-records", "knot-lean", "knot-strict", "knot-keep", "generic-reduced",
 * "generic-reduced-records", "generic-lean",
 * "generic-strict", "generic-keep" (DESIGN.md section 3). */
const char* ndlqr_hip_schedule(const NdlqrHipCtx* ctx);
/* 1 when the last solve wrote compact records (the Cholesky factor alone, packed) for the level-1 separators as well
 * as for level 0 ("reduced" / "reduced-fused2" at the instances where that is the default; NDLQR_COMPACT1=1/0), else 0:
 * the schedule name does not tell. */
int ndlqr_hip_compact_level1(const NdlqrHipCtx* ctx);
/* 1 when the fused bottom launch of the last solve took the two level-1 separators of a workgroup through one Cholesky
 * pass ("reduced-fused2" with compact level-1 records: the default of the (12,4) instance; NDLQR_PAIR1=1/0), else 0. The records are the same either way. */
int ndlqr_hip_level1_paired(const NdlqrHipCtx* ctx);
/* 1 when that paired launch ran in its 16 KB LDS layout (ten workgroups per CU instead of eight; the level-2 separator's
 * slots are stored once, without atomic adds; NDLQR_BOTTOM_LDS16=1/0, unset: by instance), else 0 -- "not applied". The
 * records and the solutions are the same either way. */
int ndlqr_hip_bottom_lds16(const NdlqrHipCtx* ctx);
/* 1 when the last solve eliminated the separators of its top tree levels (level >= max(3, K - 5)) as one block-tridiagonal
 * chain per problem in a single launch ("reduced" / "reduced-fused2" without kept records; NDLQR_TOP_CHAIN=1/0, unset: by
 * instance), else 0: the schedule name does not tell. The solutions agree to rounding, not bit for bit. */
int ndlqr_hip_top_chain(const NdlqrHipCtx* ctx);

/* Per-kernel profile (NDLQR_FLAG_PROFILE): HIP-event durations accumulated since the last
 * reset, one slot per kernel kind. Returns number of slots / fills name, total ms, launches. */
int ndlqr_hip_profile_slots(NdlqrHipCtx* ctx);
int ndlqr_hip_profile_get(NdlqrHipCtx* ctx, int slot, char* name, int name_cap, double* total_ms,
                          int* launches);
int ndlqr_hip_profile_reset(NdlqrHipCtx* ctx);

/* Dense helpers behind Matrix* of ndlqr.h (src/linalg.c:55-190 -> src/linalg_custom.c).
 * Host pointers in, host pointers out; column-major. Return 0, or -1 for a failed Cholesky. */
int ndlqr_hip_gemm(int tA, int tB, int m, int n, int k, double alpha, const double* A, int lda,
                   const double* B, int ldb, double beta, double* C, int ldc);
int ndlqr_hip_potrf_lower(int n, double* A, int lda);
int ndlqr_hip_potrs_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb);
/* one triangular substitution alone: L x = b (transposed = 0) or L' x = b (clap_LowerTriBackSub,
 * src/linalg_custom.c:113-132) */
int ndlqr_hip_trsv_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb, int transposed);

#ifdef __cplusplus
}
#endif
#endif /* NDLQR_HIP_H_ */
