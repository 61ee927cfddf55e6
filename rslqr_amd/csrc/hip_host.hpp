// hip_host.hpp -- internal: what a feature unit (hip_grad.hip, hip_box.hip, hip_refine.hip, hip_cost.hip,
// hip_dense.hip) may use from the core (ndlqr_hip.hip) and from the other features. Declarations only, like
// hip_context.hpp; nothing here is an exported symbol. Every __global__ kernel is compiled into exactly one unit: a
// unit that needs another unit's kernel calls the host function declared here and does not include the kernel header
// a second time.
#pragma once
#include "hip_context.hpp"

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------ errors (ndlqr_hip.hip)
// records the message for ndlqr_hip_last_error(), prints it, returns NDLQR_ERR_INVALID
int refuse(const std::string& msg);
int fail(const char* what, hipError_t e);  // = ndlqr_hip_fail

// ------------------------------------------------------------------------------ guards (ndlqr_hip.hip)
// entry points that are not carried through a padded horizon / dense-cost mode refuse with `who` in the message
int need_unpadded_horizon(const NdlqrHipCtx* c, const char* who);
int need_diagonal_cost(const NdlqrHipCtx* c, const char* who);
// consumers of the whole solution vector refuse a slice, and a failed constrained solve
int need_full_solution(const NdlqrHipCtx* c, const char* who);
// is there an adjoint of the resident solution of the resident inputs?
int need_adjoint(const NdlqrHipCtx* c, const char* who);

// ------------------------------------------------------------------------------ caller memory
// Where a caller's array lives. A pointer the runtime does not know (an ordinary malloc'ed one is "invalid value" to older
// runtimes) is pageable host memory.
enum class Where { Pageable, Pinned, OwnDevice, OtherDevice };
Where where(const void* p, int device);

// The caller's arrays: this device's memory is taken as it is, host memory (pinned or pageable) is staged through HBM, and
// another device's memory is refused (the caller has the wrong device, and a silent copy would hide it).
// K arrays of the caller, cnt[k] doubles each (null: absent), and their way through grad_stage. In this order: classify();
// grad_stage.grow for `stage` doubles plus whatever the caller wants behind them; sync_all; place(), which fills dev[] --
// what the kernels get -- and returns the first free double; copy(st, true) before the launches that read inputs, or
// copy(st, false) behind those that wrote outputs.
template <int K>
struct CallerArrays {
  double* user[K];
  size_t cnt[K];
  bool own[K] = {};  // this device's memory: read or written by the kernels as it is
  double* dev[K] = {};
  size_t stage = 0;  // doubles to stage
  // `who`: the API function, `what`: "an output lies", ... -- the refusal reads "who: what in the memory of another device ..."
  int classify(const NdlqrHipCtx* c, const char* who, const char* what) {
    for (int k = 0; k < K; ++k) {
      if (!user[k]) continue;
      const Where w = where(user[k], c->device);
      if (w == Where::OtherDevice)
        return refuse(std::string(who) + ": " + what + " in the memory of another device than the solver's");
      own[k] = w == Where::OwnDevice;
      if (!own[k]) stage += cnt[k];
    }
    return NDLQR_OK;
  }
  double* place(const NdlqrHipCtx* c) {
    double* at = c->grad_stage;
    for (int k = 0; k < K; ++k) {
      if (!user[k]) continue;
      dev[k] = own[k] ? user[k] : at;
      if (!own[k]) at += cnt[k];
    }
    return at;
  }
  int copy(hipStream_t st, bool in) {
    for (int k = 0; k < K; ++k)
      if (user[k] && !own[k])
        HIP_TRY(hipMemcpyAsync(in ? dev[k] : user[k], in ? user[k] : dev[k], sizeof(double) * cnt[k], hipMemcpyDefault, st));
    return NDLQR_OK;
  }
};

// KERNEL<true> under NDLQR_FLAG_STRICT_FP, KERNEL<false> otherwise: one argument list for both
#define launch_strict(strict, KERNEL, grid, block, lds, stream, ...)                            \
  do {                                                                                          \
    if (strict) hipLaunchKernelGGL(KERNEL<true>, grid, block, lds, stream, __VA_ARGS__);        \
    else hipLaunchKernelGGL(KERNEL<false>, grid, block, lds, stream, __VA_ARGS__);              \
  } while (0)

// iters / status of a constrained solve or its adjoint (`who`) go to host memory or this device's
int refuse_foreign_iters_status(const NdlqrHipCtx* c, const char* who, const int* iters, const int* status);
// The per-problem iteration counts and status words behind everything enqueued on st, for the caller (null: not asked
// for); a problem still running at max_iter (0) reports 2: the last iterate. Synchronises st.
int deliver_iters_status(const NdlqrHipCtx* c, hipStream_t st, const int* d_iters, const int* d_status, int* iters, int* status);

// ------------------------------------------------------------------------------ pipeline services (ndlqr_hip.hip)
// every solve in flight on either set has finished
hipError_t sync_all(NdlqrHipCtx* c);
// the current set's copy of the right-hand side is brought up to date in the parts of `need` (bits: q, r, d, x0)
int rhs_make_current(NdlqrHipCtx* c, unsigned need);
// the flat q, r, d, x0 (this device's memory, the caller's layout) packed into the current set's right-hand side, on its stream
hipError_t launch_pack_rhs(NdlqrHipCtx* c, const double* q, const double* r, const double* d, const double* x0);
// everything is idle and the current set's whole right-hand side has just been rewritten
void note_new_rhs(NdlqrHipCtx* c);
// the current buffer set holds the most recent solution
void note_solution(NdlqrHipCtx* c);
// the device time between the events of the (synchronised) set, for ndlqr_hip_last_solve_ms
void note_elapsed(NdlqrHipCtx* c, const BufferSet& s);
// the right-hand-side columns of the kept records / slots, saved before (restore false) and restored after a re-solve that
// is not the primal's (AdjointState::save)
hipError_t adjoint_scratch(NdlqrHipCtx* c, bool restore);
// the re-solve on what the last factorisation kept: the records where they have one, else the factor array; refused with
// `refusal` when there are records only and this shape / horizon has no record-based re-solve
int launch_resolve(NdlqrHipCtx* c, const double* rhs, double* z, const char* refusal);
// What is resident factored on the primary set as a plain solve does it (the resident solution is overwritten), with the
// pivot check: *not_spd = NDLQR_ERR_NOT_SPD, which is returned, when a pivot was not positive.
// (who, what: the entry point and the matrix, for the message)
int factor_resident(NdlqrHipCtx* c, hipStream_t st, int* not_spd, const char* who, const char* what);
// Packs the solutions of `count` problems from the blocks [count][N][2n+m] at z into dst: the whole vectors [count][nvars],
// or the slice `sel` [count][nknots][width]. u: the caller's block sizes, d: the device layout.
hipError_t launch_pack(const ndlqr::Dims& u, const ndlqr::Dims& d, const KnotSlice& sel, const double* z, double* dst,
                       hipStream_t st, unsigned count);
// Solutions of problems [p0, p0 + count) of the blocks [batch][N][2n+m] at zsrc as [count][nvars] into host memory
int download_packed(NdlqrHipCtx* c, const double* zsrc, int p0, int count, double* soln);

// ------------------------------------------------------------------------------ what one feature offers another
// hip_refine.hip: r = b - K (z (+) delta) in double-double on the current set's stream (norms == nullptr: the vector
// alone). QR: the diagonal to use -- the polish passes the saved, unshifted one --, r: the destination
int launch_residual_dd_on(NdlqrHipCtx* c, const double* QR, const double* rhs, const double* z, const double* delta,
                          double* r, unsigned long long* norms, int nslots, int slot);
// hip_cost.hip, dense-cost mode: `vec`, the packed [count][nvars] vectors of problems [p0, p0 + count) in the reduced
// variables, becomes the same in the caller's (S, in place)
hipError_t cost_map_back(NdlqrHipCtx* c, double* vec, int p0, unsigned count, hipStream_t st);
// ... the same launch without the phase timing of NDLQR_FLAG_PROFILE (which waits): what an asynchronous step uses
hipError_t cost_apply_on(NdlqrHipCtx* c, double* vec, int p0, unsigned count, hipStream_t st);
// ... the asynchronous step's way up: S' of the parts `parts` (bits q 1, r 2 -- together --, d 4, x0 8) of the caller's flat
// q, r, d, x0 (device-readable; a part not replaced may be null) straight into the device right-hand side `rhs`
hipError_t cost_pack_rhs_on(NdlqrHipCtx* c, unsigned parts, const double* q, const double* r, const double* d, const double* x0,
                            double* rhs, hipStream_t st);
// ... and its way down: S of the non-empty slice `sel` of the reduced solutions z (device layout) into dst
// [batch][nknots][width] (this device's memory)
hipError_t cost_deliver_slice_on(NdlqrHipCtx* c, const KnotSlice& sel, const double* z, double* dst, hipStream_t st);
// ... and the packed [batch][nvars] vector `vec` in the caller's variables becomes S' vec (in place): the adjoint's g
hipError_t cost_reduce_vector(NdlqrHipCtx* c, double* vec, hipStream_t st);
// ... S' (records `rec`) of the flat right-hand side q, r, d, x0 (device) into the flat arrays qt, rt, dt, x0t
hipError_t cost_reduce_rhs_to(NdlqrHipCtx* c, const double* rec, const double* q, const double* r, const double* d,
                              const double* x0, double* qt, double* rt, double* dt, double* x0t, hipStream_t st);
// ... the reduction of the dense costs Q, H (null: zero), R and of A, B (device, flat): records into rec, A~, B~ into At, Bt
hipError_t cost_reduce_problem(NdlqrHipCtx* c, const double* A, const double* B, const double* Q, const double* H,
                               const double* R, double* rec, double* At, double* Bt, hipStream_t st);
// hip_grad.hip: the caller's packed g [batch][nvars] (this device's memory) into the adjoint's resident right-hand side
hipError_t launch_adjoint_rhs(NdlqrHipCtx* c, const double* g, hipStream_t st);

#pragma GCC visibility pop
