// hip_context.hpp -- internal: the device context behind NdlqrHipCtx* and the launch-profiling
// helper, shared by every unit of the HIP host layer: the core (ndlqr_hip.hip), the feature units (hip_*.hip; what they
// share beyond the context: hip_host.hpp) and the per-instance units (small_instance.hip, reduced_instance.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "ndlqr.h"
#include "ndlqr_hip.h"

#include "kernels_common.hpp"

// records the message for ndlqr_hip_last_error(), prints it, returns NDLQR_ERR_NO_DEVICE (or
// NDLQR_ERR_INVALID for a rejected launch configuration / argument)
#pragma GCC visibility push(hidden)
int ndlqr_hip_fail(const char* what, hipError_t e);
struct NdlqrHipCtx;
int ndlqr_hip_ensure_F(NdlqrHipCtx* c);
#pragma GCC visibility pop
#define HIP_TRY(expr)                                                  \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess) return ndlqr_hip_fail(#expr, e_);            \
  } while (0)

// LDS of a workgroup on gfx950, and the dynamic LDS a kernel gets without asking for more
constexpr size_t kLdsMax = 160 * 1024;
constexpr size_t kLdsDefaultDynamic = 64 * 1024;
// ... and the asking, before a launch with `lds` bytes of dynamic LDS
template <class Kernel>
static inline hipError_t allow_dynamic_lds(Kernel* kernel, size_t lds) {
  if (lds <= kLdsDefaultDynamic) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// ------------------------------------------------------------------------------ context

enum { SLOT_LEAF = 0, SLOT_SEP, SLOT_SCHUR, SLOT_BOUNDARY, SLOT_APPLY, SLOT_BOTTOM, SLOT_UPPER, SLOT_TOP, SLOT_COUNT };

struct PendingEvent {
  int slot;
  hipEvent_t start, stop;
};

// The kernels a solve runs (plan_solve): a size-specialised instance (launch_small.hpp), the
// runtime-sized separator-only schedule (launch_reduced_generic) or the knot-based runtime-sized one (launch_generic)
enum class Family { None, Small, GenericReduced, GenericKnot };

// What the last factorisation left on the primary set (kept records and factors never pipeline), as the plain API's
// re-solves see it: they run the kernels of the family that wrote the records, whatever the flags say by then
struct KeptState {
  Family family = Family::None;  // whose records / slots these are
  bool time_shard = false;       // ... those of one chunk of a time-axis shard (launch_time_shard): no re-solve
  bool rec_complete = false;  // every separator record and factor is there (fast mode + KEEP / KEEP_RECORDS)
  bool rec_compact = false;   // ... in the compact form of the default schedule (level-0 records = L, the factors of the upper
                              // separators in the slack of those slots): the re-solve is rb_forward / rb_forward_top / rb_backsub
  bool fact_valid = false;    // the device holds a complete factorisation (last solve ran with KEEP_FACT)
  const char* schedule = "none";  // name of the launch sequence the last solve used (ndlqr_hip_schedule)
  bool rec1_compact = false;      // ... and it left compact level-1 records (SmallPlan::compact1; ndlqr_hip_compact_level1)
  bool level1_paired = false;     // ... through the paired level-1 pass (SmallPlan::pair1; ndlqr_hip_level1_paired): the records are the same
  bool bottom_lds16 = false;      // ... in the 16 KB LDS layout of that launch (SmallPlan::lds16; ndlqr_hip_bottom_lds16)
  bool top_chain = false;         // ... with the separators of the top levels as one block-tridiagonal chain (SmallPlan::chain; ndlqr_hip_top_chain)
  // the records / factors no longer belong to the resident inputs: the re-solves refuse until the next solve
  void forget_factorisation() { rec_complete = fact_valid = false; }
};

// A launch sequence captured as a hipGraph and the key it was captured under (replayed while that matches; the key
// determines the SolvePlan, and with it what the sequence leaves behind)
struct CapturedChain {
  hipGraphExec_t exec = nullptr;
  unsigned flags = 0;
  hipStream_t stream = nullptr;
  unsigned apply = 0;  // (apply_blk0 << 16 | apply_nblk): the restricted back-substitution of a step
  void reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
  }
};

// A slice of every solution: knots [knot0, knot0 + nknots), of each the blocks of `blocks` (NDLQR_SOLN_*), packed
// [batch][nknots][width]. nknots == 0: the whole solution vectors, [batch][nvars].
struct KnotSlice {
  int knot0 = 0, nknots = 0;
  unsigned blocks = 7u;
  // a non-empty range of the N knots that names some block and sets no bit outside `allowed`
  bool valid(int N, unsigned allowed) const {
    return knot0 >= 0 && nknots > 0 && knot0 + nknots <= N && (blocks & 7u) && !(blocks & ~allowed);
  }
  size_t width(const ndlqr::Dims& u) const {
    return ((blocks & 1u) ? u.n : 0) + ((blocks & 2u) ? u.n : 0) + ((blocks & 4u) ? u.m : 0);
  }
  // doubles per problem
  size_t doubles(const ndlqr::Dims& u) const { return nknots > 0 ? width(u) * nknots : (size_t)u.rows * u.N - u.m; }
};

// (internal to the library: no inline member of the owners, the feature structs and the context is an exported symbol)
#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------ owned memory
// The two owners of the host layer's memory: DevBuf<T> (hipMalloc) and PinnedBuf<T> (hipHostMalloc). Move-only, freed by
// the destructor; they convert to T*, so kernel argument lists and pointer arithmetic read as with a raw pointer.
template <class T, bool PINNED>
class OwnedBuf {
  T* p_ = nullptr;
  size_t n_ = 0;  // capacity, elements

 public:
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }  // (o frees the old one)
  ~OwnedBuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }
  void reset() {
    if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; n_ = 0;
  }
  // first-use buffers of a fixed size: allocated when empty, left alone otherwise
  hipError_t ensure(size_t count) {
    if (p_) return hipSuccess;
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, sizeof(T) * count, hipHostMallocDefault)
                                : hipMalloc((void**)&p_, sizeof(T) * count);
    if (e != hipSuccess) p_ = nullptr;
    else n_ = count;
    return e;
  }
  // ... zero-filled at that allocation (device memory: on `st`, ordered before whatever that stream runs next)
  hipError_t ensure_zeroed(size_t count, hipStream_t st = nullptr) {
    if (p_) return hipSuccess;
    const hipError_t e = ensure(count);
    if (e != hipSuccess) return e;
    if (PINNED) { memset(p_, 0, sizeof(T) * count); return hipSuccess; }
    return hipMemsetAsync(p_, 0, sizeof(T) * count, st);
  }
  // room for `count` elements: freed and allocated again when too small (the old contents go)
  hipError_t grow(size_t count) {
    if (count <= n_) return hipSuccess;
    reset();
    return ensure(count);
  }
};
template <class T> using DevBuf = OwnedBuf<T, false>;
template <class T> using PinnedBuf = OwnedBuf<T, true>;

// doubles of the device arrays every feature sizes its buffers by
static inline size_t doubles_QR(const ndlqr::Dims& d) { return (size_t)d.batch * d.N * d.w; }
static inline size_t doubles_z(const ndlqr::Dims& d) { return (size_t)d.batch * d.N * d.rows; }
static inline size_t doubles_F(const ndlqr::Dims& d) { return (size_t)d.batch * d.K * d.N * d.fb; }
// first error of a list of allocations
static inline hipError_t first_error(std::initializer_list<hipError_t> list) {
  for (const hipError_t e : list) if (e != hipSuccess) return e;
  return hipSuccess;
}

// Everything a solve writes, and what orders it. The context holds two such sets: consecutive solves alternate between
// them, each on its own stream, so that the thinly populated upper-level kernels and the HBM-bound back-substitution of
// one solve run beside the ALU-bound bottom kernel of the next (only for schedules without cross-solve state: no factor
// array, no kept records).
struct BufferSet {
  DevBuf<double> rec;   // [batch][N][2 n^2 + n] separator records f_a | f_bb | z_sep (compact forms use the front of a record and its last n entries)
  DevBuf<double> red;   // accumulators of the separator-only schedules: [batch][N/4][slot] (size-specialised shapes, allocated with the set) or [batch][N/2][4 n^2 + 2 n] (runtime-sized schedule, on its first solve)
  DevBuf<double> ytop;  // [batch][N/8][n] multipliers of the separators of level >= 3 (rb_backsub_top -> rb_backsub)
  DevBuf<double> z;
  DevBuf<double> rhs;   // this set's copy of the right-hand side (ndlqr_hip_step_async replaces it per step)
  DevBuf<double> xfer;  // transfer staging in HBM: flat q | r | d | x0 going up, packed [batch][nvars] coming down (allocated on first use)
  DevBuf<int> tree_cnt; // arrival counters of the separators of level >= 2, [batch][N / 4]; zero between solves (reset by the root's wavefront)
  PinnedBuf<int> h_fail;  // pinned host word: the batch-wide failure count, copied behind the last kernel of a solve
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  unsigned long long rhs_gen[4] = {};  // generations of this set's copy of the right-hand side (NdlqrHipCtx::rhs_latest)
  CapturedChain graph;     // the launch sequence of a solve on this set
  bool ready = false;      // allocated
  // `u`: the caller's block sizes (caller-layout data: max(flat right-hand side, packed solutions) doubles)
  hipError_t ensure_xfer(const ndlqr::Dims& u) { return xfer.ensure((size_t)u.batch * u.N * u.rows + (size_t)u.batch * u.n); }
};

// ------------------------------------------------------------------------------ one struct per feature
// The state of an optional feature: its buffers with their layout, its bookkeeping, and one ensure() that names the
// buffers and their sizes once (d: the device layout, st: the stream a zero-fill is ordered on). The entry point that
// first needs the feature calls it; the buffers go with the context. A new feature adds its struct here with a member in
// NdlqrHipCtx, its kernels_<feature>.hpp, its unit hip_<feature>.hip with the entry points (which call ensure()) and one
// line in HIP_UNITS of rslqr_amd/build.py -- nothing else, and nothing in the core unit ("Units").

// Developer switches of the environment, read once when the context is created (read_knobs, ndlqr_hip.hip)
struct DevKnobs {
  int rowbcast = -1;  // bottom levels of the separator-only schedule on the row-broadcast core (rb_bottom): NDLQR_ROWBCAST=1 always, 0 never (bottom_reduced_mc), unset (-1): by block size
  int tree = -1;  // tree schedule (bottom_reduced_mc<TREE>: one launch for the whole factorisation, wavefronts climbing on arrival counters): NDLQR_TREE=1 always, 0 never, unset (-1): when all bottom wavefronts are resident at once (small batches: fewer launches win; large ones: a launch per level is faster)
  int backsub_cols = -1;  // rb_backsub at nstates + ninputs <= 16: the body with [A | B] in registers (rb_backsub_cols, block 128) unless NDLQR_BACKSUB_COLS=0 asks for the LDS-staged one
  int fuse2 = -1;  // tree level 2 inside the bottom launch (bottom8_reduced_mc) instead of as a launch of its own: NDLQR_FUSE2=1 always, 0 never, unset (-1): where it measured faster -- the (12,4) instance (launch_small.hpp)
  int compact1 = -1;  // compact records (L alone, packed) for the level-1 separators too, substituted with by rb_backsub_cols: NDLQR_COMPACT1=1 wherever the kernels exist, 0 never, unset (-1): where it measured faster (launch_small.hpp)
  int pair1 = -1;  // one Cholesky pass for the two level-1 separators of a workgroup of the fused bottom launch (bottom8_reduced_mc<.., P1>): NDLQR_PAIR1=1 wherever fuse2 and compact1 hold, 0 never, unset (-1): where it measured faster -- the (12,4) instance (launch_small.hpp)
  int bottom_lds16 = -1;  // the paired fused bottom launch in at most 16 KB of LDS per workgroup, ten workgroups per CU (bottom8_reduced_mc<.., P1, L16>): NDLQR_BOTTOM_LDS16=1 wherever pair1 holds, 0 never, unset (-1): where it measured faster (launch_small.hpp)
  int top_chain = -1;  // the top levels of the separator-only schedule as one block-tridiagonal chain per problem (reduced_chain_top) instead of reduced_level_mc / reduced_top_mc: NDLQR_TOP_CHAIN=1 wherever the kernel exists and the schedule keeps no records, 0 never, unset (-1): where it measured faster -- horizons of 256 knots at six instances (launch_small.hpp)
  int pipeline = 2;         // NDLQR_PIPELINE: the pipeline depth a context starts with (NdlqrHipCtx::pipeline)
  bool no_top = false;      // NDLQR_NO_TOP=1: the last three tree levels as launches of their own (A/B timing of reduced_top_mc)
  bool top_levels_set = false;  // ... NDLQR_TOP_LEVELS was given (the chain stands back for an A/B of reduced_top_mc)
  int top_levels = 3;       // tree levels inside reduced_top_mc (NDLQR_TOP_LEVELS, 3 .. 5): beyond three a wavefront takes several separators of the first ones in turn
  bool no_mfma = false;     // NDLQR_NO_MFMA=1: keep the scalar Schur kernel for large blocks (A/B timing)
  int sep_threads = 0;        // NDLQR_SEP_THREADS: workgroup size of the matrix-core separator (0 = by block size)
  int mult_threads = 0;       // NDLQR_MULT_THREADS: workgroup size of backsub_multipliers_compact (0 = by block size)
  bool no_reduced_generic = false;  // NDLQR_DEV_NO_REDUCED_GENERIC (developer): A/B against the knot-based runtime-sized schedule
  bool no_pad = false;        // NDLQR_NO_PAD=1: the caller's block size on the device (A/B, tests)
  bool alt_priority_set = false;  // NDLQR_ALT_PRIORITY: stream priority of the alternate buffer set (unset: the greatest)
  int alt_priority = 0;
};

// Adjoint solve and parameter gradients (ndlqr_hip_solve_adjoint / ndlqr_hip_gradients): the adjoint right-hand side
// and its solution w in buffers of their own, [batch][N][2n+m], so that the primal state stays as it is. gen: the
// resident solution (NdlqrHipCtx::soln_gen) the adjoint belongs to (0: none); rhs_stamp: NdlqrHipCtx::rhs_stamp() when
// the plain or the constrained adjoint solve ended (ndlqr_hip_gradients_dense refuses a right-hand side replaced since).
struct AdjointState {
  DevBuf<double> rhs, z;
  DevBuf<double> save;  // right-hand-side columns of the kept records / slots, saved around a re-solve that is not the primal's
  unsigned long long gen = 0;
  unsigned long long rhs_stamp = 0;
  hipError_t ensure_save(const ndlqr::Dims& d) { return save.ensure(2 * (size_t)d.batch * d.N * d.n); }
  hipError_t ensure(const ndlqr::Dims& d, hipStream_t st) {
    // (z zeroed: the entries a re-solve does not write, the pad rows)
    return first_error({rhs.ensure(doubles_z(d)), z.ensure_zeroed(doubles_z(d), st), ensure_save(d)});
  }
};

// Box-constrained solve by ADMM (ndlqr_hip_set_bounds / ndlqr_hip_solve_box, kernels_box.hpp). Bounds lo | hi in the
// device layout [batch][N][n+m] ([N][n+m] when shared: bstride 0) and their bounded pattern; v, y and two ADMM
// right-hand sides (ping-pong) and the re-solve's z; per problem status, iterations and residuals (resid [batch][4] =
// r_prim | r_dual | sp | sd of its last update: the read-out of ndlqr_hip_download_box_residuals); rho: the penalty of
// every problem [batch]; word: running count | problems whose penalty changed | lo > hi | pattern changed (h_word: the
// same four, then the box adjoint's running count). The shifted factorisation is remembered (fact) with its penalties --
// rho, and rho_value when rho_uniform says they are all that one value -- and what the plain API's kept state was after
// it (kept), so that the next constrained solve may skip factoring. soln_gen: the solution generation the latest
// constrained solve left (0: none since the bounds were set).
struct BoxState {
  DevBuf<double> lo, hi, v, y, z, qr_save, rhs[2], resid, rho;
  DevBuf<unsigned char> mask;
  DevBuf<int> status, iters, word;
  PinnedBuf<int> h_word;
  bool shared = false, have_bounds = false, have_vy = false;
  size_t bstride = 0;      // doubles between the bounds of consecutive problems (0: shared)
  bool fact = false;       // the kept records / factors are those of QR + rho M of the current bounds pattern
  bool rho_uniform = false;
  double rho_value = 0.0;
  unsigned flags = 0;      // the flags of that factorisation
  KeptState kept;          // ... and what it left
  unsigned long long soln_gen = 0;
  hipError_t ensure(const ndlqr::Dims& d, hipStream_t st) {
    const size_t nz = doubles_z(d), nv = doubles_QR(d), nb = (size_t)d.batch;  // (bounds: room for per-problem ones, shared or not)
    return first_error({mask.ensure_zeroed(nv, st), lo.ensure(nv), hi.ensure(nv), word.ensure(4), h_word.ensure(5),
                        z.ensure_zeroed(nz, st),  // (entries a re-solve does not write: the pad rows)
                        v.ensure(nv), y.ensure(nv), qr_save.ensure(nv), rhs[0].ensure(nz), rhs[1].ensure(nz),
                        resid.ensure(4 * nb), status.ensure(nb), iters.ensure(nb), rho.ensure(nb)});
  }
};

// Infeasibility detection of the box-constrained solve (ndlqr_hip_set_box_infeasibility, kernels_box_infeas.hpp;
// DESIGN.md section 3.14). every, eps: the setting (every == 0: off -- nothing here is allocated or launched). The
// iteration before a check leaves copies of the re-solve's z, of y and of the penalties (z_prev [batch][N][2n+m], y_prev
// [batch][N][n+m], rho_prev [batch]); the certificate of every status-4 problem in the device block sizes, zero elsewhere
// (cert_lam [batch][N][n], cert_mu [batch][N][n+m]); the four numbers of every problem's latest check and the iteration
// it ran at (measures [batch][4], measured_at [batch]; zero for a problem no check examined). gen: the solution
// generation of the latest constrained solve that ran with detection on (0: none).
struct BoxInfeasState {
  DevBuf<double> z_prev, y_prev, rho_prev, cert_lam, cert_mu, measures;
  DevBuf<int> measured_at;
  int every = 0;
  double eps = 1e-4;
  unsigned long long gen = 0;
  hipError_t ensure(const ndlqr::Dims& d) {
    const size_t nv = doubles_QR(d);
    return first_error({z_prev.ensure(doubles_z(d)), y_prev.ensure(nv), rho_prev.ensure((size_t)d.batch),
                        cert_lam.ensure((size_t)d.batch * d.N * d.n), cert_mu.ensure(nv),
                        measures.ensure(4 * (size_t)d.batch), measured_at.ensure((size_t)d.batch)});
  }
};

// Anderson acceleration of the box-constrained solve (ndlqr_hip_set_box_acceleration, kernels_box_accel.hpp; DESIGN.md
// section 3.15). mem, safeguard, reg: the setting (mem == 0: off -- nothing here is allocated or launched). Scratch of
// one solve, zeroed or overwritten at its start: the ring of t and of g, ring_t, ring_g [batch][mem+1][N][n+m] (they
// grow with mem); the plain v+, y+ an accelerated step saves, pv, py [batch][N][n+m]; per problem the Gram matrix
// gram [batch][17][17], |g_prev| gprev [batch], gamma [batch][mem] of the latest accelerated step and the words
// meta [6][batch] (ring start, ring fill, accelerated, accepted, rejected, columns). gen: the solution generation of the
// latest constrained solve that ran accelerated (0: none), mem_solved: its memory -- what the read-out refers to.
struct BoxAccelState {
  DevBuf<double> ring_t, ring_g, pv, py, gram, gprev, gamma;
  DevBuf<int> meta;
  int mem = 0, mem_solved = 0;
  double safeguard = 1.0, reg = 1e-10;
  unsigned long long gen = 0;
  hipError_t ensure(const ndlqr::Dims& d) {
    const size_t nv = doubles_QR(d), nb = (size_t)d.batch;
    return first_error({ring_t.grow((size_t)(mem + 1) * nv), ring_g.grow((size_t)(mem + 1) * nv), pv.ensure(nv), py.ensure(nv),
                        gram.ensure(nb * 17 * 17), gprev.ensure(nb), gamma.ensure(nb * 16), meta.ensure(6 * nb)});
  }
};

// Gradients through the box-constrained solve (ndlqr_hip_solve_box_adjoint / ndlqr_hip_bound_gradients,
// kernels_box_grad.hpp). gen: the solution generation the box adjoint belongs to (0: none). The adjoint's own entry
// codes, v, y, ADMM right-hand sides (its resident one is adj.rhs, its solution adj.z), per problem status, iterations
// and residuals, and its running count: nothing of the forward's iteration state is touched.
struct BoxAdjointState {
  DevBuf<unsigned char> code;
  DevBuf<double> v, y, resid, rhs[2];
  DevBuf<int> status, iters, word;
  unsigned long long gen = 0;
  hipError_t ensure(const ndlqr::Dims& d) {
    const size_t nz = doubles_z(d), nv = doubles_QR(d), nb = (size_t)d.batch;
    return first_error({code.ensure(nv), v.ensure(nv), y.ensure(nv), rhs[0].ensure(nz), rhs[1].ensure(nz),
                        resid.ensure(4 * nb), status.ensure(nb), iters.ensure(nb), word.ensure(1)});
  }
};

// Iterative refinement (ndlqr_hip_refine, kernels_refine.hpp): the double-double residual and the correction in buffers
// of the right-hand side's layout, the norm slots [2][kRefineMaxSteps + 1][batch] (rho, then the scale, as bit patterns),
// what the caller gets (steps [batch], eta before | after [2 batch]) and, under NDLQR_FLAG_PROFILE, the device time of
// the residual kernels | re-solves | commits of the latest call.
constexpr int kRefineMaxSteps = 8;
struct RefineState {
  DevBuf<double> r, delta, eta;
  DevBuf<unsigned long long> norms;
  DevBuf<int> steps;
  double phase_ms[3] = {};
  static size_t norm_count(const ndlqr::Dims& d) { return 2 * (kRefineMaxSteps + 1) * (size_t)d.batch; }
  hipError_t ensure_r(const ndlqr::Dims& d) { return r.ensure(doubles_z(d)); }  // (ndlqr_hip_kkt_residual_vector: the residual alone)
  hipError_t ensure(const ndlqr::Dims& d, hipStream_t st) {
    return first_error({ensure_r(d), norms.ensure(norm_count(d)), steps.ensure((size_t)d.batch), eta.ensure(2 * (size_t)d.batch),
                        delta.ensure_zeroed(doubles_z(d), st)});  // (entries a re-solve does not write: the pad rows)
  }
};

// Active-set polish of a constrained solve (ndlqr_hip_polish_box, kernels_box_polish.hpp). Entry codes (bytes) and mu in
// the layout of the bounds; the accepted iterate z | mu | bt (bt: the right-hand side b - E_A' mu of the residual) and the
// candidate zc | muc | btc; z0: the resident solution as found (the factorisations overwrite it); r, delta: residual and
// correction; norms: the slots of one round, [2][kPolishMaxSteps + 1][batch] as RefineState's; sig [batch]; per problem
// its state (what the caller gets as status), its accepted steps and those of the current round; word: running count |
// problems whose set changed (h_word: the same). The factorisation of the last round is remembered (fact) with its flags
// and what it left (kept) for the adjoint on the same system; whatever drops box.fact drops it (forget_shifted).
// soln_gen: the solution generation the latest polish left (0: none). The adjoint on the same system
// (ndlqr_hip_solve_polished_adjoint) shares the candidate, residual, correction and norm buffers.
constexpr int kPolishMaxSteps = 32;
struct PolishState {
  DevBuf<unsigned char> code;
  DevBuf<double> z, mu, bt, zc, muc, btc, z0, r, delta, sig;
  DevBuf<double> nu, abt, ones;      // the adjoint's multipliers and right-hand side (its w is adj.z); 1.0 [batch]
  DevBuf<int> astate, asteps, ahere;  // ... its states and steps
  unsigned long long adj_gen = 0;     // the solution generation the polished adjoint belongs to (0: none)
  DevBuf<unsigned long long> norms;
  DevBuf<int> state, steps, here, word;
  PinnedBuf<int> h_word;
  bool fact = false;
  unsigned flags = 0;
  KeptState kept;
  unsigned long long soln_gen = 0;
  static size_t norm_count(const ndlqr::Dims& d) { return 2 * (kPolishMaxSteps + 1) * (size_t)d.batch; }
  hipError_t ensure(const ndlqr::Dims& d, hipStream_t st) {
    const size_t nz = doubles_z(d), nv = doubles_QR(d), nb = (size_t)d.batch;
    return first_error({code.ensure(nv), z.ensure(nz), mu.ensure(nv), bt.ensure(nz), zc.ensure(nz), muc.ensure(nv),
                        btc.ensure(nz), z0.ensure(nz), r.ensure(nz),
                        delta.ensure_zeroed(nz, st),  // (entries a re-solve does not write: the pad rows)
                        sig.ensure(nb), norms.ensure(norm_count(d)), state.ensure(nb), steps.ensure(nb), here.ensure(nb),
                        word.ensure(2), h_word.ensure(2)});
  }
  hipError_t ensure_adjoint(const ndlqr::Dims& d) {
    const size_t nb = (size_t)d.batch;
    return first_error({nu.ensure(doubles_QR(d)), abt.ensure(doubles_z(d)), ones.ensure(nb), astate.ensure(nb), asteps.ensure(nb),
                        ahere.ensure(nb)});
  }
};

// Several right-hand sides per problem (ndlqr_hip_solve_multi_rhs): buffers for `cap` right-hand sides ([cap] of the
// right-hand side, the solution, z_sep, the pushed sums and the top multipliers; the caller-layout inputs and packed
// solutions), grown on demand
struct MultiRhsState {
  DevBuf<double> rhs, z, zsep, fsum, ytop, in, out;
  // (u: the caller's block sizes. Padded shapes: the pad entries of rhs and z are zero and stay zero -- the pack kernel
  //  never touches them)
  hipError_t ensure(const ndlqr::Dims& d, const ndlqr::Dims& u, size_t cap, hipStream_t st) {
    const size_t nz = cap * d.N * d.rows;
    if (rhs.count() >= nz) return hipSuccess;
    hipError_t e = first_error({rhs.grow(nz), z.grow(nz), zsep.grow(cap * d.N * d.n), fsum.grow(cap * (d.N / 8) * 2 * d.n),
                                ytop.grow(cap * (d.N / 8) * d.n), in.grow(cap * ((size_t)u.N * (2 * u.n + u.m) + u.n)),
                                out.grow(cap * ((size_t)u.rows * u.N - u.m))});
    if (e == hipSuccess) e = first_error({hipMemsetAsync(rhs, 0, sizeof(double) * nz, st), hipMemsetAsync(z, 0, sizeof(double) * nz, st)});
    if (e != hipSuccess)
      for (DevBuf<double>* b : {&rhs, &z, &zsep, &fsum, &ytop, &in, &out}) b->reset();
    return e;
  }
};

// Dense cost matrices by reduction to a unit-cost problem (ndlqr_hip_init_dense, kernels_cost.hpp; DESIGN.md section
// 3.16). dense: the resident problem is the reduction of a dense-cost one -- the mode every diagonal initialiser leaves.
// All in the CALLER's block sizes and horizon (u): rec [batch][N][n^2 + m^2 + m n], the records L | L_R | G of every knot,
// resident while the mode lasts; the reduced problem in the flat layout the pack kernels read -- At [batch][N][n^2], Bt
// [batch][N][n m], qt, dt [batch][N][n], rt [batch][N][m], x0t [batch][n] and ones [batch][N][n+m] (Q~ | R~ = 1); stage
// [batch][nvars], the packed vector S' goes through on its way into the adjoint solve.
struct CostState {
  bool dense = false;
  unsigned long long mapped_gen = 0;  // the resident solution of this generation is already in the caller's variables (a constrained solve's): the delivery does not map it back
  DevBuf<double> rec, At, Bt, qt, rt, dt, x0t, ones, stage;
  bool mapped(unsigned long long gen) const { return mapped_gen != 0 && mapped_gen == gen; }
  double phase_ms[3] = {};  // under NDLQR_FLAG_PROFILE: device time of the latest cost_factor + cost_transform | cost_apply_t | cost_apply
  static size_t record_doubles(const ndlqr::Dims& u) { return (size_t)u.n * u.n + (size_t)u.m * u.m + (size_t)u.m * u.n; }
  hipError_t ensure(const ndlqr::Dims& u) {
    const size_t kn = (size_t)u.batch * u.N;
    return first_error({rec.ensure(kn * record_doubles(u)), At.ensure(kn * u.n * u.n), Bt.ensure(kn * u.n * u.m),
                        qt.ensure(kn * u.n), rt.ensure(kn * u.m), dt.ensure(kn * u.n), x0t.ensure((size_t)u.batch * u.n),
                        ones.ensure(kn * u.w), stage.ensure((size_t)u.batch * ((size_t)u.rows * u.N - u.m))});
  }
};

// General linear inequality constraints lo <= C x + D u <= hi by ADMM on the dense-cost reduction
// (ndlqr_hip_init_constrained / ndlqr_hip_solve_constrained, kernels_lin.hpp). active: the
// resident problem came from the constrained initialiser -- a dense-cost mode with constraints; every other initialiser
// leaves it. All in the CALLER's block sizes and horizon (u), p rows per knot. Retained inputs in the flat layout: A, B,
// Q, H (has_H), R and the caller's right-hand side q, r, d, x0 (rhs_new: replaced since the shifted S' last ran); C
// [batch][N][p n], D [batch][N][p m]; lo, hi, mask [P][N][p] (bstride 0: shared). The shifted problem: costs Qs, Hs, Rs,
// records rec, and the reduced flat arrays At .. x0t (CostState keeps the plain ones). Iteration state: v, y [batch][N][p],
// the re-solve's z~ and two right-hand sides in the device layout, per problem status, iters, resid [4]; word: the
// running count | lo > hi | pattern changed (within a solve word[1] counts the problems whose penalty moved at an adapt
// iteration, moved [batch] marks them: section 3.19). The shifted reduction and factorisation are remembered (fact) with
// the penalties rho [batch] -- rho_value when rho_uniform says they are all that one value --, the flags and what the
// factorisation left (kept). soln_gen: the solution generation the latest constrained solve left. adapt_every, rho_min,
// rho_max: the setting of ndlqr_hip_set_constraint_adaptation, the solver's and not the problem's: no initialiser resets it.
struct LinState {
  bool active = false, has_H = false, shared = false, have_vy = false, rhs_new = true, fact = false;
  bool rho_uniform = false;
  int p = 0;
  int adapt_every = 0;
  size_t bstride = 0;
  double rho_value = 0.0, rho_min = 1e-6, rho_max = 1e6;
  unsigned flags = 0;
  KeptState kept;
  unsigned long long soln_gen = 0;
  size_t lds_asked[5] = {};  // dynamic LDS already asked for lin_shift_cost | lin_start | lin_update<true> | <false> | lin_finish
  DevBuf<double> A, B, Q, H, R, q, r, d, x0, C, D, lo, hi, Qs, Hs, Rs, rec, At, Bt, qt, rt, dt, x0t, v, y, z, rhs[2], resid, rho;
  DevBuf<unsigned char> mask;
  DevBuf<int> status, iters, word, moved;
  PinnedBuf<int> h_word;
  // the buffers that depend on p are allocated again when p changes
  hipError_t ensure(const ndlqr::Dims& u, const ndlqr::Dims& dd, int rows_per_knot, hipStream_t st) {
    const size_t kn = (size_t)u.batch * u.N, n = (size_t)u.n, m = (size_t)u.m, nb = (size_t)u.batch;
    if (rows_per_knot != p)
      for (DevBuf<double>* b : {&C, &D, &lo, &hi, &v, &y}) b->reset();
    if (rows_per_knot != p) mask.reset();
    p = rows_per_knot;
    const size_t np = kn * (size_t)p;
    return first_error({A.ensure(kn * n * n), B.ensure(kn * n * m), Q.ensure(kn * n * n), H.ensure(kn * n * m), R.ensure(kn * m * m),
                        q.ensure(kn * n), r.ensure(kn * m), d.ensure(kn * n), x0.ensure(nb * n), C.ensure(np * n), D.ensure(np * m),
                        lo.ensure(np), hi.ensure(np), mask.ensure_zeroed(np, st), Qs.ensure(kn * n * n), Hs.ensure(kn * n * m),
                        Rs.ensure(kn * m * m), rec.ensure(kn * (n * n + m * m + m * n)), At.ensure(kn * n * n),
                        Bt.ensure(kn * n * m), qt.ensure(kn * n), rt.ensure(kn * m), dt.ensure(kn * n), x0t.ensure(nb * n),
                        v.ensure(np), y.ensure(np),
                        z.ensure_zeroed(doubles_z(dd), st),  // (entries a re-solve does not write: the pad rows)
                        rhs[0].ensure(doubles_z(dd)), rhs[1].ensure(doubles_z(dd)), resid.ensure(4 * nb),
                        rho.ensure(nb), status.ensure(nb), iters.ensure(nb), word.ensure(3), h_word.ensure(3),
                        moved.ensure_zeroed(nb, st)});
  }
};

// Gradients through the solve with linear inequality constraints (ndlqr_hip_solve_constrained_adjoint /
// ndlqr_hip_constraint_gradients, kernels_lin_grad.hpp). gen: the solution generation the
// constrained adjoint belongs to (0: none). The adjoint's own row codes, v, y [batch][N][p], ADMM right-hand sides (its
// resident one is adj.rhs, its re-solves go to lin.z, its solution to adj.z), per problem status, iterations and
// residuals, and its running count (word, h_word): nothing of the forward's iteration state is touched. lds_asked: as
// LinState's, for lin_adjoint_start | lin_adjoint_update<true> | <false> | lin_adjoint_finish.
struct LinAdjointState {
  DevBuf<unsigned char> code;
  DevBuf<double> v, y, resid, rhs[2];
  DevBuf<int> status, iters, word;
  PinnedBuf<int> h_word;
  int p = 0;
  size_t lds_asked[4] = {};
  unsigned long long gen = 0;
  // the buffers that depend on p are allocated again when p changes
  hipError_t ensure(const ndlqr::Dims& u, const ndlqr::Dims& dd, int rows_per_knot) {
    if (rows_per_knot != p) {
      code.reset(); v.reset(); y.reset();
    }
    p = rows_per_knot;
    const size_t np = (size_t)u.batch * u.N * p, nz = doubles_z(dd), nb = (size_t)u.batch;
    return first_error({code.ensure(np), v.ensure(np), y.ensure(np), rhs[0].ensure(nz), rhs[1].ensure(nz), resid.ensure(4 * nb),
                        status.ensure(nb), iters.ensure(nb), word.ensure(1), h_word.ensure(1)});
  }
};

// Infeasibility detection of the solve with linear inequality constraints (ndlqr_hip_set_constraint_infeasibility,
// kernels_lin_infeas.hpp). every, eps: the setting, the solver's and not the problem's (every == 0:
// off -- nothing here is allocated or launched). All in the CALLER's block sizes and horizon (u): lam_prev, lam_cur
// [batch][N][n], the multipliers of the re-solve before a check and of the check's in the caller's variables; mu_prev
// [batch][N][p] = rho y after the update before a check; the certificate of every status-4 problem, zero elsewhere
// (cert_lam [batch][N][n], cert_mu [batch][N][p]); the four numbers of every problem's latest check and the iteration it
// ran at (measures [batch][4], measured_at [batch]; zero for a problem no check examined). All of it is zeroed at the
// start of every solve with detection on. gen: the solution generation of the latest constrained solve that ran with
// detection on (0: none). lds_asked: as LinState's, for lin_lambda_out | lin_certify.
struct LinInfeasState {
  DevBuf<double> lam_prev, lam_cur, mu_prev, cert_lam, cert_mu, measures;
  DevBuf<int> measured_at;
  int every = 0, p = 0;
  double eps = 1e-4;
  size_t lds_asked[2] = {};
  unsigned long long gen = 0;
  // the buffers that depend on p are allocated again when p changes
  hipError_t ensure(const ndlqr::Dims& u, int rows_per_knot) {
    if (rows_per_knot != p) {
      mu_prev.reset(); cert_mu.reset();
    }
    p = rows_per_knot;
    const size_t nl = (size_t)u.batch * u.N * u.n, np = (size_t)u.batch * u.N * p, nb = (size_t)u.batch;
    return first_error({lam_prev.ensure(nl), lam_cur.ensure(nl), mu_prev.ensure(np), cert_lam.ensure(nl), cert_mu.ensure(np),
                        measures.ensure(4 * nb), measured_at.ensure(nb)});
  }
};

// Active-set polish of the solve with linear inequality constraints (ndlqr_hip_polish_constrained,
// kernels_lin_polish.hpp). Per row, in the CALLER's horizon [batch][N][p]: the codes (bytes), the
// accepted multipliers mu, the candidate muc and rc, the constraint residual of the iterate evaluated last. In the device
// layout [batch][d.N][2 d.n + d.m]: the accepted iterate z and the candidate zc in the caller's variables, z0 (the resident
// solution as found: the factorisations overwrite it), r (the right-hand side of the correction in the caller's
// variables), rt (S^' r) and delta (the re-solve's reduced correction). norms: the slots of one round,
// [2][kPolishMaxSteps + 1][batch] bit patterns -- max(|r_z|, |r_c|), then |r_c| --; sig [batch]; per problem its state (what
// the caller gets as status), its accepted steps and those of the current round; word: running count | problems whose set
// changed (h_word: the same, pinned). The shifted costs, records and reduced problem are LinState's: a polish drops the
// ADMM factorisation. soln_gen: the solution generation the latest polish left (0: none); rounds: its factorisations.
// lds_asked: as LinState's, for lin_polish_shift_cost | lin_polish_residual | lin_polish_apply_t | lin_polish_update<true> |
// <false>.
struct LinPolishState {
  DevBuf<unsigned char> code;
  DevBuf<double> mu, muc, rc, z, zc, z0, r, rt, delta, sig;
  DevBuf<unsigned long long> norms;
  DevBuf<int> state, steps, here, word;
  PinnedBuf<int> h_word;
  int p = 0, rounds = 0;
  size_t lds_asked[5] = {};
  unsigned long long soln_gen = 0;
  double phase_ms[3] = {};  // under NDLQR_FLAG_PROFILE: device time of the latest polish's residuals | S^' + re-solves | updates
  int phase_spans[3] = {};  // ... and how many spans each adds up
  static size_t norm_count(const ndlqr::Dims& d) { return 2 * (kPolishMaxSteps + 1) * (size_t)d.batch; }
  // the buffers that depend on p are allocated again when p changes
  hipError_t ensure(const ndlqr::Dims& u, const ndlqr::Dims& dd, int rows_per_knot, hipStream_t st) {
    if (rows_per_knot != p) {
      code.reset(); mu.reset(); muc.reset(); rc.reset();
    }
    p = rows_per_knot;
    const size_t np = (size_t)u.batch * u.N * p, nz = doubles_z(dd), nb = (size_t)u.batch;
    return first_error({code.ensure(np), mu.ensure(np), muc.ensure(np), rc.ensure(np), z.ensure(nz), zc.ensure(nz), z0.ensure(nz),
                        r.ensure_zeroed(nz, st), rt.ensure_zeroed(nz, st),
                        delta.ensure_zeroed(nz, st),  // (entries a re-solve does not write: the pad rows)
                        sig.ensure(nb), norms.ensure(norm_count(dd)), state.ensure(nb), steps.ensure(nb), here.ensure(nb),
                        word.ensure(2), h_word.ensure(2)});
  }
};

struct NdlqrHipCtx {
  ndlqr::Dims d = {};   // block sizes of the DEVICE layout (every kernel works on these)
  ndlqr::Dims du = {};  // the caller's block sizes and horizon: the same, or smaller when the problem runs zero-padded into
                        // the next size-specialised instance ("padded shapes", ndlqr_hip_create) or with its horizon padded
                        // to the next power of two (du.N < d.N, "padded horizon"); only the boundary functions see it
  bool padded = false;  // d differs from du in a block size or in the horizon
  int device = 0;
  unsigned flags = 0;
  DevKnobs knobs;
  bool own_stream = true;  // the primary set's stream is the context's own (ndlqr_hip_set_stream)
  DevBuf<double> AB, QR;
  DevBuf<double> F;  // complete factor array; allocated by the first solve whose schedule touches it (ndlqr_hip_ensure_F)
  DevBuf<int> info;
  DevBuf<double> pad_stage;    // HBM staging of caller-layout inputs / outputs of a padded shape (grow_pad_stage)
  DevBuf<double> grad_stage;   // HBM staging of the host outputs / inputs of the gradient and bounds functions and their partial batch sums (grown on demand)
  DevBuf<double> kkt_out;      // [2 batch] scratch of ndlqr_hip_kkt_residual (allocated on first use)
  DevBuf<double> sep_scratch;  // S-bar and panel of every level-0 separator in global memory: blocks beyond the LDS of separator_generic (allocated on first use)
  PinnedBuf<double> h_stage[2];  // bounce buffers of the downloads into pageable host memory (allocated on first use)
  BufferSet set[2];     // the two-deep solve pipeline: [0] the primary set, [1] the alternate (allocated on first use)
  int cur = 0;          // the set the next launches go to
  int latest = 0;       // the set holding the most recent solution
  int pipeline = 2;     // 1: stream-ordered solves; 2 (default, DevKnobs::pipeline): consecutive solves alternate sets
  unsigned solve_count = 0;  // solves enqueued so far (parity picks the set)
  bool state_dirty = false;  // a solve failed to launch or to complete: counters / failure words are zeroed before the next one
  int fail_base = 0;         // value of the (cumulative) batch-wide failure counter at the last synchronisation
  KeptState kept;  // of the latest solve
  hipEvent_t ev_step[2] = {};  // end of the steps of ndlqr_hip_step_async, alternating (ndlqr_hip_synchronize_previous)
  unsigned step_count = 0;
  hipEvent_t ev_inputs = nullptr;  // orders the other buffer set's stream behind a device-side replacement of the inputs
  // One LOGICAL right-hand side, two physical copies (one per buffer set): generation counters per part -- 0: q,
  // 1: r, 2: d, 3: x0 -- of the latest write here, and of each set's copy in BufferSet::rhs_gen. Whoever writes
  // (uploads, device packing, an MPC step) writes the CURRENT set and bumps its generations; a solve or step that
  // lands on a set whose copy is behind in a part it does not replace copies that part over first (rhs_make_current).
  unsigned long long rhs_latest[4] = {};
  KnotSlice sel;  // what an MPC step brings down (ndlqr_hip_set_step_selection)
  // With NDLQR_SOLN_ONLY (8) in sel.blocks a step computes nothing but the selected knots: the last launch of the
  // back-substitution covers workgroups [apply_blk0, apply_blk0 + apply_nblk) of eight knots only
  // (apply_nblk == 0: all; set by ApplySlice around the launches of a step or a slice, honoured by the schedules that end in
  // rb_backsub, part of the key of the captured launch sequence), and z_partial says that the latest solution is such a
  // slice -- [z_blk0, z_blk0 + z_nblk) -- so that nothing else is handed out until the next complete solve
  int apply_blk0 = 0, apply_nblk = 0;
  bool z_partial = false;
  bool z_invalid = false;  // the resident solution is not one (a constrained solve failed after its factorisation)
  int z_blk0 = 0, z_nblk = 0;
  int step_set[2] = {};  // buffer set of the steps behind ev_step[0 / 1]
  // One-shot solve of a small batch from / into pinned host staging (ndlqr_hip_solve_staged; the drop-in ndlqr_Solve):
  // AB | QR | rhs going up, the solution blocks [batch][N][2n+m] coming down, all in the caller's block size; the whole
  // sequence -- three copies up, the launch chain, the copy down -- is ONE captured graph.
  PinnedBuf<double> h_io;  // AB | QR | rhs | z
  CapturedChain staged;
  bool timing_pending = false;
  double last_ms = 0;
  int last_failures = 0;
  unsigned long long soln_gen = 0;  // counts the resident solutions (note_solution)
  bool inputs_replaced = false;     // new A, B, Q, R since the last solve
  // the optional features, each with its buffers (allocated on first use by its ensure())
  AdjointState adj;
  BoxState box;
  BoxInfeasState infeas;
  BoxAccelState accel;
  BoxAdjointState abox;
  RefineState ref;
  PolishState pol;
  MultiRhsState multi;
  CostState cost;
  LinState lin;
  LinAdjointState alin;
  LinInfeasState lin_infeas;
  LinPolishState lin_pol;
  unsigned long long factor_count = 0;  // factorisations launched (ndlqr_hip_factor_count)
  // the remembered shifted factorisations (ADMM's and the polish's) no longer match the records / factors
  void forget_shifted() { box.fact = pol.fact = lin.fact = false; }
  // adj.z holds w of the constrained adjoint of the resident solution, in the caller's variables already
  bool lin_adjoint_resident() const {
    return alin.gen != 0 && alin.gen == soln_gen && adj.gen == soln_gen && lin.soln_gen == soln_gen && !lin.rhs_new;
  }
  // the resident solution is that of the latest polish of a solve with linear inequality constraints
  bool lin_polished() const { return lin_pol.soln_gen != 0 && lin_pol.soln_gen == soln_gen; }
  // grows with every write of a part of the right-hand side (rhs_latest)
  unsigned long long rhs_stamp() const { return rhs_latest[0] + rhs_latest[1] + rhs_latest[2] + rhs_latest[3]; }
  // profile
  std::vector<PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
  double slot_ms[SLOT_COUNT] = {};
  int slot_launches[SLOT_COUNT] = {};
  // Room for `doubles` in pad_stage. Growing waits for the current set's stream, which may still read the old array, and
  // drops the staged graph, which holds its address.
  hipError_t grow_pad_stage(size_t doubles) {
    if (doubles <= pad_stage.count()) return hipSuccess;
    const hipError_t e = pad_stage ? hipStreamSynchronize(set[cur].stream) : hipSuccess;
    if (e != hipSuccess) return e;
    staged.reset();
    return pad_stage.grow(doubles);
  }
};

#pragma GCC visibility pop

static inline hipEvent_t take_event(NdlqrHipCtx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t ev = c->event_pool.back();
    c->event_pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  (void)hipEventCreate(&ev);
  return ev;
}

struct ScopedSlot {  // brackets one kernel launch with events when profiling is on
  NdlqrHipCtx* c;
  PendingEvent pe;
  bool on;
  ScopedSlot(NdlqrHipCtx* ctx, int slot) : c(ctx), on((ctx->flags & NDLQR_FLAG_PROFILE) != 0) {
    if (!on) return;
    pe.slot = slot; pe.start = take_event(c); pe.stop = take_event(c);
    (void)hipEventRecord(pe.start, c->set[c->cur].stream);
  }
  ~ScopedSlot() {
    if (!on) return;
    (void)hipEventRecord(pe.stop, c->set[c->cur].stream);
    c->pending.push_back(pe);
  }
};
