// ndlqr_hip.hip -- gfx950 (MI355X, CDNA4) implementation of the device boundary in
// include/ndlqr_hip.h: context/memory management, launch sequence, D2H converters and the
// dense Matrix* helpers. Kernels live in kernels_generic.hpp (any n, m) and kernels_small.hpp
// (size-specialised, one knot row per lane).
//
// Written for wave64 / gfx950 only; built with -ffp-contract=off so that every fused
// multiply-add in the kernels is an explicit fma() (fast mode) or an explicit mul + add
// (NDLQR_FLAG_STRICT_FP, which reproduces the reference's default CPU build bit for bit).
#include <mutex>

#include "hip_context.hpp"
#include "kernels_generic.hpp"
#include "kernels_box.hpp"
#include "kernels_box_grad.hpp"
#include "kernels_box_accel.hpp"
#include "kernels_box_infeas.hpp"
#include "kernels_box_polish.hpp"
#include "kernels_cost.hpp"
#include "kernels_grad.hpp"
#include "kernels_refine.hpp"
#include "kernels_mfma.hpp"
#include "kernels_reduced_mfma.hpp"
#include "launch_small.hpp"  // (SmallInstance; its templates are instantiated in small_instance.hip)

// ------------------------------------------------------------------------------ errors

static thread_local std::string g_last_error = "";

const char* ndlqr_hip_last_error(void) { return g_last_error.c_str(); }

int ndlqr_hip_fail(const char* what, hipError_t e) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  fprintf(stderr, "ndlqr_hip: %s\n", g_last_error.c_str());
  // a launch configuration / argument the device rejects is the caller's (or this library's) error,
  // not a missing device
  if (e == hipErrorInvalidConfiguration || e == hipErrorInvalidValue) return NDLQR_ERR_INVALID;
  return NDLQR_ERR_NO_DEVICE;
}
static int fail(const char* what, hipError_t e) { return ndlqr_hip_fail(what, e); }
// records the message for ndlqr_hip_last_error(), prints it, returns NDLQR_ERR_INVALID
static int refuse(const std::string& msg) {
  g_last_error = msg;
  fprintf(stderr, "ndlqr_hip: %s\n", g_last_error.c_str());
  return NDLQR_ERR_INVALID;
}

// Padded horizon (ndlqr_hip_create_ex): an entry point that is not carried through refuses here -- it would index the
// caller's arrays, which have du.N knots, with the device's d.N
static int need_unpadded_horizon(const NdlqrHipCtx* c, const char* who) {
  if (c->du.N == c->d.N) return NDLQR_OK;
  return refuse(std::string(who) + ": not available for a padded horizon (horizon " + std::to_string(c->du.N) +
                " runs as " + std::to_string(c->d.N) + " knots); use a power-of-two horizon");
}

// Dense-cost mode (ndlqr_hip_init_dense): the resident problem is the unit-cost reduction of the
// caller's. An entry point that is not carried through refuses here -- the rows, records and arrays it would work on are
// those of the reduced system
static int need_diagonal_cost(const NdlqrHipCtx* c, const char* who) {
  if (!c->cost.dense) return NDLQR_OK;
  return refuse(std::string(who) + ": not available in dense-cost mode (the resident problem is the unit-cost reduction "
                "ndlqr_InitializeBatchFlatDense left); use a diagonal initialiser");
}

// one launch of a kernel of kernels_cost.hpp: a wavefront per (knot, problem) of `count` problems
template <class... Params, class... Args>
static hipError_t launch_cost(void (*kernel)(Params...), size_t lds_doubles, const ndlqr::Dims& u, unsigned count, hipStream_t st,
                              Args... args) {
  const size_t lds = sizeof(double) * lds_doubles;
  const hipError_t e = allow_dynamic_lds(kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(u.N, count), dim3(64), lds, st, static_cast<Params>(args)...);
  return hipGetLastError();
}
// Under NDLQR_FLAG_PROFILE: HIP events around the launches of one phase of the reduction (CostState::phase_ms[which]);
// stop() waits for them, so a profiled call is synchronous. Without the flag nothing is recorded.
struct CostPhase {
  NdlqrHipCtx* c;
  hipStream_t st;
  int which;
  hipEvent_t a = nullptr, b = nullptr;
  CostPhase(NdlqrHipCtx* ctx, hipStream_t stream, int phase) : c(ctx), st(stream), which(phase) {
    if (!(c->flags & NDLQR_FLAG_PROFILE)) return;
    a = take_event(c); b = take_event(c);
    (void)hipEventRecord(a, st);
  }
  void stop() {
    if (!a) return;
    float ms = 0.0f;
    if (hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
      c->cost.phase_ms[which] = ms;
    c->event_pool.push_back(a);
    c->event_pool.push_back(b);
    a = b = nullptr;
  }
};
// dense-cost mode: `vec`, the packed [count][nvars] vectors of problems [p0, p0 + count) in the reduced variables, becomes
// the same in the caller's (S, in place)
static hipError_t cost_map_back(NdlqrHipCtx* c, double* vec, int p0, unsigned count, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  CostPhase phase(c, st, 2);
  const hipError_t e = launch_cost(ndlqr::cost_apply, ndlqr::cost_apply_lds(u.n, u.m), u, count, st, u.n, u.m, u.N,
                                   c->cost.rec + (size_t)p0 * u.N * CostState::record_doubles(u), vec);
  phase.stop();
  return e;
}

// Where a caller's array lives. A pointer the runtime does not know (an ordinary malloc'ed one is "invalid value" to older
// runtimes) is pageable host memory.
enum class Where { Pageable, Pinned, OwnDevice, OtherDevice };
static Where where(const void* p, int device) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return Where::Pageable; }
  if (a.type == hipMemoryTypeDevice) return a.device == device ? Where::OwnDevice : Where::OtherDevice;
  return a.type == hipMemoryTypeHost ? Where::Pinned : Where::Pageable;
}

int ndlqr_hip_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

static const char* kSlotNames[SLOT_COUNT] = {"leaf", "separator", "schur", "schur_boundary", "apply", "bottom", "upper", "top"};

static bool has_small_instance(int nstates, int ninputs);  // defined with the instance table below
static void pick_pad_instance(int nstates, int ninputs, int* pn, int* pm);

static size_t bytes_QR(const ndlqr::Dims& d) { return sizeof(double) * doubles_QR(d); }
static size_t bytes_z(const ndlqr::Dims& d) { return sizeof(double) * doubles_z(d); }
static size_t bytes_F(const ndlqr::Dims& d) { return sizeof(double) * doubles_F(d); }

// Every getenv of the context: the developer switches, read once per context
static DevKnobs read_knobs() {
  DevKnobs k;
  const auto num = [](const char* name, int* v) { if (getenv(name)) *v = atoi(getenv(name)); };
  const auto onoff = [](const char* name, int* v) { if (getenv(name)) *v = atoi(getenv(name)) != 0 ? 1 : 0; };
  num("NDLQR_PIPELINE", &k.pipeline);
  onoff("NDLQR_TREE", &k.tree);                  // unset: by batch size
  onoff("NDLQR_ROWBCAST", &k.rowbcast);          // unset: by block size
  onoff("NDLQR_FUSE2", &k.fuse2);                // unset: by instance (launch_small)
  onoff("NDLQR_BACKSUB_COLS", &k.backsub_cols);
  k.no_mfma = getenv("NDLQR_NO_MFMA") != nullptr;
  k.no_top = getenv("NDLQR_NO_TOP") != nullptr;
  num("NDLQR_TOP_LEVELS", &k.top_levels);
  if (k.top_levels < 3 || k.top_levels > 5) k.top_levels = 3;
  num("NDLQR_SEP_THREADS", &k.sep_threads);
  num("NDLQR_MULT_THREADS", &k.mult_threads);
  k.no_reduced_generic = getenv("NDLQR_DEV_NO_REDUCED_GENERIC") != nullptr;
  k.no_pad = getenv("NDLQR_NO_PAD") != nullptr;
  k.alt_priority_set = getenv("NDLQR_ALT_PRIORITY") != nullptr;
  num("NDLQR_ALT_PRIORITY", &k.alt_priority);
  return k;
}

// What both buffer sets allocate alike, on the set's stream (created by the caller): events, records, solution, its copy of
// the right-hand side, failure word; with `slots` (size-specialised shapes) the accumulator slots, the multipliers of the
// top separators and the arrival counters (the runtime-sized schedule's slots: ensure_red_generic)
static bool alloc_set(NdlqrHipCtx* c, BufferSet& s, bool slots) {
  const ndlqr::Dims& d = c->d;
  hipError_t e = first_error({hipEventCreate(&s.ev_start), hipEventCreate(&s.ev_stop), s.rec.ensure((size_t)d.batch * d.N * (2 * d.n * d.n + d.n)),
                              s.rhs.ensure(doubles_z(d)), s.h_fail.ensure_zeroed(1)});
  if (e == hipSuccess && slots) {
    // slot = DL | DR (packed lower triangles) | CA | CB | gL | gR, padded to whole 128-byte lines (RedSlot<NX>::SIZE)
    const size_t slot_doubles = ((size_t)d.n * (d.n + 1) + 2 * (size_t)d.n * d.n + 2 * d.n + 15) / 16 * 16;
    e = first_error({s.red.ensure_zeroed((size_t)d.batch * (d.N / 4) * slot_doubles, s.stream),
                     s.ytop.ensure((size_t)d.batch * (d.N / 8) * d.n),
                     s.tree_cnt.ensure_zeroed((size_t)d.batch * (d.N / 4), s.stream)});
  }
  return e == hipSuccess && s.z.ensure_zeroed(doubles_z(d), s.stream) == hipSuccess;
}

NdlqrHipCtx* ndlqr_hip_create(int nstates, int ninputs, int nhorizon, int batch, int device) {
  return ndlqr_hip_create_ex(nstates, ninputs, nhorizon, batch, device, 0u);
}

NdlqrHipCtx* ndlqr_hip_create_ex(int nstates, int ninputs, int nhorizon, int batch, int device, unsigned create_flags) {
  if (nstates <= 0 || ninputs <= 0 || batch <= 0 || nhorizon < 2 || nhorizon > (1 << 24)) {
    g_last_error = "invalid dimensions";
    return nullptr;
  }
  if (batch > 65535) {  // the batch index rides on gridDim.y
    g_last_error = "batch > 65535 problems per solver: split the batch over several solvers";
    fprintf(stderr, "ndlqr_hip: %s\n", g_last_error.c_str());
    return nullptr;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_last_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    return nullptr;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= count) {
    g_last_error = "device index out of range";
    return nullptr;
  }
  if ((e = hipSetDevice(device)) != hipSuccess) { fail("hipSetDevice", e); return nullptr; }

  NdlqrHipCtx* c = new NdlqrHipCtx();
  c->knobs = read_knobs();
  c->pipeline = c->knobs.pipeline;
  ndlqr::Dims& d = c->d;
  // Padded horizon: the device works on the next power of two (the tree, the schedules and the size-specialised kernels
  // see nothing else); the knots beyond the caller's are decoupled unit knots ([A | B] = 0, Q = R = 1, zero right-hand
  // side: pad_fill_generic) and the caller's last knot becomes an interior device knot with [A | B] = 0, R = 1 and a zero
  // r slot (the pack kernels). The tail solves to exactly zero and the caller's solution is a prefix of the device's.
  int phorizon = 1;
  while (phorizon < nhorizon) phorizon <<= 1;
  auto set_dims = [&](ndlqr::Dims& x, int n_, int m_, int N_) {
    x.n = n_; x.m = m_; x.N = N_; x.batch = batch;
    x.K = 0; while ((1 << x.K) < phorizon) ++x.K;
    x.rows = 2 * n_ + m_; x.w = n_ + m_; x.fb = x.rows * n_; x.xoff = 0;
  };
  set_dims(c->du, nstates, ninputs, nhorizon);
  nhorizon = phorizon;  // (everything below is sized and chosen by the device's horizon)
  // Padded shapes: a block size without a size-specialised instance runs zero-padded inside the cheapest instance
  // that contains it (dummy states and inputs with unit weights and no coupling: they solve to exactly zero and the
  // real variables see the same arithmetic plus exact zeros) instead of the runtime-sized kernels, which are 3-4x
  // slower below 16 states. NDLQR_NO_PAD=1 keeps the caller's block size (A/B, tests).
  int pn = nstates, pm = ninputs;
  const bool may_pad = !c->knobs.no_pad && !(create_flags & NDLQR_CREATE_NO_PAD);
  if (!has_small_instance(nstates, ninputs) && nhorizon >= 8 && may_pad)
    pick_pad_instance(nstates, ninputs, &pn, &pm);
  // ... and beyond 128 states (the knot-based kernels: launch_generic) a block that does not fill 16 x 16 tiles is padded
  // to the next one that does: separator_mfma instead of separator_generic, 3-7x faster there (round 4)
  if (nstates > 128 && (nstates % 16 != 0 || (nstates + ninputs) % 4 != 0) && may_pad) {
    pn = (nstates + 15) / 16 * 16;
    pm = ninputs + (4 - (pn + ninputs) % 4) % 4;
  }
  set_dims(d, pn, pm, phorizon);
  c->padded = pn != nstates || pm != ninputs || c->du.N != d.N;
  c->device = device;
  BufferSet& s = c->set[0];
  bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_step[0], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_step[1], hipEventDisableTiming) == hipSuccess &&
            c->AB.ensure((size_t)d.batch * d.N * d.n * d.w) == hipSuccess && c->QR.ensure(doubles_QR(d)) == hipSuccess &&
            alloc_set(c, s, nhorizon >= 8 && has_small_instance(d.n, d.m));
  if (ok && c->padded) {
    hipLaunchKernelGGL(ndlqr::pad_fill_generic, dim3(d.N, d.batch), dim3(128), 0, s.stream, d, c->AB, c->QR, s.rhs);
    ok = hipGetLastError() == hipSuccess;
  }
  // (the factor array F is allocated by the first solve whose schedule touches it: ndlqr_hip_ensure_F)
  ok = ok && c->info.ensure_zeroed((size_t)batch + 1, s.stream) == hipSuccess && hipStreamSynchronize(s.stream) == hipSuccess;
  if (!ok) {
    fail("device allocation", hipGetLastError());
    ndlqr_hip_destroy(c);
    return nullptr;
  }
  s.ready = true;
  return c;
}

// release buffer set i (the primary set's stream only where the context owns it): what is not memory by hand, the
// buffers with the set
static void free_set(NdlqrHipCtx* c, int i) {
  BufferSet& s = c->set[i];
  if (s.stream) (void)hipStreamSynchronize(s.stream);
  s.graph.reset();
  if (s.ev_start) (void)hipEventDestroy(s.ev_start);
  if (s.ev_stop) (void)hipEventDestroy(s.ev_stop);
  if (s.stream && (i == 1 || c->own_stream)) (void)hipStreamDestroy(s.stream);
  s = BufferSet();
}

void ndlqr_hip_destroy(NdlqrHipCtx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (int i = 1; i >= 0; --i) free_set(c, i);
  c->staged.reset();
  for (auto& p : c->pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
  for (auto& ev : c->event_pool) (void)hipEventDestroy(ev);
  if (c->ev_inputs) (void)hipEventDestroy(c->ev_inputs);
  for (hipEvent_t ev : c->ev_step) if (ev) (void)hipEventDestroy(ev);
  delete c;  // (every buffer goes with its owner)
}

// ------------------------------------------------------------------------------ two-deep solve pipeline

// the current buffer set holds the most recent solution -- all of it, or (a step with NDLQR_SOLN_ONLY) the knots of the
// workgroups its back-substitution ran
static void note_solution(NdlqrHipCtx* c) {
  ++c->soln_gen;  // (an adjoint of an earlier solution no longer applies)
  c->latest = c->cur;
  c->z_partial = c->apply_nblk > 0;
  c->z_invalid = false;
  c->z_blk0 = c->apply_blk0;
  c->z_nblk = c->apply_nblk;
}
// Everything is idle (the caller has just waited for both streams) and the current buffer set has received a new right-hand
// side: let the next pipelined solve start on THIS set instead of the other one, whose copy of the right-hand side would
// have to be brought up to date first (copy_rhs_parts_generic: 62 us per 1024 x (12,4,256) in a loop that replaces the
// problem every iteration).
static void next_solve_on_current_set(NdlqrHipCtx* c) {
  if ((c->solve_count & 1u) != (unsigned)c->cur) ++c->solve_count;
}
// consumers of the whole solution vector refuse a slice
static int need_full_solution(const NdlqrHipCtx* c, const char* who) {
  if (c->z_invalid)
    return refuse(std::string(who) + ": the last constrained solve failed; there is no resident solution until the next solve");
  if (!c->z_partial) return NDLQR_OK;
  g_last_error = std::string(who) + ": the last step computed only knots " + std::to_string(8 * c->z_blk0) + " .. " +
                 std::to_string(8 * (c->z_blk0 + c->z_nblk) - 1) + " (NDLQR_SOLN_ONLY); run a solve or a step without it first";
  return NDLQR_ERR_INVALID;
}

// allocate the alternate set on first use; false (and depth 1 from then on) when it does not fit
static bool ensure_alt(NdlqrHipCtx* c) {
  BufferSet& a = c->set[1];
  if (a.ready) return true;
  const BufferSet& p = c->set[0];  // (current: the alternate set is not in use before it exists)
  // The second set's stream gets another priority than the first's: streams of one priority share a few hardware
  // queues round-robin with every other stream of the process, and two streams on ONE hardware queue run strictly one
  // after the other (measured: the step pipeline lost all its overlap in a process that had created other streams
  // before, tools/e2e_probe.py --other-solvers; with its own priority level it keeps it).
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const int alt_prio = c->knobs.alt_priority_set ? c->knobs.alt_priority : prio_greatest;
  bool ok = hipStreamCreateWithPriority(&a.stream, hipStreamNonBlocking, alt_prio) == hipSuccess &&
            alloc_set(c, a, p.tree_cnt != nullptr);
  // this set's own copy of the right-hand side (a step of ndlqr_hip_step_async replaces the right-hand side of
  // ITS buffer set only; rhs_gen / rhs_make_current keep track of which copy is behind in what)
  ok = ok && hipStreamSynchronize(p.stream) == hipSuccess &&
       hipMemcpyAsync(a.rhs, p.rhs, bytes_z(c->d), hipMemcpyDeviceToDevice, a.stream) == hipSuccess &&
       hipStreamSynchronize(a.stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    free_set(c, 1);
    c->pipeline = 1;
    return false;
  }
  *a.h_fail = *p.h_fail;
  for (int q = 0; q < 4; ++q) a.rhs_gen[q] = p.rhs_gen[q];  // (the new set's copy of the right-hand side was taken from p)
  a.ready = true;
  return true;
}

// every solve in flight on either set has finished
static hipError_t sync_all(NdlqrHipCtx* c) {
  hipError_t e = hipSuccess;
  for (const BufferSet& s : c->set)
    if (s.stream) { const hipError_t e2 = hipStreamSynchronize(s.stream); if (e == hipSuccess) e = e2; }
  return e;
}

static int rhs_make_current(NdlqrHipCtx* c, unsigned need);  // below

int ndlqr_hip_set_pipeline_depth(NdlqrHipCtx* c, int depth) {
  if (!c || depth < 1) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  if (c->cur != 0) {  // keep the latest solution where the single-set code expects it
    c->cur = 0;
    {  // (the right-hand side the latest solution belongs to: after ndlqr_hip_step_async the two sets may differ)
      const int merr = rhs_make_current(c, 0xFu);
      if (merr) return merr;
      HIP_TRY(hipStreamSynchronize(c->set[0].stream));
    }
    if (c->latest == 1) {
      HIP_TRY(hipMemcpy(c->set[0].z, c->set[1].z, bytes_z(c->d), hipMemcpyDeviceToDevice));
      HIP_TRY(hipDeviceSynchronize());  // (a device-to-device copy on the null stream need not be finished on return;
                                        //  the solver's streams do not wait for the null stream)
      c->latest = 0;
    }
  }
  c->pipeline = depth > 2 ? 2 : depth;
  return NDLQR_OK;
}
int ndlqr_hip_pipeline_depth(const NdlqrHipCtx* c) { return c ? c->pipeline : 0; }

// The complete factor array [batch][K][N][2n+m][n] (5.6 GB at (12,4,256) x 1024, 87 GB at
// (64,16,512) x 256) exists only for the schedules that touch it: strict mode, KEEP_FACT, the
// knot-based and runtime-sized paths, and the factors kept by KEEP_RECORDS. The default
// separator-only fast path never allocates it. Must run outside stream capture (hipMalloc).
int ndlqr_hip_ensure_F(NdlqrHipCtx* c) {
  if (c->F) return NDLQR_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (c->F.ensure(doubles_F(c->d)) != hipSuccess) {
    (void)hipGetLastError();
    return refuse("factor array does not fit on the device (" + std::to_string(bytes_F(c->d) >> 20) +
                  " MiB): use the default fast mode without NDLQR_FLAG_KEEP_FACT, or a smaller batch");
  }
  // Structural zeros of F are never written by the kernels; zero once so that the factor
  // download matches the reference's calloc'ed array (src/nddata.c:34).
  HIP_TRY(hipMemsetAsync(c->F, 0, bytes_F(c->d), c->set[c->cur].stream));
  return NDLQR_OK;
}

int ndlqr_hip_set_flags(NdlqrHipCtx* c, unsigned flags) {
  if (!c) return NDLQR_ERR_INVALID;
  c->flags = flags;
  return NDLQR_OK;
}
unsigned ndlqr_hip_get_flags(const NdlqrHipCtx* c) { return c ? c->flags : 0u; }

int ndlqr_hip_set_stream(NdlqrHipCtx* c, void* hip_stream) {
  if (!c) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  {
    const int perr = ndlqr_hip_set_pipeline_depth(c, c->pipeline);  // drains both sets, primary set current
    if (perr) return perr;
  }
  BufferSet& s = c->set[0];
  if (c->own_stream && s.stream) HIP_TRY(hipStreamDestroy(s.stream));
  if (hip_stream) {
    s.stream = (hipStream_t)hip_stream;
    c->own_stream = false;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return NDLQR_OK;
}
void* ndlqr_hip_get_stream(NdlqrHipCtx* c) { return c ? (void*)c->set[c->cur].stream : nullptr; }

// The right-hand side exists once per buffer set of the pipeline (hip_context.hpp: rhs_latest / rhs_gen).
// rhs_written_cur: the parts of `mask` of the CURRENT set's copy have just been (re)written.
static void rhs_written_cur(NdlqrHipCtx* c, unsigned mask) {
  for (int p = 0; p < 4; ++p)
    if (mask & (1u << p)) c->set[c->cur].rhs_gen[p] = ++c->rhs_latest[p];
}
// rhs_make_current: the current set's copy is brought up to date in the parts of `need` before a solve reads it. Only a
// change of flow gets here with something to do (full MPC steps followed by x0-only steps, a plain solve behind steps,
// the first solve on the other set after an upload): everything in flight is waited for, the stale parts are copied
// from the other set on this set's stream, and the other set's stream waits for that copy before it may rewrite its own.
static int rhs_make_current(NdlqrHipCtx* c, unsigned need) {
  BufferSet& s = c->set[c->cur];
  const BufferSet& o = c->set[1 - c->cur];
  unsigned stale = 0;
  for (int p = 0; p < 4; ++p)
    if ((need & (1u << p)) && s.rhs_gen[p] < c->rhs_latest[p]) stale |= 1u << p;
  if (!stale || !o.rhs) return NDLQR_OK;
  HIP_TRY(sync_all(c));
  hipLaunchKernelGGL(ndlqr::copy_rhs_parts_generic, dim3(c->d.N, c->d.batch), dim3(64), 0, s.stream, c->d, stale,
                     (const double*)o.rhs, s.rhs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev_inputs, s.stream));
  if (o.stream) HIP_TRY(hipStreamWaitEvent(o.stream, c->ev_inputs, 0));
  for (int p = 0; p < 4; ++p)
    if (stale & (1u << p)) s.rhs_gen[p] = c->rhs_latest[p];
  return NDLQR_OK;
}

// the other buffer set's stream waits for everything enqueued on the current one so far
static hipError_t other_stream_waits(NdlqrHipCtx* c) {
  const hipStream_t other = c->set[1 - c->cur].stream;
  if (!other) return hipSuccess;
  const hipError_t e = hipEventRecord(c->ev_inputs, c->set[c->cur].stream);
  return e != hipSuccess ? e : hipStreamWaitEvent(other, c->ev_inputs, 0);
}

// the current buffer set holds new A, B, Q, R and a whole new right-hand side: neither a cached factor array nor cached
// records match them any more
static void note_new_inputs(NdlqrHipCtx* c) {
  rhs_written_cur(c, 0xFu);
  next_solve_on_current_set(c);
  c->kept.forget_factorisation();
  c->inputs_replaced = true;
  c->forget_shifted();
}

int ndlqr_hip_upload_inputs(NdlqrHipCtx* c, int p0, int count, const double* AB, const double* QR,
                            const double* rhs) {
  if (!c || !AB || !QR || !rhs || p0 < 0 || count <= 0 || p0 + count > c->d.batch) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  BufferSet& s = c->set[c->cur];
  HIP_TRY(sync_all(c));  // solves in flight on either slot still read the inputs
  {  // (a partial upload lands on a complete, current copy: the other set then takes the whole of it on its next use)
    const int merr = rhs_make_current(c, 0xFu);
    if (merr) return merr;
  }
  if (c->padded) {  // the caller's layout goes to a staging array in HBM, a kernel files it into the padded arrays
    const ndlqr::Dims& u = c->du;
    const size_t uAB = (size_t)u.N * u.n * u.w * count, uQR = (size_t)u.N * u.w * count, uz = (size_t)u.N * u.rows * count;
    HIP_TRY(c->grow_pad_stage(uAB + uQR + uz));
    double* s0 = c->pad_stage;
    HIP_TRY(hipMemcpyAsync(s0, AB, sizeof(double) * uAB, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s0 + uAB, QR, sizeof(double) * uQR, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s0 + uAB + uQR, rhs, sizeof(double) * uz, hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(ndlqr::pad_inputs_generic, dim3(d.N, count), dim3(128), 0, s.stream, u, d, p0, s0, s0 + uAB,
                       s0 + uAB + uQR, c->AB, c->QR, s.rhs);
    HIP_TRY(hipGetLastError());
  } else {
    const size_t sAB = (size_t)d.N * d.n * d.w, sQR = (size_t)d.N * d.w, sz = (size_t)d.N * d.rows;
    HIP_TRY(hipMemcpyAsync(c->AB + p0 * sAB, AB, sizeof(double) * sAB * count, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(c->QR + p0 * sQR, QR, sizeof(double) * sQR * count, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s.rhs + p0 * sz, rhs, sizeof(double) * sz * count, hipMemcpyHostToDevice, s.stream));
  }
  HIP_TRY(hipStreamSynchronize(s.stream));  // the host staging buffers are reused by the caller
  note_new_inputs(c);
  c->cost.dense = false;
  return NDLQR_OK;
}

int ndlqr_hip_pack_flat_device(NdlqrHipCtx* c, const double* A, const double* B, const double* Q,
                               const double* R, const double* q, const double* r, const double* d,
                               const double* x0) {
  if (!c || !A || !B || !Q || !R || !q || !r || !d || !x0) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  BufferSet& s = c->set[c->cur];
  HIP_TRY(sync_all(c));  // solves in flight on either slot still read the inputs
  // (eight knots per workgroup while a thread's eight loads -- the same entry of eight consecutive blocks -- stay within what
  //  the caches hold together: at (64,16) the strided reads of eight 40 KB blocks at once took 9.5 instead of 5 ms)
  const bool hp = c->du.N != c->d.N;  // padded horizon: the per-knot guards of the pack kernels
  if (c->d.N % 8 == 0 && c->du.n <= 16 && hp)
    hipLaunchKernelGGL((ndlqr::pack_flat_generic<8, true>), dim3(c->d.N / 8, c->d.batch), dim3(128), 0, s.stream, c->du, c->d, A,
                       B, Q, R, q, r, d, x0, c->AB, c->QR, s.rhs);
  else if (c->d.N % 8 == 0 && c->du.n <= 16)
    hipLaunchKernelGGL(ndlqr::pack_flat_generic<8>, dim3(c->d.N / 8, c->d.batch), dim3(128), 0, s.stream, c->du, c->d, A, B, Q,
                       R, q, r, d, x0, c->AB, c->QR, s.rhs);
  else if (c->du.n > 16 && sizeof(double) * (size_t)(c->du.n | 1) * c->du.w <= kLdsDefaultDynamic)  // through LDS, whole lines in and out
    hipLaunchKernelGGL(ndlqr::pack_flat_tiled, dim3(c->d.N, c->d.batch), dim3(256), sizeof(double) * (size_t)(c->du.n | 1) * c->du.w,
                       s.stream, c->du, c->d, A, B, Q, R, q, r, d, x0, c->AB, c->QR, s.rhs);
  else if (hp)
    hipLaunchKernelGGL((ndlqr::pack_flat_generic<1, true>), dim3(c->d.N, c->d.batch), dim3(128), 0, s.stream, c->du, c->d, A, B,
                       Q, R, q, r, d, x0, c->AB, c->QR, s.rhs);
  else
    hipLaunchKernelGGL(ndlqr::pack_flat_generic<1>, dim3(c->d.N, c->d.batch), dim3(128), 0, s.stream, c->du, c->d, A, B, Q, R,
                       q, r, d, x0, c->AB, c->QR, s.rhs);
  HIP_TRY(hipGetLastError());
  note_new_inputs(c);              // (the whole batch: nothing of the older copies is needed any more)
  c->cost.dense = false;           // (ndlqr_hip_init_dense, which gets here with the reduced arrays, sets it again)
  HIP_TRY(other_stream_waits(c));  // the next solve may run on the other buffer set's stream
  return NDLQR_OK;
}

int ndlqr_hip_device_pointers(NdlqrHipCtx* c, void** out5) {
  if (!c || !out5) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_device_pointers")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_device_pointers")) return cerr;
  if (c->padded)
    return refuse("no raw device pointers for a block size that runs zero-padded (the arrays have another layout): "
                  "use ndlqr_hip_pack_flat_device, or NDLQR_NO_PAD=1");
  const int ferr = ndlqr_hip_ensure_F(c);  // the caller asks for the factor array: it has to exist
  if (ferr) return ferr;
  const int perr = ndlqr_hip_set_pipeline_depth(c, 1);  // the caller holds raw pointers: one buffer set from now on
  if (perr) return perr;
  out5[0] = c->AB; out5[1] = c->QR; out5[2] = c->set[0].rhs; out5[3] = c->F; out5[4] = c->set[0].z;
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ launches

// lean (fast mode without KEEP): the Schur passes only keep the boundary knots of every subtree
// up to date, the solution comes from the back-substitution over the separator records.
constexpr int kSepChunkTiles = 3;  // column tiles of the right-hand-side panel resident in LDS (separator_mfma)

// Separator-only schedule for blocks that fill 16x16 matrix-core tiles (kernels_reduced_mfma.hpp): workgroup
// size and LDS of separator_reduced_mfma, or false when the shape does not qualify (-> generic-lean).
struct ReducedGenericPlan {
  bool ok;
  int threads;
  size_t lds;
  int nb;    // 16 x 16 tiles per block row
  bool pad;  // the block does not fill them
  bool keep; // NDLQR_FLAG_KEEP_RECORDS
};
static ReducedGenericPlan plan_reduced_generic(const NdlqrHipCtx* c) {
  const ndlqr::Dims& d = c->d;
  ReducedGenericPlan p = {false, 0, 0, 0, false, false};
  if (c->flags & (NDLQR_FLAG_STRICT_FP | NDLQR_FLAG_KEEP_FACT)) return p;
  if (c->knobs.no_mfma || c->knobs.no_reduced_generic || d.n > 128 || d.N < 2) return p;
  p.keep = (c->flags & NDLQR_FLAG_KEEP_RECORDS) != 0;  // W of every separator kept for rhs-only re-solves
  p.nb = (d.n + 15) / 16;
  const int npad = 16 * p.nb, wpad = (d.w + 3) / 4 * 4;
  p.pad = npad != d.n || wpad != d.w;  // blocks that do not fill their tiles: zero-padded in LDS (PAD instances)
  // one wavefront per 16x16 block where the weights fit its lanes: many small workgroups fill the chip better than
  // a four-wavefront workgroup whose phases are mostly serial at this size
  // a wavefront per 16-column tile where the weights fit the lanes ("two rounds", kernels_reduced_mfma.hpp: small
  // workgroups, three or more of them per CU), else twice that
  p.threads = wpad <= 64 * p.nb ? 64 * p.nb : (p.nb >= 3 ? 512 : 256);
  if (wpad > p.threads) return p;  // one weight / rhs entry per thread
  if (p.nb >= 5 && p.threads != 64 * p.nb) return p;  // (beyond 64 states the second panel array does not fit the LDS)
  p.lds = sizeof(double) * (size_t)ndlqr::reduced_lds_doubles(npad, wpad, p.threads == 64 * p.nb);
  if (p.lds > kLdsMax) return p;
  p.ok = true;
  return p;
}

static size_t doubles_red_generic(const ndlqr::Dims& d) {
  return (size_t)d.batch * (d.N / 2) * (4 * (size_t)d.n * d.n + 2 * d.n);
}

// slots of the separators of level >= 1 (runtime-sized separator-only schedule); allocated by the first
// solve that takes it, for both buffer sets of the pipeline. Never zeroed: the level-0 launch stores
// every accumulator block. Must run outside stream capture.
static int ensure_red_generic(NdlqrHipCtx* c) {
  if (c->d.N < 4) return NDLQR_OK;  // a single separator: no slots
  const size_t need = doubles_red_generic(c->d);
  for (BufferSet& s : c->set) {
    if (!s.ready || s.red.count() >= need) continue;
    // (a context of a size-specialised shape under NDLQR_FLAG_GENERIC comes with the smaller array of ITS schedule)
    HIP_TRY(sync_all(c));
    s.graph.reset();  // a launch sequence captured on this buffer set holds the old address
    if (s.red.grow(need) != hipSuccess) {
      (void)hipGetLastError();
      g_last_error = "accumulator slots of the separator-only schedule do not fit on the device";
      return NDLQR_ERR_INVALID;
    }
    // (zeros for the size-specialised schedule, should the context go back to it. hipMemset runs on the null
    //  stream and may return before it is done; the solver's streams are non-blocking: wait here, or the
    //  level-0 launch races with it)
    HIP_TRY(hipMemset(s.red, 0, sizeof(double) * need));
    HIP_TRY(hipDeviceSynchronize());
  }
  return NDLQR_OK;
}

// back-substitution of the runtime-sized separator-only schedule: its records are compact (the Cholesky factor and y~ instead of
// f_a | f_bb | z_sep, the couplings come from the slots / the problem data), and one launch resolves the level-0
// multipliers and the states / inputs of every knot
static void launch_backsub_reduced_generic(NdlqrHipCtx* c, const double* rhs, double* z) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  ScopedSlot t(c, SLOT_APPLY);
  const size_t lds_m = sizeof(double) * ((size_t)d.n * (d.n + 1) / 2 + 2 * (size_t)d.n + 16);
  // (rows of CA | CB eight per wavefront. Four wavefronts per separator leave a CU a quarter full at small blocks: one up to
  //  32 states, two up to 64, four beyond -- profiles/r04_mult_threads_ab.txt: (16,4,256) x 1024 2.30 -> 1.86 ms per solve,
  //  (20,20) 1.32 -> 1.23, (48,16,512) 6.44 -> 6.27, (96,16) best at four; NDLQR_MULT_THREADS overrides)
  const int thr_env = c->knobs.mult_threads;
  const int thr_m = (thr_env == 64 || thr_env == 128 || thr_env == 256) ? thr_env : (d.n <= 32 ? 64 : (d.n <= 64 ? 128 : 256));
  // A step that wants knots [k0, k1] alone (NDLQR_SOLN_ONLY: apply_blk0 / apply_nblk in units of eight knots): of every
  // level the separators whose subtree meets [k0 - 1, k1 + 2] -- a set closed under "needs the multipliers of the
  // separators bounding its subtree" (those are ancestors: their subtrees contain it) --, of level 0 the pairs of the range
  const bool part = c->apply_nblk > 0;
  const int k0 = 8 * c->apply_blk0;  // (< N: the selection lies inside the horizon)
  const int k1 = 8 * (c->apply_blk0 + c->apply_nblk) - 1 < d.N ? 8 * (c->apply_blk0 + c->apply_nblk) - 1 : d.N - 1;  // (horizons below 8 knots)
  const int ka = k0 > 0 ? k0 - 1 : 0, kb = k1 + 2 < d.N ? k1 + 2 : d.N - 1;
  for (int l = d.K - 1; l >= 1; --l) {
    ndlqr::Dims dl = d;
    int cnt = d.N >> (l + 1);
    if (part) { dl.xoff = ka >> (l + 1); cnt = (kb >> (l + 1)) - dl.xoff + 1; }
    hipLaunchKernelGGL(ndlqr::backsub_multipliers_compact, dim3(cnt, d.batch), dim3(thr_m), lds_m, s.stream, dl, l,
                       s.red, s.rec, z);
  }
  const int thr = d.n <= 16 ? 64 : (d.n <= 32 ? 128 : 256);  // (its y_s step wants n <= threads)
  const size_t lds = sizeof(double) * ((size_t)d.n * (d.n + 1) / 2 + 5 * (size_t)d.n + 4 * (size_t)d.w + 2 * (size_t)d.rows + thr);
  ndlqr::Dims d0 = d;
  if (part) d0.xoff = k0 >> 1;
  hipLaunchKernelGGL(ndlqr::backsub_level0_states_generic, dim3(part ? (k1 >> 1) - (k0 >> 1) + 1 : d.N >> 1, d.batch), dim3(thr),
                     lds, s.stream, d0, c->AB, c->QR, rhs, s.rec, z);
}

static int launch_reduced_generic(NdlqrHipCtx* c, const ReducedGenericPlan& p) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  for (int l = 0; l < d.K; ++l) {
    ScopedSlot t(c, SLOT_SEP);
    const dim3 grid(d.N >> (l + 1), d.batch);
#define NDLQR_LAUNCH_SEP2(NB_, NT_, L0_, PAD_)                                                                     \
  hipLaunchKernelGGL((ndlqr::separator_reduced_mfma<NB_, NT_, L0_, PAD_>), grid, dim3(NT_), p.lds, s.stream, d, l, \
                     c->AB, c->QR, s.rhs, s.red, s.rec, c->info)
#define NDLQR_LAUNCH_SEP(NB_, NT_)                                          \
  do {                                                                      \
    if (l == 0 && p.pad) NDLQR_LAUNCH_SEP2(NB_, NT_, true, true);           \
    else if (l == 0) NDLQR_LAUNCH_SEP2(NB_, NT_, true, false);              \
    else if (p.pad) NDLQR_LAUNCH_SEP2(NB_, NT_, false, true);               \
    else NDLQR_LAUNCH_SEP2(NB_, NT_, false, false);                         \
  } while (0)
    switch (p.nb) {
      case 1:
        if (p.threads == 64) NDLQR_LAUNCH_SEP(1, 64);
        else NDLQR_LAUNCH_SEP(1, 256);
        break;
      case 2:
        if (p.threads == 128) NDLQR_LAUNCH_SEP(2, 128);
        else NDLQR_LAUNCH_SEP(2, 256);
        break;
      case 3:
        if (p.threads == 192) NDLQR_LAUNCH_SEP(3, 192);
        else NDLQR_LAUNCH_SEP(3, 512);
        break;
      case 4:
        if (p.threads == 256) NDLQR_LAUNCH_SEP(4, 256);
        else NDLQR_LAUNCH_SEP(4, 512);
        break;
      case 5:  // (beyond 64 states: one workgroup per CU, the form with one wavefront per tile column only)
        NDLQR_LAUNCH_SEP(5, 320);
        break;
      case 6:
        NDLQR_LAUNCH_SEP(6, 384);
        break;
      case 7:
        NDLQR_LAUNCH_SEP(7, 448);
        break;
      default:
        NDLQR_LAUNCH_SEP(8, 512);
        break;
    }
#undef NDLQR_LAUNCH_SEP2
#undef NDLQR_LAUNCH_SEP
  }
  launch_backsub_reduced_generic(c, s.rhs, s.z);
  return NDLQR_OK;
}

// rhs-only re-solve on the records, slots and separator factors of a generic-reduced-records sweep: right-hand side
// `rhs`, solution into `z` (the primal ones, or those of the adjoint solve)
static void launch_rhs_reduced_generic(NdlqrHipCtx* c, const double* rhs, double* z) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  const int np = (d.n + 15) / 16 * 16;
  const size_t lds = sizeof(double) * (2 * (size_t)d.w + d.n + 3 * (size_t)np + 256 + (size_t)d.n * (d.n + 1) / 2);
  for (int l = 0; l < d.K; ++l) {
    ScopedSlot t(c, SLOT_SEP);
    hipLaunchKernelGGL(ndlqr::rhs_reduced_generic, dim3(d.N >> (l + 1), d.batch), dim3(256), lds, s.stream, d, l, np,
                       c->AB, c->QR, rhs, s.red, s.rec);
  }
  launch_backsub_reduced_generic(c, rhs, z);
}

// The separator kernel of the knot-based runtime-sized schedules and where its S-bar (n x (n+1)) and right-hand-side panel
// (n x (2n+1)) live: separator_mfma (fast mode, blocks that fill 16x16 tiles; the panel goes through LDS in chunks of
// kSepChunkTiles column tiles, + the inverses of the 16x16 diagonal blocks, pitch 17) while its LDS and its wavefronts
// fit a workgroup; else separator_generic with both arrays in LDS; else -- blocks beyond ~80 states -- separator_generic
// with both arrays in global memory (NdlqrHipCtx::sep_scratch): every mode, any block size the device holds.
struct GenericSepPlan {
  bool mfma;
  bool scratch;
  size_t lds;
  int threads;
  int schur_nb;  // the Schur update beside it: schur_mfma<schur_nb> (1 .. 4), schur_mfma_rt (0) or schur_generic (-1)
};
static GenericSepPlan plan_generic_sep(const NdlqrHipCtx* c, const bool strict) {
  const ndlqr::Dims& d = c->d;
  GenericSepPlan p;
  // block sizes that fill 16x16 MFMA tiles: Schur update on the fp64 matrix cores (fast mode; beyond 64 states the
  // runtime-sized form)
  p.schur_nb = (strict || d.n % 16 != 0 || c->knobs.no_mfma) ? -1 : (d.n > 64 ? 0 : (d.rows % 16 == 0 ? d.n / 16 : -1));
  p.mfma = !strict && d.n % 16 == 0 && d.w % 4 == 0 && !c->knobs.no_mfma;
  p.scratch = false;
  const int ctl = 2 * (d.n / 16) + 1, ctc = ctl < kSepChunkTiles ? ctl : kSepChunkTiles;
  const size_t lds_mfma = sizeof(double) * ((size_t)d.n * (d.n + 1) + (size_t)d.n * (16 * ctc + 1) + (size_t)d.n * 17);
  const size_t lds_generic = sizeof(double) * ((size_t)d.n * (d.n + 1) + (size_t)d.n * (2 * d.n + 1));
  // matrix-core separator: one wavefront per 16x16 tile of the products / updates; 512 threads let two
  // workgroups (67 KB of LDS each at n = 64) share a CU
  p.threads = c->knobs.sep_threads > 0 ? c->knobs.sep_threads : (d.n >= 32 ? 512 : 256);
  if (p.mfma) {  // separator_mfma: a wavefront per tile of a block row of W, at most three panel tiles per wavefront
    const int need = (d.n / 16) > ((d.n / 16) * ctc + 2) / 3 ? (d.n / 16) : ((d.n / 16) * ctc + 2) / 3;
    if (p.threads < 64 * need) p.threads = 64 * need;
    if (p.threads > 1024) p.mfma = false;
  }
  if (p.mfma) {
    // (beyond 112 states S-bar / L goes to global memory: the panel chunk and the inverses of the diagonal blocks stay)
    const size_t lds_no_s = lds_mfma - sizeof(double) * (size_t)d.n * (d.n + 1);
    if (lds_mfma <= kLdsMax) { p.lds = lds_mfma; return p; }
    if (lds_no_s <= kLdsMax) { p.lds = lds_no_s; p.scratch = true; return p; }
    p.mfma = false;
  }
  p.scratch = lds_generic > kLdsMax;
  p.lds = p.scratch ? 0 : lds_generic;
  p.threads = p.scratch ? 1024 : 256;
  return p;
}

// Everything a solve decides before it launches, by plan_solve (below) from the block sizes, the flags, the NDLQR_*
// switches read at creation and the optional buffers of the primary set: which launch sequence runs, what that needs
// allocated (prepare_solve) and what it leaves behind (launch_solve). The launch functions get it and only issue launches.
struct SolvePlan {
  Family family;
  const SmallInstance* inst;  // Family::Small
  SmallPlan small;            // ... and what its launch_small does
  ReducedGenericPlan red;     // Family::GenericReduced (red.ok)
  GenericSepPlan sep;         // Family::GenericKnot: its separator and Schur kernels
  bool strict, keep;          // NDLQR_FLAG_STRICT_FP, NDLQR_FLAG_KEEP_FACT
  bool lean;                  // Family::GenericKnot, fast mode without KEEP: the Schur passes only keep the boundary knots of
                              // every subtree up to date, the solution comes from the back-substitution over the records
  bool rec_as_factors;        // NDLQR_FLAG_KEEP_RECORDS where no schedule keeps records (Family::GenericKnot: blocks beyond 128
                              // states, inputs wider than a workgroup): the factor array is kept instead, the re-solve is the
                              // factor-based sweep
  // what has to exist before the launches (and any capture of them)
  bool needs_F;               // the factor array (ndlqr_hip_ensure_F)
  size_t sep_scratch_bytes;   // NdlqrHipCtx::sep_scratch (0: not used)
  bool needs_red_generic;     // the runtime-sized slots (ensure_red_generic)
  bool may_pipeline;          // nothing but records and the solution stay: may alternate between the two buffer sets
  KeptState kept;             // what the solve leaves (fact_valid: a complete factor array)
};

template <bool STRICT>
static int launch_generic(NdlqrHipCtx* c, const SolvePlan& plan) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  const bool lean = plan.lean;
  double* rec = lean ? s.rec : nullptr;
  {
    ScopedSlot t(c, SLOT_LEAF);
    hipLaunchKernelGGL((ndlqr::leaf_generic<STRICT>), dim3(d.N, d.batch), dim3(128), 0, s.stream, d,
                       c->AB, c->QR, s.rhs, c->F, s.z, c->info, lean ? 1 : 0);
  }
  // S (n x (n+1)) + right-hand-side panel (n x (2n+1)); on the matrix-core path the panel goes through
  // LDS in chunks of kSepChunkTiles column tiles (+ the inverses of the 16x16 diagonal blocks, pitch 17)
  const GenericSepPlan& sp = plan.sep;
  const bool p1mfma = sp.mfma;
  const size_t lds = sp.lds;
  const int sep_threads = sp.threads;
  double* sep_scratch = sp.scratch ? c->sep_scratch : nullptr;  // (allocated by prepare_solve)
  for (int l = 0; l < d.K; ++l) {
    const int nsub = d.N >> (l + 1);
    {
      ScopedSlot t(c, SLOT_SEP);
      if (p1mfma)
        hipLaunchKernelGGL((ndlqr::separator_mfma<kSepChunkTiles>), dim3(nsub, d.batch), dim3(sep_threads), lds,
                           s.stream, d, l, c->AB, c->F, s.z, c->info, rec, sep_scratch,
                           (size_t)d.n * (d.n + 1) + (size_t)d.n * (2 * d.n + 1));
      else
        hipLaunchKernelGGL((ndlqr::separator_generic<STRICT>), dim3(nsub, d.batch), dim3(sep_threads), lds,
                           s.stream, d, l, c->AB, c->F, s.z, c->info, rec, sep_scratch);
    }
    if (lean && l == d.K - 1) break;  // nothing above the root separator
    {
      ScopedSlot t(c, lean ? SLOT_BOUNDARY : SLOT_SCHUR);
      const int bnd = lean ? 1 : 0;
      const unsigned gx = lean ? 2u * (unsigned)nsub : (unsigned)d.N;  // knots this pass updates
      const size_t flds = sizeof(double) * (size_t)d.n * (d.n + 16);
      if (sp.schur_nb == 4)
        hipLaunchKernelGGL((ndlqr::schur_mfma<4>), dim3(gx, d.batch), dim3(256), flds, s.stream, d, l, c->F, s.z, bnd,
                           (const double*)rec);
      else if (sp.schur_nb == 3)
        hipLaunchKernelGGL((ndlqr::schur_mfma<3>), dim3(gx, d.batch), dim3(256), flds, s.stream, d, l, c->F, s.z, bnd,
                           (const double*)rec);
      else if (sp.schur_nb == 2)
        hipLaunchKernelGGL((ndlqr::schur_mfma<2>), dim3(gx, d.batch), dim3(256), flds, s.stream, d, l, c->F, s.z, bnd,
                           (const double*)rec);
      else if (sp.schur_nb == 1)
        hipLaunchKernelGGL((ndlqr::schur_mfma<1>), dim3(gx, d.batch), dim3(256), flds, s.stream, d, l, c->F, s.z, bnd,
                           (const double*)rec);
      else if (sp.schur_nb == 0)  // (runtime-sized matrix-core form: blocks beyond 64 states)
        hipLaunchKernelGGL(ndlqr::schur_mfma_rt, dim3(gx, d.batch), dim3(256), 0, s.stream, d, l, c->F, s.z, bnd,
                           (const double*)rec);
      else {
        const long work = (long)gx * d.rows * d.n;
        hipLaunchKernelGGL((ndlqr::schur_generic<STRICT>), dim3((unsigned)((work + 255) / 256), d.batch),
                           dim3(256), 0, s.stream, d, l, c->F, s.z, bnd, (const double*)rec);
      }
    }
  }
  if (lean) {
    ScopedSlot t(c, SLOT_APPLY);
    for (int l = d.K - 1; l >= 0; --l) {
      hipLaunchKernelGGL(ndlqr::backsub_multipliers_generic, dim3(d.N >> (l + 1), d.batch), dim3(64), 0, s.stream,
                         d, l, s.rec, s.z);
    }
    const int work = d.N * d.rows;
    hipLaunchKernelGGL(ndlqr::backsub_states_generic, dim3((work + 255) / 256, d.batch), dim3(256), 0, s.stream, d,
                       c->AB, c->QR, s.rhs, s.z);
  }
  return NDLQR_OK;
}

// ---- size-specialised instances: one translation unit each (small_instance.hip), listed in
//      small_instances.def; developer builds with NDLQR_SINGLE_TU (tools/segtime.py) hold every instance here
#ifdef NDLQR_SINGLE_TU
#define NDLQR_SMALL_INSTANCE(NX_, NU_) static const SmallInstance NDLQR_SMALL_NAME(NX_, NU_) = make_small_instance<NX_, NU_>();
#else
#define NDLQR_SMALL_INSTANCE(NX_, NU_) extern const SmallInstance NDLQR_SMALL_NAME(NX_, NU_);
#endif
#include "small_instances.def"
#undef NDLQR_SMALL_INSTANCE

static const SmallInstance* const kSmallInstances[] = {
#define NDLQR_SMALL_INSTANCE(NX_, NU_) &NDLQR_SMALL_NAME(NX_, NU_),
#include "small_instances.def"
#undef NDLQR_SMALL_INSTANCE
};

static bool has_small_instance(int nstates, int ninputs) {
  for (const SmallInstance* s : kSmallInstances)
    if (s->nx == nstates && s->nu == ninputs) return true;
  return false;
}

// cheapest instance (with a matrix-core path: six states or more) that contains the block size; *pn, *pm untouched
// when there is none
static void pick_pad_instance(int nstates, int ninputs, int* pn, int* pm) {
  long best = -1;
  for (const SmallInstance* si : kSmallInstances) {
    if (si->nx < nstates || si->nu < ninputs || si->nx < 6) continue;
    const long cost = (long)si->nx * si->nx * (si->nx + si->nu);
    if (best < 0 || cost < best) { best = cost; *pn = si->nx; *pm = si->nu; }
  }
}

static const SmallInstance* find_small(const ndlqr::Dims& d) {
  for (const SmallInstance* s : kSmallInstances)
    if (s->nx == d.n && s->nu == d.m) return s;
  return nullptr;
}

// the size-specialised instance that serves this context (nullptr: runtime-sized kernels)
static const SmallInstance* pick_small(const NdlqrHipCtx* c) {
  const ndlqr::Dims& d = c->d;
  if (c->flags & NDLQR_FLAG_GENERIC) return nullptr;
  const SmallInstance* inst = find_small(d);
  // the fused kernels own eight knots per workgroup and two tree levels: shorter horizons run the
  // runtime-sized kernels
  if (!inst || d.N < inst->kpb || d.K < 3) return nullptr;
  return inst;
}

// the instance whose records the last factorisation left (nullptr: none, or another family's)
static const SmallInstance* kept_instance(const NdlqrHipCtx* c) {
  return c->kept.family == Family::Small ? find_small(c->d) : nullptr;
}

static SolvePlan plan_solve(const NdlqrHipCtx* c) {
  const ndlqr::Dims& d = c->d;
  SolvePlan p = {};
  p.strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  p.keep = (c->flags & NDLQR_FLAG_KEEP_FACT) != 0;
  p.inst = pick_small(c);
  if (p.inst) {
    p.family = Family::Small;
    p.small = p.inst->plan(c, p.strict, p.keep);
    p.needs_F = p.small.needs_F;
    p.kept.schedule = p.small.schedule;
    p.kept.rec_complete = p.small.rec_complete;
    p.kept.rec_compact = p.small.rec_compact;
  } else if ((p.red = plan_reduced_generic(c)).ok) {
    p.family = Family::GenericReduced;
    p.needs_red_generic = true;
    p.kept.schedule = p.red.keep ? "generic-reduced-records" : "generic-reduced";
    p.kept.rec_complete = p.red.keep;  // records, slots and W of every separator stay: rhs-only re-solves (launch_rhs_reduced_generic)
  } else {
    p.family = Family::GenericKnot;
    p.rec_as_factors = (c->flags & NDLQR_FLAG_KEEP_RECORDS) && !p.strict;
    p.lean = !p.strict && !p.keep && !p.rec_as_factors;
    p.needs_F = true;
    p.sep = plan_generic_sep(c, p.strict);
    // a block too large for the separator kernel's LDS: S-bar and the panel of every level-0 separator in global memory
    if (p.sep.scratch)
      p.sep_scratch_bytes = sizeof(double) * ((size_t)d.n * (d.n + 1) + (size_t)d.n * (2 * d.n + 1)) * (size_t)d.batch *
                            (d.N / 2 > 0 ? d.N / 2 : 1);
    p.kept.schedule = p.lean ? "generic-lean" : (p.strict ? "generic-strict" : "generic-keep");
  }
  p.kept.family = p.family;
  // a complete factor array is on the device with KEEP, and on the strict runtime-sized path
  p.kept.fact_valid = p.keep || p.rec_as_factors || ((c->flags & NDLQR_FLAG_GENERIC) && p.strict);
  // Two-deep pipeline: solves that leave nothing behind but records and the solution may alternate between two buffer
  // sets. Everything else -- factor array, kept records, per-kernel events -- stays stream-ordered on the primary set.
  p.may_pipeline = !p.needs_F && !(c->flags & (NDLQR_FLAG_PROFILE | NDLQR_FLAG_KEEP_RECORDS | NDLQR_FLAG_KEEP_FACT));
  return p;
}

// Enqueue leaf/bottom + per-level + apply launches on the context's stream.
static int enqueue_solve(NdlqrHipCtx* c, const SolvePlan& plan) {
  BufferSet& s = c->set[c->cur];
  // (the failure counters are cumulative: no memset node; the host subtracts what it has seen)
  int err = NDLQR_OK;
  switch (plan.family) {
    case Family::Small: err = plan.inst->solve(c, plan.small); break;
    case Family::GenericReduced: err = launch_reduced_generic(c, plan.red); break;
    default: err = plan.strict ? launch_generic<true>(c, plan) : launch_generic<false>(c, plan); break;
  }
  // the batch-wide failure count travels to pinned host memory behind the last kernel: the host
  // reads it after the stream synchronisation without another blocking copy
  if (!err) HIP_TRY(hipMemcpyAsync(s.h_fail, c->info + c->d.batch, sizeof(int), hipMemcpyDeviceToHost, s.stream));
  return err;
}

// first half of a solve: its plan (*plan), the allocations that asks for, recovery from a failed solve, choice of the
// buffer set (c->cur on return).
static int prepare_solve(NdlqrHipCtx* c, SolvePlan* plan) {
  HIP_TRY(hipSetDevice(c->device));
  *plan = plan_solve(c);
  // before any capture starts: allocation is not a stream operation
  if (plan->needs_F) {
    const int ferr = ndlqr_hip_ensure_F(c);
    if (ferr) return ferr;
  }
  if (plan->sep_scratch_bytes && c->sep_scratch.ensure(plan->sep_scratch_bytes / sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return refuse("global scratch of the large-block separator kernel does not fit on the device (" +
                  std::to_string(plan->sep_scratch_bytes >> 20) + " MiB): use a smaller batch");
  }
  if (c->state_dirty) {
    // the previous solve did not launch or complete: its arrival counters may be odd and its failure
    // words meaningless -- start from zero (the kernels themselves leave both clean)
    (void)sync_all(c);
    const hipStream_t st = c->set[c->cur].stream;
    for (const BufferSet& s : c->set)
      if (s.tree_cnt) HIP_TRY(hipMemsetAsync(s.tree_cnt, 0, sizeof(int) * (size_t)c->d.batch * (c->d.N / 4), st));
    HIP_TRY(hipMemsetAsync(c->info, 0, sizeof(int) * ((size_t)c->d.batch + 1), st));
    HIP_TRY(hipStreamSynchronize(st));
    for (const BufferSet& s : c->set)
      if (s.h_fail) *s.h_fail = 0;
    c->fail_base = 0;
    c->state_dirty = false;
  }
  // (each set on its own stream, the other set may still be in flight; a caller-owned stream stays stream-ordered)
  const bool pipelined = c->pipeline >= 2 && c->own_stream && plan->may_pipeline;
  const bool want_alt = pipelined && (c->solve_count & 1u) && ensure_alt(c);
  if (!pipelined && c->set[1].stream) HIP_TRY(hipStreamSynchronize(c->set[1].stream));
  if (plan->needs_red_generic) {  // (after ensure_alt: both buffer sets get their slots)
    const int rerr = ensure_red_generic(c);
    if (rerr) return rerr;
  }
  c->cur = want_alt ? 1 : 0;
  ++c->solve_count;
  c->state_dirty = true;  // until this solve is known to have been enqueued completely
  return NDLQR_OK;
}

// The launch sequence `enqueue` issues on the current buffer set's stream, replayed as the hipGraph of `g`: a fixed chain
// of short launches, captured once (launch-bound single solves -- batch 1 -- gain the most) and again whenever the key it
// was captured under changes (the key determines the plan).
static int replay_chain(NdlqrHipCtx* c, CapturedChain& g, const SolvePlan& plan, int (*enqueue)(NdlqrHipCtx*, const SolvePlan&)) {
  const hipStream_t st = c->set[c->cur].stream;
  const unsigned apply = ((unsigned)c->apply_blk0 << 16) | (unsigned)c->apply_nblk;  // (restricted back-substitution of a step)
  if (!g.exec || g.flags != c->flags || g.stream != st || g.apply != apply) {
    g.reset();
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int err = enqueue(c, plan);
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (err) { if (graph) (void)hipGraphDestroy(graph); return err; }
    if (e != hipSuccess) return fail("hipStreamEndCapture", e);
    e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { g.exec = nullptr; return fail("hipGraphInstantiate", e); }
    g.flags = c->flags;
    g.stream = st;
    g.apply = apply;
  }
  HIP_TRY(hipGraphLaunch(g.exec, st));
  return NDLQR_OK;
}

// second half: the launch sequence on the current buffer set's stream (per-kernel events need eager launches)
static int launch_solve(NdlqrHipCtx* c, const SolvePlan& plan) {
  c->kept.rec_complete = c->kept.rec_compact = false;  // (the launches overwrite the records)
  const int err = (c->flags & NDLQR_FLAG_PROFILE) ? enqueue_solve(c, plan)
                                                  : replay_chain(c, c->set[c->cur].graph, plan, enqueue_solve);
  if (err) return err;
  HIP_TRY(hipGetLastError());
  note_solution(c);
  c->kept = plan.kept;
  c->inputs_replaced = false;
  c->forget_shifted();  // (the records / factors are those of the unshifted matrix now)
  ++c->factor_count;
  return NDLQR_OK;
}

int ndlqr_hip_solve_async(NdlqrHipCtx* c) {
  if (!c) return NDLQR_ERR_INVALID;
  SolvePlan plan;
  int err = prepare_solve(c, &plan);
  if (err) return err;
  BufferSet& s = c->set[c->cur];
  err = rhs_make_current(c, 0xFu);  // (this buffer set's copy of the right-hand side may be behind: steps write one set)
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  err = launch_solve(c, plan);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  c->timing_pending = true;
  c->state_dirty = false;
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ one-shot solve from pinned staging
// The drop-in ndlqr_Solve is a batch of one whose inputs come from the host and whose solution goes back to it on
// every call (src/solve.c:38-201 works on host memory). Doing that with the batch functions costs three blocking
// uploads, a launch, and a blocking download -- four host synchronisations around 40 us of kernels. Here the caller
// packs straight into pinned staging (ndlqr_hip_staged_io), and ndlqr_hip_solve_staged replays ONE captured graph:
// AB, QR, rhs up (copy nodes), the launch chain of the schedule, the solution blocks down; one launch, one
// synchronisation. Stream-ordered on the primary buffer set (pipeline depth 1 from then on).
static size_t staged_doubles(const ndlqr::Dims& u, size_t* oAB, size_t* oQR, size_t* orhs, size_t* oz) {
  const size_t nAB = (size_t)u.batch * u.N * u.n * u.w, nQR = (size_t)u.batch * u.N * u.w, nz = (size_t)u.batch * u.N * u.rows;
  *oAB = 0; *oQR = nAB; *orhs = nAB + nQR; *oz = nAB + nQR + nz;
  return nAB + nQR + 2 * nz;
}

int ndlqr_hip_staged_io(NdlqrHipCtx* c, double** AB, double** QR, double** rhs, double** z) {
  if (!c || !AB || !QR || !rhs || !z) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_staged_io")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_staged_io")) return cerr;
  HIP_TRY(hipSetDevice(c->device));
  size_t oAB, oQR, orhs, oz;
  const size_t total = staged_doubles(c->du, &oAB, &oQR, &orhs, &oz);
  if (!c->h_io) {
    HIP_TRY(c->h_io.ensure(total));
    if (c->padded) {  // (caller-layout staging in HBM for both directions; allocated outside any capture)
      HIP_TRY(c->grow_pad_stage(total));
    }
    const int perr = ndlqr_hip_set_pipeline_depth(c, 1);
    if (perr) return perr;
  }
  *AB = c->h_io + oAB; *QR = c->h_io + oQR; *rhs = c->h_io + orhs; *z = c->h_io + oz;
  return NDLQR_OK;
}

// the copies around the launch chain, on the context's stream (captured, or eager under NDLQR_FLAG_PROFILE)
static int enqueue_staged(NdlqrHipCtx* c, const SolvePlan& plan) {
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  BufferSet& s = c->set[c->cur];
  size_t oAB, oQR, orhs, oz;
  (void)staged_doubles(u, &oAB, &oQR, &orhs, &oz);
  const size_t nAB = oQR, nQR = orhs - oQR, nz = oz - orhs;
  hipStream_t st = s.stream;
  if (c->padded) {
    double* s0 = c->pad_stage;
    HIP_TRY(hipMemcpyAsync(s0, c->h_io, sizeof(double) * (nAB + nQR + nz), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ndlqr::pad_inputs_generic, dim3(d.N, d.batch), dim3(128), 0, st, u, d, 0, (const double*)s0,
                       (const double*)(s0 + oQR), (const double*)(s0 + orhs), c->AB, c->QR, s.rhs);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(c->AB, c->h_io + oAB, sizeof(double) * nAB, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->QR, c->h_io + oQR, sizeof(double) * nQR, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.rhs, c->h_io + orhs, sizeof(double) * nz, hipMemcpyHostToDevice, st));
  }
  const int err = enqueue_solve(c, plan);
  if (err) return err;
  if (c->padded) {
    hipLaunchKernelGGL(ndlqr::unpad_blocks_generic, dim3(d.N * d.batch), dim3(64), 0, st, u, d, (const double*)s.z,
                       c->pad_stage + oz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_io + oz, c->pad_stage + oz, sizeof(double) * nz, hipMemcpyDeviceToHost, st));
  } else {
    HIP_TRY(hipMemcpyAsync(c->h_io + oz, s.z, sizeof(double) * nz, hipMemcpyDeviceToHost, st));
  }
  return NDLQR_OK;
}

int ndlqr_hip_solve_staged(NdlqrHipCtx* c) {
  if (!c || !c->h_io) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_staged")) return cerr;
  if (c->pipeline != 1) {
    const int perr = ndlqr_hip_set_pipeline_depth(c, 1);
    if (perr) return perr;
  }
  SolvePlan plan;
  int err = prepare_solve(c, &plan);  // (allocations, recovery from a failed solve; depth 1: the primary set)
  if (err) return err;
  rhs_written_cur(c, 0xFu);
  c->kept.forget_factorisation();  // new A, B, Q, R: neither a cached factor array nor cached records match
  c->forget_shifted();
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  err = (c->flags & NDLQR_FLAG_PROFILE) ? enqueue_staged(c, plan) : replay_chain(c, c->staged, plan, enqueue_staged);
  if (err) return err;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  note_solution(c);
  c->kept = plan.kept;
  c->inputs_replaced = false;
  c->timing_pending = true;
  c->state_dirty = false;
  return ndlqr_hip_synchronize(c);
}

// ------------------------------------------------------------------------------ time-axis sharding
// One problem (or a small batch) over G ranks along the horizon: launch_time_shard (launch_small.hpp) says what the
// phases do. The G - 1 top slots of every problem travel packed as [G - 1][batch][slot doubles].
static const SmallInstance* time_shard_instance(NdlqrHipCtx* c, int G) {
  if (!c || G < 2 || c->padded) return nullptr;
  const SmallInstance* inst = pick_small(c);
  if (!inst || c->d.N % G || (c->d.N / G) < 16) return nullptr;
  return inst;
}

int ndlqr_hip_time_shard_top_doubles(NdlqrHipCtx* c, int G) {
  if (c && need_unpadded_horizon(c, "ndlqr_hip_time_shard_top_doubles")) return NDLQR_ERR_INVALID;
  if (c && need_diagonal_cost(c, "ndlqr_hip_time_shard_top_doubles")) return NDLQR_ERR_INVALID;
  const SmallInstance* inst = time_shard_instance(c, G);
  return inst ? (G - 1) * c->d.batch * inst->slot : NDLQR_ERR_INVALID;
}

static int time_shard_copy_slots(NdlqrHipCtx* c, int G, double* buf, bool to_buf) {
  if (c && need_unpadded_horizon(c, to_buf ? "ndlqr_hip_time_shard_export" : "ndlqr_hip_time_shard_import")) return NDLQR_ERR_INVALID;
  if (c && need_diagonal_cost(c, to_buf ? "ndlqr_hip_time_shard_export" : "ndlqr_hip_time_shard_import")) return NDLQR_ERR_INVALID;
  const SmallInstance* inst = time_shard_instance(c, G);
  if (!inst || !buf) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& d = c->d;
  BufferSet& b = c->set[c->cur];
  const size_t slot = (size_t)inst->slot;
  const size_t pitch_red = sizeof(double) * (size_t)(d.N >> 2) * slot, width = sizeof(double) * slot;
  HIP_TRY(hipSetDevice(c->device));
  for (int j = 1; j < G; ++j) {
    const int s = j * (d.N / G) - 1;
    double* p = b.red + (size_t)(s >> 2) * slot;
    double* q = buf + (size_t)(j - 1) * d.batch * slot;
    if (to_buf) HIP_TRY(hipMemcpy2DAsync(q, width, p, pitch_red, width, (size_t)d.batch, hipMemcpyDefault, b.stream));
    else HIP_TRY(hipMemcpy2DAsync(p, pitch_red, q, width, width, (size_t)d.batch, hipMemcpyDefault, b.stream));
  }
  HIP_TRY(hipStreamSynchronize(b.stream));
  return NDLQR_OK;
}
int ndlqr_hip_time_shard_export(NdlqrHipCtx* c, int G, double* buf) { return time_shard_copy_slots(c, G, buf, true); }
int ndlqr_hip_time_shard_import(NdlqrHipCtx* c, int G, const double* buf) {
  return time_shard_copy_slots(c, G, const_cast<double*>(buf), false);
}

static int time_shard_phase(NdlqrHipCtx* c, int phase, int g, int G) {
  if (c && need_unpadded_horizon(c, phase == 0 ? "ndlqr_hip_time_shard_factor" : "ndlqr_hip_time_shard_finish")) return NDLQR_ERR_INVALID;
  if (c && need_diagonal_cost(c, phase == 0 ? "ndlqr_hip_time_shard_factor" : "ndlqr_hip_time_shard_finish")) return NDLQR_ERR_INVALID;
  if (c) c->forget_shifted();  // (the phases overwrite the records)
  const SmallInstance* inst = time_shard_instance(c, G);
  if (!inst) {
    g_last_error = "time-axis sharding: needs a size-specialised block size with a matrix-core instance, G a power of two, "
                   "N / G >= 16";
    return NDLQR_ERR_INVALID;
  }
  if (c->flags & ~NDLQR_FLAG_PROFILE) { g_last_error = "time-axis sharding runs the default fast mode only"; return NDLQR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  if (phase == 0) {
    if (c->pipeline != 1 || c->cur != 0) {
      const int perr = ndlqr_hip_set_pipeline_depth(c, 1);  // stream-ordered on the primary buffer set
      if (perr) return perr;
    }
    const int merr = rhs_make_current(c, 0xFu);
    if (merr) return merr;
    HIP_TRY(hipEventRecord(c->set[0].ev_start, c->set[0].stream));
  }
  const int err = inst->tshard(c, phase, g, G);
  if (err) {
    if (g_last_error.empty() || err == NDLQR_ERR_INVALID) g_last_error = "time-axis sharding: horizon / chunk not supported by this instance";
    return err;
  }
  HIP_TRY(hipGetLastError());
  if (phase == 1) {
    BufferSet& s = c->set[c->cur];
    HIP_TRY(hipMemcpyAsync(s.h_fail, c->info + c->d.batch, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
    c->timing_pending = true;
    note_solution(c);
    c->kept.forget_factorisation();
  }
  return NDLQR_OK;
}
int ndlqr_hip_time_shard_factor(NdlqrHipCtx* c, int g, int G) { return time_shard_phase(c, 0, g, G); }
int ndlqr_hip_time_shard_finish(NdlqrHipCtx* c, int g, int G) { return time_shard_phase(c, 1, g, G); }

// Packs the solutions of `count` problems from the blocks [count][N][2n+m] at z into dst: the whole vectors [count][nvars],
// or the slice `sel` [count][nknots][width]. u: the caller's block sizes, d: the device layout.
static hipError_t launch_pack(const ndlqr::Dims& u, const ndlqr::Dims& d, const KnotSlice& sel, const double* z, double* dst,
                              hipStream_t st, unsigned count) {
  if (sel.nknots > 0)
    hipLaunchKernelGGL(ndlqr::pack_selection_generic, dim3(sel.nknots, count), dim3(64), 0, st, u, d, sel.knot0, sel.nknots,
                       sel.blocks & 7u, z, dst);
  else
    hipLaunchKernelGGL(ndlqr::pack_solutions_generic, dim3(ndlqr::pack_solutions_chunks(u), count), dim3(256), 0, st, u, d, z,
                       dst);
  return hipGetLastError();
}

// ... into `dst`: packed in place where that is this device's memory (`own`), else packed into `stage` and copied out
static int deliver(const ndlqr::Dims& u, const ndlqr::Dims& d, const KnotSlice& sel, const double* z, double* dst, bool own,
                   double* stage, hipMemcpyKind kind, hipStream_t st, unsigned count) {
  HIP_TRY(launch_pack(u, d, sel, z, own ? dst : stage, st, count));
  if (!own) HIP_TRY(hipMemcpyAsync(dst, stage, sizeof(double) * sel.doubles(u) * count, kind, st));
  return NDLQR_OK;
}

// While in scope, the last launch of the back-substitution runs only the workgroups (eight knots each) that hold the knots
// of `sel` (launch_small.hpp: apply_grid / apply_dims; schedules without that launch compute everything); an empty slice,
// or `on` false, leaves it whole.
struct ApplySlice {
  NdlqrHipCtx* c;
  ApplySlice(NdlqrHipCtx* ctx, const KnotSlice& sel, bool on = true) : c(ctx) {
    if (!on || sel.nknots <= 0) return;
    c->apply_blk0 = sel.knot0 >> 3;
    c->apply_nblk = ((sel.knot0 + sel.nknots - 1) >> 3) - c->apply_blk0 + 1;
  }
  ~ApplySlice() { c->apply_blk0 = c->apply_nblk = 0; }
};

static bool try_launch_rhs_records(NdlqrHipCtx* c, const double* rhs, double* z);  // below

int ndlqr_hip_step_async(NdlqrHipCtx* c, const double* q, const double* r, const double* dd, const double* x0,
                         double* soln) {
  if (!c || !x0 || !soln) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_step_async")) return cerr;
  const ndlqr::Dims& d = c->d;
  SolvePlan plan;
  int err = prepare_solve(c, &plan);
  if (err) return err;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(s.ensure_xfer(c->du));  // (before anything is captured: allocation is not a stream operation)
  // the parts of the right-hand side this step does not replace: this buffer set's copy of them may be behind the other's
  const unsigned written = (q ? 1u : 0u) | (r ? 2u : 0u) | (dd ? 4u : 0u) | 8u;
  err = rhs_make_current(c, ~written & 0xFu);
  if (err) return err;
  // Everything of this step is ordered on the stream of its buffer set. Right-hand side: a streaming kernel reads
  // pinned host arrays over the host link directly; pageable ones go through the staging first (the runtime stages
  // those copies itself and blocks). Solutions: pack kernel, then ONE copy-engine transfer. With the two-deep
  // pipeline the transfers of one step run beside the kernels of the other set's step; otherwise (factor array /
  // records kept, caller-owned stream, depth 1) the steps are simply stream-ordered.
  hipStream_t st = s.stream;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  const ndlqr::Dims& u = c->du;
  const size_t nq = (size_t)u.batch * u.N * u.n, nr = (size_t)u.batch * u.N * u.m, nx = (size_t)u.batch * u.n;
  const double* src[4] = {q, r, dd, x0};
  const size_t cnt[4] = {nq, nr, nq, nx};
  const double* view[4];
  double* stage = s.xfer;
  for (int k = 0; k < 4; ++k) {
    view[k] = src[k];  // null: a part this step does not replace; this device's memory: read as it is
    const Where w = src[k] ? where(src[k], c->device) : Where::OwnDevice;
    void* dv = nullptr;
    if (w == Where::Pinned && hipHostGetDevicePointer(&dv, const_cast<double*>(src[k]), 0) == hipSuccess) {
      view[k] = static_cast<const double*>(dv);  // the kernel reads it over the host link
    } else if (w != Where::OwnDevice) {  // pageable, another device's, or pinned without a device-side view
      if (w == Where::Pinned) (void)hipGetLastError();
      HIP_TRY(hipMemcpyAsync(stage, src[k], sizeof(double) * cnt[k], hipMemcpyDefault, st));
      view[k] = stage;
    }
    stage += cnt[k];
  }
  if (u.N != d.N)  // (a padded horizon: the per-entry guards)
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<true>, dim3(512), dim3(256), 0, st, u, d, view[0], view[1], view[2],
                       view[3], s.rhs);
  else
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<false>, dim3(512), dim3(256), 0, st, u, d, view[0], view[1], view[2],
                       view[3], s.rhs);
  HIP_TRY(hipGetLastError());
  rhs_written_cur(c, written);
  // NDLQR_SOLN_ONLY: nothing but the selected knots is wanted
  const ApplySlice apply_slice(c, c->sel, (c->sel.blocks & NDLQR_SOLN_ONLY) != 0);
  // A step never changes A, B, Q, R. Under NDLQR_FLAG_KEEP_RECORDS the first step (or a solve before it) leaves the
  // compact records of the default schedule, and every further step is the right-hand-side re-solve on them (rb_forward,
  // rb_forward_top, rb_backsub: 0.46 instead of 0.59 ms per (12,4,256) x 1024) -- until new inputs are uploaded, which
  // clears rec_complete. Stream-ordered on the primary buffer set like every solve with that flag.
  // (the runtime-sized separator-only schedule likewise where its re-solve is the faster one -- beyond 32 states: 8.0
  //  against 11.5 ms at (64,16,512) x 256, 4.8 against 6.4 at (48,16,512) x 256; at (32,8) the two are equal and at
  //  (16,4,256) x 1024 the re-solve takes 2.8 ms against 1.9 for factor + solve, profiles/r04_mpc_steps.txt. The
  //  full-record form of the small shapes -- tree schedule -- re-solves no faster than it factors and keeps factoring.)
  const bool generic_records = c->kept.family == Family::GenericReduced && c->d.n > 32;
  if ((c->flags & NDLQR_FLAG_KEEP_RECORDS) && !(c->flags & (NDLQR_FLAG_STRICT_FP | NDLQR_FLAG_KEEP_FACT)) && c->kept.rec_complete &&
      (c->kept.rec_compact || generic_records) && c->cur == 0 && try_launch_rhs_records(c, s.rhs, s.z)) {
    HIP_TRY(hipGetLastError());
    note_solution(c);
    c->kept.schedule = generic_records ? "generic-reduced-records (re-solve)" : "reduced-compact-records (re-solve)";
  } else {
    err = launch_solve(c, plan);
    if (err) return err;
  }
  // (the staging has been consumed by the pack kernel: it now takes the packed solutions -- all of them, or the slice
  //  chosen with ndlqr_hip_set_step_selection)
  err = deliver(u, d, c->sel, s.z, soln, where(soln, c->device) == Where::OwnDevice, s.xfer, hipMemcpyDefault, st, d.batch);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  HIP_TRY(hipEventRecord(c->ev_step[c->step_count & 1u], st));
  c->step_set[c->step_count & 1u] = c->cur;
  ++c->step_count;
  c->timing_pending = true;
  c->state_dirty = false;
  return NDLQR_OK;
}

// Factor + solve of the resident problems, of which knots [knot0, knot0 + nknots) -- blocks `blocks` -- are computed by the
// last launch and written to `out` ([batch][nknots][width]; host, pinned or this device's memory), asynchronously: the
// solve of a loop that replaces A, B, Q, R as well (ndlqr_hip_pack_flat_device / uploads) and consumes u of knot 0.
// Consecutive calls alternate between the buffer sets like ndlqr_hip_solve_async; complete after ndlqr_hip_synchronize.
int ndlqr_hip_solve_slices_async(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks, double* out) {
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!c || !out || !sel.valid(c->du.N, 15u)) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_slices_async")) return cerr;
  const ndlqr::Dims& d = c->d;
  SolvePlan plan;
  int err = prepare_solve(c, &plan);
  if (err) return err;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(s.ensure_xfer(c->du));
  err = rhs_make_current(c, 0xFu);
  if (err) return err;
  hipStream_t st = s.stream;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  const ApplySlice apply_slice(c, sel);
  err = launch_solve(c, plan);
  if (err) return err;
  err = deliver(c->du, d, sel, s.z, out, where(out, c->device) == Where::OwnDevice, s.xfer, hipMemcpyDefault, st, d.batch);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  c->timing_pending = true;
  c->state_dirty = false;
  return NDLQR_OK;
}

// the step before the most recent one is complete (its `soln` may be read) -- whichever stream it ran on
int ndlqr_hip_synchronize_previous(NdlqrHipCtx* c) {
  if (!c) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  if (c->step_count < 2) return NDLQR_OK;
  const unsigned slot = c->step_count & 1u;  // the step before the most recent one: step_count - 2
  HIP_TRY(hipEventSynchronize(c->ev_step[slot]));
  // The failure word of that step's buffer set holds the cumulative count of non-positive pivots as of the end of its
  // solve: anything beyond what has been reported so far belongs to it (or to a step before it).
  const int* word = c->set[c->step_set[slot]].h_fail;
  if (word && *word > c->fail_base) {
    c->last_failures = *word - c->fail_base;
    c->fail_base = *word;
    return NDLQR_ERR_NOT_SPD;
  }
  return NDLQR_OK;
}

// What a step of ndlqr_hip_step_async brings down: knots [knot0, knot0 + nknots) of every problem, of each knot the
// blocks of `blocks` (NDLQR_SOLN_LAMBDA | NDLQR_SOLN_STATE | NDLQR_SOLN_INPUT), packed [batch][nknots][width].
// nknots == 0: every solution, [batch][nvars] (the default). The reference hands back the whole vector
// (src/solve.c:192-201); an MPC loop consumes u of knot 0.
int ndlqr_hip_set_step_selection(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks) {
  if (!c) return NDLQR_ERR_INVALID;
  if (nknots == 0) { c->sel = KnotSlice(); return NDLQR_OK; }
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_set_step_selection")) return cerr;
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!sel.valid(c->du.N, 15u)) return NDLQR_ERR_INVALID;
  c->sel = sel;
  return NDLQR_OK;
}

// the same slice of the most recent solve, synchronously: out = [batch][nknots][width] doubles
int ndlqr_hip_download_selection(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks, double* out) {
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!c || !out || !sel.valid(c->du.N, 7u)) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_selection")) return cerr;
  BufferSet& s = c->set[c->cur];
  if (c->z_invalid || (c->z_partial && (knot0 < 8 * c->z_blk0 || knot0 + nknots > 8 * (c->z_blk0 + c->z_nblk))))
    return need_full_solution(c, "ndlqr_hip_download_selection");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  HIP_TRY(s.ensure_xfer(c->du));
  const int derr =
      deliver(c->du, c->d, sel, c->set[c->latest].z, out, false, s.xfer, hipMemcpyDeviceToHost, s.stream, c->d.batch);
  if (derr) return derr;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

void* ndlqr_hip_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void ndlqr_hip_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
// device memory for callers without HIP headers of their own (the arrays a device-resident MPC loop hands to
// ndlqr_hip_step_async), and a synchronous copy in any direction
void* ndlqr_hip_device_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void ndlqr_hip_device_free(void* p) {
  if (p) (void)hipFree(p);
}
int ndlqr_hip_copy(void* dst, const void* src, size_t bytes) {
  if (!dst || !src) return NDLQR_ERR_INVALID;
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
  return NDLQR_OK;
}

int ndlqr_hip_upload_rhs(NdlqrHipCtx* c, int p0, int count, const double* rhs) {
  if (!c || !rhs || p0 < 0 || count <= 0 || p0 + count > c->d.batch) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  {
    const int merr = rhs_make_current(c, 0xFu);
    if (merr) return merr;
  }
  const size_t sz = (size_t)d.N * d.rows;
  if (c->padded) {
    const size_t uz = (size_t)c->du.N * c->du.rows * count;
    HIP_TRY(c->grow_pad_stage(uz));
    HIP_TRY(hipMemcpyAsync(c->pad_stage, rhs, sizeof(double) * uz, hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(ndlqr::pad_inputs_generic, dim3(d.N, count), dim3(128), 0, s.stream, c->du, d, p0,
                       (const double*)nullptr, (const double*)nullptr, (const double*)c->pad_stage, c->AB, c->QR, s.rhs);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(s.rhs + p0 * sz, rhs, sizeof(double) * sz * count, hipMemcpyHostToDevice, s.stream));
  }
  HIP_TRY(hipStreamSynchronize(s.stream));
  rhs_written_cur(c, 0xFu);
  next_solve_on_current_set(c);
  return NDLQR_OK;
}

// the factor-array sweep of a re-solve: right-hand side `rhs`, solution into `z`
template <bool STRICT>
static void launch_rhs_sweep(NdlqrHipCtx* c, const double* rhs, double* z) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  {
    ScopedSlot t(c, SLOT_LEAF);
    hipLaunchKernelGGL((ndlqr::rhs_leaf_generic<STRICT>), dim3(d.N, d.batch), dim3(64), 0, s.stream, d, c->QR,
                       rhs, z);
  }
  for (int l = 0; l < d.K; ++l) {
    {
      ScopedSlot t(c, SLOT_SEP);
      const size_t lds_staged = sizeof(double) * ((size_t)d.n * (d.n + 1) + d.n);
      const int staged = lds_staged <= kLdsMax ? 1 : 0;
      hipLaunchKernelGGL((ndlqr::rhs_separator_generic<STRICT>), dim3(d.N >> (l + 1), d.batch), dim3(64),
                         staged ? lds_staged : sizeof(double) * (size_t)d.n, s.stream, d, l, c->AB, c->F, z, staged);
    }
    {
      ScopedSlot t(c, SLOT_SCHUR);
      const int work = d.N * d.rows;
      hipLaunchKernelGGL((ndlqr::rhs_update_generic<STRICT>), dim3((work + 255) / 256, d.batch), dim3(256), 0,
                         s.stream, d, l, c->F, z);
    }
  }
}

// the record-based re-solve where the kept records have one, by the kernels of the family that wrote them: right-hand
// side `rhs`, solution into `z`
static bool try_launch_rhs_records(NdlqrHipCtx* c, const double* rhs, double* z) {
  const ndlqr::Dims& d = c->d;
  if (!c->kept.rec_complete || (c->flags & NDLQR_FLAG_STRICT_FP)) return false;
  if (c->kept.family == Family::GenericReduced) {  // records + slots + W of every separator
    launch_rhs_reduced_generic(c, rhs, z);
    return true;
  }
  const SmallInstance* inst = kept_instance(c);
  if (!inst) return false;
  // (the full-record forms: sweep array of rhs_forward_upper within the default dynamic LDS, backsub_small's K + 4
  //  separators of nx rows in one workgroup; the compact form -- rb_forward / rb_forward_top -- was checked by its plan)
  if (!c->kept.rec_compact && (d.N < 8 || (size_t)(d.N / 8) * d.n * sizeof(double) > 60 * 1024 || (d.K + 4) * inst->nx > 256))
    return false;
  inst->rhs(c, rhs, z);
  return true;
}

// the re-solve on what the last factorisation kept: the records where they have one, else the factor array; refused with
// `refusal` when there are records only and this shape / horizon has no record-based re-solve
static int launch_resolve(NdlqrHipCtx* c, const double* rhs, double* z, const char* refusal) {
  if (try_launch_rhs_records(c, rhs, z)) return NDLQR_OK;
  if (!c->kept.fact_valid) return refuse(refusal);
  if (c->flags & NDLQR_FLAG_STRICT_FP) launch_rhs_sweep<true>(c, rhs, z); else launch_rhs_sweep<false>(c, rhs, z);
  return NDLQR_OK;
}

int ndlqr_hip_solve_rhs_async(NdlqrHipCtx* c) {
  if (!c) return NDLQR_ERR_INVALID;
  if (!c->kept.fact_valid && !c->kept.rec_complete)
    return refuse("rhs-only solve needs a previous solve with NDLQR_FLAG_KEEP_FACT or "
                  "NDLQR_FLAG_KEEP_RECORDS (cached factorisation)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  c->cur = 0;  // cached records / factors live in the primary set
  BufferSet& s = c->set[0];
  {
    const int merr = rhs_make_current(c, 0xFu);
    if (merr) return merr;
  }
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  const int rerr = launch_resolve(c, s.rhs, s.z, "rhs-only solve: this configuration needs NDLQR_FLAG_KEEP_FACT");
  if (rerr) return rerr;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  c->timing_pending = true;
  note_solution(c);
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ adjoint solve, parameter gradients
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

// ------------------------------------------------------------------------------ dense cost matrices
// Layered ABOVE the plain entry points: the dense-cost problem is reduced on the device to a unit-cost problem of the same
// shape (kernels_cost.hpp), whose flat arrays -- device-resident, in the caller's layout -- go to ndlqr_hip_pack_flat_device
// and the right-hand-side pack kernel like any caller's. The solve kernels, their schedules and captured graphs never
// learn of it; solutions and adjoints are mapped back where they are packed for the caller (cost_map_back).

// S' of the flat right-hand side at q, r, d, x0 (device) into the reduced flat arrays, on `st`
static hipError_t cost_reduce_rhs(NdlqrHipCtx* c, const double* q, const double* r, const double* d, const double* x0,
                                  hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  CostState& k = c->cost;
  CostPhase phase(c, st, 1);
  const hipError_t e = launch_cost(ndlqr::cost_apply_t, ndlqr::cost_apply_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N,
                                   k.rec.get(), q, r, d, x0, nullptr, k.qt.get(), k.rt.get(), k.dt.get(), k.x0t.get(), nullptr);
  phase.stop();
  return e;
}

int ndlqr_hip_init_dense(NdlqrHipCtx* c, const double* A, const double* B, const double* Q, const double* H, const double* R,
                         const double* q, const double* r, const double* d, const double* x0) {
  if (!c || !A || !B || !Q || !R || !q || !r || !d || !x0) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& u = c->du;
  const size_t lds = sizeof(double) * ndlqr::cost_transform_lds(u.n, u.m);
  if (lds > kLdsMax)
    return refuse("ndlqr_hip_init_dense: cost_transform stages " + std::to_string(lds) + " bytes per knot at (" +
                  std::to_string(u.n) + "," + std::to_string(u.m) + "), beyond the " + std::to_string(kLdsMax) +
                  " bytes of LDS of a workgroup");
  HIP_TRY(hipSetDevice(c->device));
  const size_t kn = (size_t)u.batch * u.N, n = (size_t)u.n, m = (size_t)u.m;
  CallerArrays<9> ca = {{const_cast<double*>(A), const_cast<double*>(B), const_cast<double*>(Q), const_cast<double*>(H),
                         const_cast<double*>(R), const_cast<double*>(q), const_cast<double*>(r), const_cast<double*>(d),
                         const_cast<double*>(x0)},
                        {kn * n * n, kn * n * m, kn * n * n, kn * n * m, kn * m * m, kn * n, kn * m, kn * n, (size_t)u.batch * n}};
  int err = ca.classify(c, "ndlqr_hip_init_dense", "an input lies");
  if (err) return err;
  HIP_TRY(sync_all(c));  // solves in flight still read the inputs (and the staging)
  CostState& k = c->cost;
  const bool fresh = !k.ones;
  HIP_TRY(k.ensure(u));
  HIP_TRY(c->grad_stage.grow(ca.stage));
  ca.place(c);
  const hipStream_t st = c->set[c->cur].stream;
  err = ca.copy(st, true);
  if (err) return err;
  if (fresh) {
    hipLaunchKernelGGL(ndlqr::cost_fill, dim3(256), dim3(256), 0, st, k.ones.get(), kn * (n + m), 1.0);
    HIP_TRY(hipGetLastError());
  }
  {
    CostPhase phase(c, st, 0);
    HIP_TRY(launch_cost(ndlqr::cost_factor, ndlqr::cost_factor_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, u.batch, ca.dev[2],
                        ca.dev[3], ca.dev[4], k.rec.get(), c->info.get()));
    HIP_TRY(launch_cost(ndlqr::cost_transform, ndlqr::cost_transform_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, ca.dev[0],
                        ca.dev[1], k.rec.get(), k.At.get(), k.Bt.get()));
    phase.stop();
  }
  HIP_TRY(cost_reduce_rhs(c, ca.dev[5], ca.dev[6], ca.dev[7], ca.dev[8], st));
  // (waits for the stream first: the caller's arrays and the staging are free again when this returns)
  err = ndlqr_hip_pack_flat_device(c, k.At, k.Bt, k.ones, k.ones + kn * n, k.qt, k.rt, k.dt, k.x0t);
  if (err) return err;
  k.dense = true;
  return NDLQR_OK;
}

int ndlqr_hip_cost_is_dense(const NdlqrHipCtx* c) { return c && c->cost.dense ? 1 : 0; }
int ndlqr_hip_cost_phase_ms(NdlqrHipCtx* c, double* out3) {
  if (!c || !out3) return NDLQR_ERR_INVALID;
  for (int i = 0; i < 3; ++i) out3[i] = c->cost.phase_ms[i];
  return NDLQR_OK;
}

// ndlqr_BatchSetRhsFlat in dense-cost mode: flat q, r, d, x0 in the caller's variables (host, pinned or this device's
// memory) -> S' -> the resident right-hand side of the reduced problem
int ndlqr_hip_set_rhs_dense(NdlqrHipCtx* c, const double* q, const double* r, const double* d, const double* x0) {
  if (!c || !q || !r || !d || !x0) return NDLQR_ERR_INVALID;
  if (!c->cost.dense) return refuse("ndlqr_hip_set_rhs_dense: the solver is not in dense-cost mode");
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  const size_t kn = (size_t)u.batch * u.N;
  CallerArrays<4> ca = {{const_cast<double*>(q), const_cast<double*>(r), const_cast<double*>(d), const_cast<double*>(x0)},
                        {kn * u.n, kn * u.m, kn * u.n, (size_t)u.batch * u.n}};
  int err = ca.classify(c, "ndlqr_hip_set_rhs_dense", "an input lies");
  if (err) return err;
  HIP_TRY(sync_all(c));
  HIP_TRY(c->grad_stage.grow(ca.stage));
  ca.place(c);
  BufferSet& s = c->set[c->cur];
  err = ca.copy(s.stream, true);
  if (err) return err;
  HIP_TRY(cost_reduce_rhs(c, ca.dev[0], ca.dev[1], ca.dev[2], ca.dev[3], s.stream));
  const CostState& k = c->cost;
  if (u.N != c->d.N)
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<true>, dim3(512), dim3(256), 0, s.stream, u, c->d, (const double*)k.qt,
                       (const double*)k.rt, (const double*)k.dt, (const double*)k.x0t, s.rhs.get());
  else
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<false>, dim3(512), dim3(256), 0, s.stream, u, c->d, (const double*)k.qt,
                       (const double*)k.rt, (const double*)k.dt, (const double*)k.x0t, s.rhs.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s.stream));
  rhs_written_cur(c, 0xFu);
  next_solve_on_current_set(c);
  return NDLQR_OK;
}

// Read-out for the tests: the records and the reduced problem in the caller's flat layout, each [batch][N][..] (x0t
// [batch][n]) into HOST memory; any pointer may be null. L [n*n], LR [m*m], G [m*n] column-major.
int ndlqr_hip_download_cost_reduction(NdlqrHipCtx* c, double* L, double* LR, double* G, double* At, double* Bt, double* qt,
                                      double* rt, double* dt, double* x0t) {
  if (!c) return NDLQR_ERR_INVALID;
  if (!c->cost.dense) return refuse("ndlqr_hip_download_cost_reduction: the solver is not in dense-cost mode");
  const ndlqr::Dims& u = c->du;
  const CostState& k = c->cost;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  const size_t kn = (size_t)u.batch * u.N, n = (size_t)u.n, m = (size_t)u.m, recd = CostState::record_doubles(u);
  double* const part[3] = {L, LR, G};
  const size_t width[3] = {n * n, m * m, m * n};
  size_t off = 0;
  for (int i = 0; i < 3; off += width[i], ++i)
    if (part[i])
      HIP_TRY(hipMemcpy2D(part[i], sizeof(double) * width[i], k.rec + off, sizeof(double) * recd, sizeof(double) * width[i], kn,
                          hipMemcpyDeviceToHost));
  double* const dst[6] = {At, Bt, qt, rt, dt, x0t};
  const double* const src[6] = {k.At, k.Bt, k.qt, k.rt, k.dt, k.x0t};
  const size_t cnt[6] = {kn * n * n, kn * n * m, kn * n, kn * m, kn * n, (size_t)u.batch * n};
  for (int i = 0; i < 6; ++i)
    if (dst[i]) HIP_TRY(hipMemcpy(dst[i], src[i], sizeof(double) * cnt[i], hipMemcpyDeviceToHost));
  return NDLQR_OK;
}

// KERNEL<true> under NDLQR_FLAG_STRICT_FP, KERNEL<false> otherwise: one argument list for both
#define launch_strict(strict, KERNEL, grid, block, lds, stream, ...)                            \
  do {                                                                                          \
    if (strict) hipLaunchKernelGGL(KERNEL<true>, grid, block, lds, stream, __VA_ARGS__);        \
    else hipLaunchKernelGGL(KERNEL<false>, grid, block, lds, stream, __VA_ARGS__);              \
  } while (0)

// the device time between the events of the (synchronised) set, for ndlqr_hip_last_solve_ms
static void note_elapsed(NdlqrHipCtx* c, const BufferSet& s) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s.ev_start, s.ev_stop) == hipSuccess) c->last_ms = ms;
}

// The re-solves of the kept records write what depends on the right-hand side into them (z_sep / y~: the last n entries
// of every record) and, on the runtime-sized schedule, into the slots (gL | gR). Every re-solve recomputes those before
// it reads them; the adjoint solve still leaves them as it found them: saved before, restored after (2 n doubles per
// knot instead of the whole records).
static hipError_t adjoint_scratch(NdlqrHipCtx* c, bool restore) {
  const ndlqr::Dims& d = c->d;
  const BufferSet& s = c->set[0];
  const size_t col = sizeof(double) * d.n, rows = (size_t)d.batch * d.N;
  double* save = c->adj.save;
  double* rec_col = s.rec + 2 * (size_t)d.n * d.n;
  const size_t rec_pitch = sizeof(double) * (2 * (size_t)d.n * d.n + d.n);
  hipError_t e = restore ? hipMemcpy2DAsync(rec_col, rec_pitch, save, col, col, rows, hipMemcpyDeviceToDevice, s.stream)
                         : hipMemcpy2DAsync(save, col, rec_col, rec_pitch, col, rows, hipMemcpyDeviceToDevice, s.stream);
  if (e != hipSuccess || c->kept.family != Family::GenericReduced || d.N < 4) return e;
  double* slot_g = s.red + 4 * (size_t)d.n * d.n;
  const size_t slot_pitch = sizeof(double) * (4 * (size_t)d.n * d.n + 2 * d.n), nslots = (size_t)d.batch * (d.N / 2);
  save += rows * d.n;
  return restore ? hipMemcpy2DAsync(slot_g, slot_pitch, save, 2 * col, 2 * col, nslots, hipMemcpyDeviceToDevice, s.stream)
                 : hipMemcpy2DAsync(save, 2 * col, slot_g, slot_pitch, 2 * col, nslots, hipMemcpyDeviceToDevice, s.stream);
}

int ndlqr_hip_solve_adjoint(NdlqrHipCtx* c, const double* g) {
  if (!c || !g) return NDLQR_ERR_INVALID;
  if (!c->kept.fact_valid && !c->kept.rec_complete)
    return refuse("adjoint solve needs a previous solve with NDLQR_FLAG_KEEP_FACT or NDLQR_FLAG_KEEP_RECORDS (cached "
                  "factorisation) of the resident inputs");
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_solve_adjoint");
  if (c->kept.time_shard) return refuse("adjoint solve: not available on a time-axis shard");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  if (c->cost.dense) {  // g~ = S' g in the staging vector, which then is the adjoint's g
    const size_t count = ((size_t)u.rows * u.N - u.m) * d.batch;
    if (where(g, c->device) == Where::OtherDevice)
      return refuse("ndlqr_hip_solve_adjoint: g lies in the memory of another device than the solver's");
    HIP_TRY(sync_all(c));
    const hipStream_t st = c->set[0].stream;
    HIP_TRY(hipMemcpyAsync(c->cost.stage, g, sizeof(double) * count, hipMemcpyDefault, st));
    HIP_TRY(launch_cost(ndlqr::cost_apply_t, ndlqr::cost_apply_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, c->cost.rec.get(),
                        nullptr, nullptr, nullptr, nullptr, c->cost.stage.get(), nullptr, nullptr, nullptr, nullptr,
                        c->cost.stage.get()));
    g = c->cost.stage;
  }
  CallerArrays<1> ga = {{const_cast<double*>(g)}, {((size_t)u.rows * u.N - u.m) * d.batch}};
  int err = ga.classify(c, "ndlqr_hip_solve_adjoint", "g lies");
  if (err) return err;
  HIP_TRY(sync_all(c));
  c->cur = 0;  // cached records / factors live in the primary set
  BufferSet& s = c->set[0];
  HIP_TRY(c->adj.ensure(d, s.stream));
  HIP_TRY(c->grad_stage.grow(ga.stage));
  ga.place(c);
  err = ga.copy(s.stream, true);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  hipLaunchKernelGGL(ndlqr::adjoint_rhs_generic, dim3(d.N, d.batch), dim3(64), 0, s.stream, u, d, (const double*)ga.dev[0],
                     c->adj.rhs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(adjoint_scratch(c, false));
  err = launch_resolve(c, c->adj.rhs, c->adj.z,
                       "adjoint solve: this configuration needs NDLQR_FLAG_KEEP_FACT (like the rhs-only solve)");
  if (err) return err;
  HIP_TRY(hipGetLastError());
  HIP_TRY(adjoint_scratch(c, true));
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  note_elapsed(c, s);
  c->adj.gen = c->soln_gen;
  return NDLQR_OK;
}

// is there an adjoint of the resident solution of the resident inputs?
static int need_adjoint(const NdlqrHipCtx* c, const char* who) {
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  if (c->adj.gen == 0 || c->adj.gen != c->soln_gen)
    return refuse(std::string(who) + ": no adjoint of the resident solution (ndlqr_hip_solve_adjoint after the latest solve)");
  if (c->inputs_replaced) return refuse(std::string(who) + ": the inputs were replaced after the factorisation");
  return NDLQR_OK;
}

static int download_packed(NdlqrHipCtx* c, const double* zsrc, int p0, int count, double* soln);  // below

int ndlqr_hip_download_adjoint(NdlqrHipCtx* c, double* w) {
  if (!c || !w) return NDLQR_ERR_INVALID;
  const int aerr = need_adjoint(c, "ndlqr_hip_download_adjoint");
  if (aerr) return aerr;
  HIP_TRY(hipSetDevice(c->device));
  const Where ww = where(w, c->device);
  if (ww == Where::OtherDevice) return refuse("ndlqr_hip_download_adjoint: w lies in the memory of another device than the solver's");
  if (ww != Where::OwnDevice) return download_packed(c, c->adj.z, 0, c->d.batch, w);
  const BufferSet& s = c->set[0];
  HIP_TRY(sync_all(c));
  HIP_TRY(launch_pack(c->du, c->d, KnotSlice(), c->adj.z, w, s.stream, c->d.batch));
  if (c->cost.dense) HIP_TRY(cost_map_back(c, w, 0, c->d.batch, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

int ndlqr_hip_gradients(NdlqrHipCtx* c, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gR, double* gq,
                        double* gr, double* gd, double* gx0) {
  if (!c || (sum_mask & ~0xFFu)) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_gradients")) return cerr;
  const int aerr = need_adjoint(c, "ndlqr_hip_gradients");
  if (aerr) return aerr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<ndlqr::GRAD_COUNT> ga = {{gA, gB, gQ, gR, gq, gr, gd, gx0}, {}};
  double* const* user = ga.user;
  size_t total = 0;
  ndlqr::GradOut out = {};
  for (int o = 0; o < ndlqr::GRAD_COUNT; ++o) {
    if (!user[o]) continue;
    const bool summed = (sum_mask >> o) & 1u;
    const size_t per = o == ndlqr::GRAD_x0 ? (size_t)u.n : (size_t)u.N * ndlqr::grad_width(u, o);
    ga.cnt[o] = summed ? per : per * d.batch;
    if (summed) { out.off[o] = total; total += per; }
  }
  int err = ga.classify(c, "ndlqr_hip_gradients", "an output lies");
  if (err) return err;
  out.sum = sum_mask;
  out.total = total;
  // chunk of knots per workgroup: the accumulators of its summed outputs and its z | w blocks within 48 KB of LDS where
  // they fit (one knot of the batch-summed gA at 128 states is 128 KB)
  int wsum = 0;
  for (int o = 0; o < ndlqr::GRAD_COUNT; ++o)
    if (user[o] && ((sum_mask >> o) & 1u)) wsum += ndlqr::grad_width(u, o);
  int KC = 8;
  while (KC > 1 && (KC > d.N || sizeof(double) * ((size_t)KC * wsum + 2 * (size_t)(KC + 1) * d.rows) > 48 * 1024)) KC >>= 1;
  const size_t lds_max = kLdsMax / sizeof(double), zw = 2 * (size_t)(KC + 1) * d.rows, nacc = (size_t)KC * wsum;
  if (zw >= lds_max)
    return refuse("ndlqr_hip_gradients: z and w of two knots of this block size exceed the LDS of a workgroup");
  // where the accumulators of one knot do not fit beside z | w (a batch-summed gA from about 139 states on), they are
  // spread over nslice workgroups of EC entries each (a third grid dimension); one slice otherwise
  int nslice = (int)((nacc + (lds_max - zw) - 1) / (lds_max - zw));
  if (nslice < 1) nslice = 1;
  const size_t EC = (nacc + nslice - 1) / nslice;
  const size_t lds = sizeof(double) * (EC + zw);
  const int nchunks = d.N / KC;
  // problems per workgroup row: one without batch sums; with them, about 2048 workgroups in all (the split sums meet in
  // a second, ordered pass)
  int ppb = 1, nsplit = d.batch;
  if (total > 0) {
    nsplit = 2048 / (nchunks * nslice);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > d.batch) nsplit = d.batch;
    while (nsplit > 1 && (size_t)nsplit * total > ((size_t)64 << 20)) nsplit >>= 1;  // partial sums within 512 MB
    ppb = (d.batch + nsplit - 1) / nsplit;
    nsplit = (d.batch + ppb - 1) / ppb;
  }
  const size_t npart = nsplit > 1 ? (size_t)nsplit * total : 0;
  HIP_TRY(c->grad_stage.grow(ga.stage + npart));
  HIP_TRY(sync_all(c));
  BufferSet& s = c->set[0];
  double* part = ga.place(c);  // (the partial sums behind the staged outputs)
  if (!npart) part = nullptr;
  for (int o = 0; o < ndlqr::GRAD_COUNT; ++o) out.p[o] = ga.dev[o];
  const double* z = c->set[c->latest].z;
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  HIP_TRY(strict ? allow_dynamic_lds(&ndlqr::grad_assemble<true>, lds) : allow_dynamic_lds(&ndlqr::grad_assemble<false>, lds));
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  launch_strict(strict, ndlqr::grad_assemble, dim3(nchunks, nsplit, nslice), dim3(256), lds, s.stream, u, d, KC, ppb, (int)EC,
                z, (const double*)c->adj.z, out, part);
  HIP_TRY(hipGetLastError());
  if (part) {
    hipLaunchKernelGGL(ndlqr::grad_sum_splits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s.stream, out, nsplit,
                       (const double*)part);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  err = ga.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  note_elapsed(c, s);
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ box-constrained solve (ADMM)
// Scaled ADMM with a fixed penalty on the kept factorisation (kernels_box.hpp): QR is shifted by
// rho M in place -- the pointers, and with them the captured launch chain of the primary set, stay valid, and every record
// re-solve reads the shifted diagonal --, factored once (or not at all while the remembered shifted factorisation still
// applies), and every iteration is one re-solve into box.z plus one box_update; the host reads the running count every
// check_every iterations. The penalty is a device vector, box.rho [batch]. With adapt_every > 0
// box_update may move a problem's penalty at every adapt_every-th iteration; the host then reads the count of changed
// problems next to the running count and, when it is not zero, restores QR, shifts it by the new vector and factors the
// whole batch again -- one factorisation serves every problem that changed in that round.
// Infeasibility detection (ndlqr_hip_set_box_infeasibility, kernels_box_infeas.hpp): with a check
// period set, the iteration before a check leaves copies of z, y and rho behind its box_update, and the check iteration
// runs box_certify behind its own: a certified problem (status 4) leaves the running count like a converged one.
// Anderson acceleration (ndlqr_hip_set_box_acceleration, kernels_box_accel.hpp): with a memory
// set, box_update_accel takes the place of box_update in the loop; the iteration before an infeasibility check and the
// check iteration take plain steps.


// Bounds in the caller's layout, [P][N][n] and [P][N][m] with P = batch, or P = 1 (shared): this device's memory is read
// as it is, host memory is staged through HBM. Checked (lo <= hi for every used entry) before anything is replaced.
int ndlqr_hip_set_bounds(NdlqrHipCtx* c, int shared, const double* xlo, const double* xhi, const double* ulo,
                         const double* uhi) {
  if (!c) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_set_bounds")) return cerr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  const int P = shared ? 1 : d.batch;
  const size_t nx = (size_t)P * u.N * u.n, nu = (size_t)P * u.N * u.m;
  CallerArrays<4> in = {{const_cast<double*>(xlo), const_cast<double*>(xhi), const_cast<double*>(ulo), const_cast<double*>(uhi)},
                        {nx, nx, nu, nu}};
  int err = in.classify(c, "ndlqr_hip_set_bounds", "bounds lie");
  if (err) return err;
  BufferSet& s = c->set[0];
  HIP_TRY(c->grad_stage.grow(in.stage));
  HIP_TRY(c->box.ensure(d, s.stream));
  HIP_TRY(sync_all(c));  // (a solve in flight may still read the bounds)
  in.place(c);
  err = in.copy(s.stream, true);
  if (err) return err;
  const double* const* view = in.dev;
  HIP_TRY(hipMemsetAsync(c->box.word, 0, 4 * sizeof(int), s.stream));
  hipLaunchKernelGGL(ndlqr::box_bounds, dim3(d.N, P), dim3(64), 0, s.stream, u, d, view[0], view[1], view[2], view[3], 0,
                     c->box.lo, c->box.hi, c->box.mask, c->box.word + 2, c->box.word + 3);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->box.h_word, c->box.word, 4 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  if (c->box.h_word[2]) return refuse("ndlqr_hip_set_bounds: a lower bound exceeds its upper bound (or is NaN)");
  // the pattern lives in mask per problem: shared bounds are compared against problem 0's row of it, so a change between
  // shared and per-problem bounds always counts as a new pattern
  hipLaunchKernelGGL(ndlqr::box_bounds, dim3(d.N, P), dim3(64), 0, s.stream, u, d, view[0], view[1], view[2], view[3], 1,
                     c->box.lo, c->box.hi, c->box.mask, c->box.word + 2, c->box.word + 3);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->box.h_word, c->box.word, 4 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  if (c->box.h_word[3] || (bool)shared != c->box.shared || !c->box.have_bounds) c->box.fact = false;
  c->pol.fact = false;  // (the polish belongs to the bounds it ran with)
  c->pol.soln_gen = 0;
  c->box.soln_gen = 0;  // (a box adjoint needs the constrained solution of these bounds)
  c->box.shared = shared != 0;
  c->box.bstride = shared ? 0 : (size_t)d.N * d.w;
  c->box.have_bounds = true;
  return NDLQR_OK;
}

int ndlqr_hip_solve_box(NdlqrHipCtx* c, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                        int check_every, int warm_start, int* iters, int* status) {
  return ndlqr_hip_solve_box_ex(c, rho, alpha, eps_abs, eps_rel, max_iter, check_every, warm_start, iters, status, 0, 1e-6,
                                1e6);
}

// The shifted matrix factored on the primary set as a plain solve does it (the resident solution is overwritten), with
// the pivot check: *not_spd = NDLQR_ERR_NOT_SPD, which is returned, when a pivot was not positive.
// (who, what: the entry point and the shifted matrix, for the message)
static int box_factor(NdlqrHipCtx* c, hipStream_t st, int* not_spd, const char* who = "ndlqr_hip_solve_box",
                      const char* what = "Q + rho M, R + rho M") {
  c->forget_shifted();
  SolvePlan plan;
  int err = prepare_solve(c, &plan);  // (KEEP_*: stream-ordered on the primary set)
  if (!err) err = launch_solve(c, plan);
  if (err) return err;
  c->state_dirty = false;
  HIP_TRY(hipStreamSynchronize(st));
  // a non-positive pivot of the shifted factorisation (e.g. Q or R <= 0 on an unbounded entry): no iterations
  int seen = 0;
  for (const BufferSet& b : c->set)
    if (b.h_fail && *b.h_fail > seen) seen = *b.h_fail;
  c->last_failures = seen - c->fail_base;
  c->fail_base = seen;
  if (c->last_failures > 0) {
    refuse(std::string(who) + ": " + std::to_string(c->last_failures) + " non-positive pivot(s) in the factorisation of " + what);
    return *not_spd = NDLQR_ERR_NOT_SPD;
  }
  return NDLQR_OK;
}

// QR shifted by rho M in place, with the flags of the shifted factorisation instead of the caller's and, once the caller has
// put it there, its kept state instead of the plain API's: from open() to close(). A scope left without close() (an early
// return) restores the same. Everything is enqueued on the primary set's stream.
struct ShiftedQR {
  NdlqrHipCtx* c;
  const unsigned user_flags;
  bool open_ = false, columns_saved = false;
  explicit ShiftedQR(NdlqrHipCtx* ctx) : c(ctx), user_flags(ctx->flags) {}
  ShiftedQR(const ShiftedQR&) = delete;
  ~ShiftedQR() { (void)close(); }
  int shift(const double* rho) {
    const ndlqr::Dims& d = c->d;
    hipLaunchKernelGGL(ndlqr::box_shift_qr, dim3(d.N, d.batch), dim3(64), 0, c->set[0].stream, d, rho, (const double*)c->box.lo,
                       (const double*)c->box.hi, c->box.bstride, c->QR);
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  }
  // QR saved, c->flags = flags; the caller shifts (the polish: by sigma on its active entries)
  int open_unshifted(unsigned flags) {
    HIP_TRY(hipMemcpyAsync(c->box.qr_save, c->QR, bytes_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream));
    open_ = true;
    c->flags = flags;
    return NDLQR_OK;
  }
  // the saved QR again
  int restore() {
    HIP_TRY(hipMemcpyAsync(c->QR, c->box.qr_save, bytes_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream));
    return NDLQR_OK;
  }
  // QR saved, shifted by the penalties `rho` [batch] on the bounded entries, c->flags = flags
  int open(const double* rho, unsigned flags) {
    const int err = open_unshifted(flags);
    return err ? err : shift(rho);
  }
  // new penalties: the saved QR again, shifted by them
  int reshift(const double* rho) {
    const int err = restore();
    return err ? err : shift(rho);
  }
  // the right-hand-side columns of the kept records, which the re-solves of an adjoint overwrite: restored by close()
  int save_record_columns() {
    HIP_TRY(adjoint_scratch(c, false));
    columns_saved = true;
    return NDLQR_OK;
  }
  // Record columns and QR restored, the caller's flags back; the kept records / factors belong to the shifted matrix, so the
  // plain re-solves refuse until the next solve. The first error.
  int close() {
    if (!open_) return NDLQR_OK;
    open_ = false;
    const hipError_t ce = columns_saved ? adjoint_scratch(c, true) : hipSuccess;
    const hipError_t qe = hipMemcpyAsync(c->QR, c->box.qr_save, bytes_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream);
    c->flags = user_flags;
    c->kept.forget_factorisation();
    if (ce != hipSuccess) return fail("restoring the record columns", ce);
    return qe != hipSuccess ? fail("restoring QR", qe) : NDLQR_OK;
  }
};

// iters / status of a constrained solve or its adjoint (`who`) go to host memory or this device's
static int refuse_foreign_iters_status(const NdlqrHipCtx* c, const char* who, const int* iters, const int* status) {
  for (const int* p : {iters, status})
    if (p && where(p, c->device) == Where::OtherDevice)
      return refuse(std::string(who) + ": iters / status lie in the memory of another device than the solver's");
  return NDLQR_OK;
}

// The per-problem iteration counts and status words behind everything enqueued on st, for the caller (null: not asked
// for); a problem still running at max_iter (0) reports 2: the last iterate. Synchronises st.
static int deliver_iters_status(const NdlqrHipCtx* c, hipStream_t st, const int* d_iters, const int* d_status, int* iters,
                                int* status) {
  const size_t bytes = sizeof(int) * (size_t)c->d.batch;
  std::vector<int> h_it((size_t)c->d.batch), h_st((size_t)c->d.batch);
  HIP_TRY(hipMemcpyAsync(h_it.data(), d_iters, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_st.data(), d_status, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int& v : h_st)
    if (v == 0) v = 2;
  int* user[2] = {iters, status};
  const int* val[2] = {h_it.data(), h_st.data()};
  for (int k = 0; k < 2; ++k) {
    if (!user[k]) continue;
    if (where(user[k], c->device) == Where::OwnDevice) HIP_TRY(hipMemcpy(user[k], val[k], bytes, hipMemcpyHostToDevice));
    else memcpy(user[k], val[k], bytes);
  }
  return NDLQR_OK;
}

int ndlqr_hip_solve_box_ex(NdlqrHipCtx* c, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                           int check_every, int warm_start, int* iters, int* status, int adapt_every, double rho_min,
                           double rho_max) {
  if (!c || !(rho > 0.0) || !(alpha > 0.0 && alpha < 2.0) || !(eps_abs >= 0.0) || !(eps_rel >= 0.0) || max_iter < 1 ||
      check_every < 1 || adapt_every < 0 || (adapt_every > 0 && !(rho_min > 0.0 && rho_min <= rho_max)))
    return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_box")) return cerr;
  if (!c->box.have_bounds) return refuse("ndlqr_hip_solve_box: no bounds (ndlqr_hip_set_bounds first)");
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  int err = refuse_foreign_iters_status(c, "ndlqr_hip_solve_box", iters, status);
  if (err) return err;
  HIP_TRY(c->box.ensure(d, c->set[0].stream));
  const int infeas_every = c->infeas.every;
  if (infeas_every > 0) HIP_TRY(c->infeas.ensure(d));
  c->infeas.gen = 0;
  const int accel_mem = c->accel.mem;
  if (accel_mem > 0) HIP_TRY(c->accel.ensure(d));
  c->accel.gen = 0;
  // 1. everything idle, the primary set current with an up-to-date right-hand side
  HIP_TRY(sync_all(c));
  c->cur = 0;
  err = rhs_make_current(c, 0xFu);
  if (err) return err;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  const unsigned box_flags = c->flags | (strict ? NDLQR_FLAG_KEEP_FACT : NDLQR_FLAG_KEEP_RECORDS);
  // the remembered factorisation applies to an adaptive warm start whatever its penalties are (the settings' rho is
  // ignored: an MPC loop keeps what it learnt); everywhere else only when they are all the settings' rho
  const bool usable = c->box.fact && c->box.flags == box_flags;
  const bool keep_rho = usable && adapt_every > 0 && warm_start;
  const bool reuse = keep_rho || (usable && c->box.rho_uniform && c->box.rho_value == rho);
  bool uniform = keep_rho ? c->box.rho_uniform : true;
  const double uniform_value = keep_rho ? c->box.rho_value : rho;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  // 2. the penalties
  if (!reuse) {
    c->forget_shifted();  // (the remembered factorisation belongs to the penalties overwritten here)
    hipLaunchKernelGGL(ndlqr::box_fill_rho, dim3((d.batch + 255) / 256), dim3(256), 0, st, d.batch, rho, c->box.rho);
    HIP_TRY(hipGetLastError());
  }
  bool factored = false;  // the shifted matrix was factored in this call (the resident solution is then overwritten)
  int not_spd = NDLQR_OK;
  ShiftedQR shifted(c);
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto iterate = [&]() -> int {
    // 3. shift QR; factor the shifted matrix, unless the remembered factorisation applies
    int e = shifted.open(c->box.rho, box_flags);
    if (e) return e;
    if (reuse) {
      c->kept = c->box.kept;
    } else {
      factored = true;
      e = box_factor(c, st, &not_spd);
      if (e) return e;
    }
    // 4. the iterations
    const double* lo = c->box.lo;
    const double* hi = c->box.hi;
    const size_t bs = c->box.bstride;
    const ndlqr::BoxParams P = {alpha, 1.0 - alpha, eps_abs, eps_rel, rho_min, rho_max};
    const double* rhov = c->box.rho;
    const int cold = warm_start && c->box.have_vy ? 0 : 1;
    launch_strict(strict, ndlqr::box_start, dim3(d.N, d.batch), dim3(64), 0, st, d, rhov, cold, (const int*)c->box.status, lo,
                  hi, bs, (const double*)s.rhs, c->box.v, c->box.y, c->box.rhs[0], c->box.rhs[1]);
    HIP_TRY(hipGetLastError());
    BoxInfeasState& inf = c->infeas;
    if (infeas_every > 0) {  // (the certificate rows of the problems that do not end as 4 are zero)
      HIP_TRY(hipMemsetAsync(inf.cert_lam, 0, sizeof(double) * (size_t)d.batch * d.N * d.n, st));
      HIP_TRY(hipMemsetAsync(inf.cert_mu, 0, sizeof(double) * doubles_QR(d), st));
      HIP_TRY(hipMemsetAsync(inf.measures, 0, sizeof(double) * 4 * (size_t)d.batch, st));
      HIP_TRY(hipMemsetAsync(inf.measured_at, 0, sizeof(int) * (size_t)d.batch, st));
    }
    const auto is_check = [&](int i) { return infeas_every > 0 && i >= 2 && i <= max_iter && i % infeas_every == 0; };
    BoxAccelState& acc = c->accel;
    const ndlqr::AccelParams AP = {accel_mem, acc.safeguard, acc.reg};
    const ndlqr::AccelBufs AX = {acc.ring_t, acc.ring_g, acc.pv, acc.py, acc.gram, acc.gprev, acc.gamma, acc.meta};
    if (accel_mem > 0) {  // an empty history, warm start or cold; the ring, pv, py and gram are written before they are read
      HIP_TRY(hipMemsetAsync(acc.meta, 0, sizeof(int) * ndlqr::ACCEL_WORDS * (size_t)d.batch, st));
      HIP_TRY(hipMemsetAsync(acc.gprev, 0, sizeof(double) * (size_t)d.batch, st));
      HIP_TRY(hipMemsetAsync(acc.gamma, 0, sizeof(double) * (size_t)accel_mem * d.batch, st));
    }
    c->box.have_vy = true;
    c->box.h_word[0] = d.batch;
    c->box.h_word[1] = 0;
    HIP_TRY(hipMemcpyAsync(c->box.word, c->box.h_word, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->box.status, 0, sizeof(int) * (size_t)d.batch, st));
    for (int it = 1; it <= max_iter; ++it) {
      const double* rc = c->box.rhs[(it - 1) & 1];
      double* rn = c->box.rhs[it & 1];
      e = launch_resolve(c, rc, c->box.z, "box-constrained solve: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
      const int adapt = adapt_every > 0 && it % adapt_every == 0 && it < max_iter;
      if (accel_mem > 0)
        launch_strict(strict, ndlqr::box_update_accel, dim3(d.batch), dim3(256), 0, st, d, it, adapt,
                      is_check(it) || is_check(it + 1) ? 1 : 0, P, AP, (const double*)c->box.z, lo, hi, bs, c->box.v, c->box.y,
                      (const double*)s.rhs, rc, rn, c->box.rho, c->box.status, c->box.iters, c->box.resid, c->box.word, AX);
      else
        launch_strict(strict, ndlqr::box_update, dim3(d.batch), dim3(256), 0, st, d, it, adapt, P, (const double*)c->box.z, lo, hi,
                      bs, c->box.v, c->box.y, (const double*)s.rhs, rc, rn, c->box.rho, c->box.status, c->box.iters,
                      c->box.resid, c->box.word);
      HIP_TRY(hipGetLastError());
      if (is_check(it)) {  // the differences over this iteration: a certificate?
        hipLaunchKernelGGL(ndlqr::box_certify, dim3(d.batch), dim3(256), ndlqr::certify_lds_bytes(d), st, d, it, inf.eps,
                           (const double*)c->AB, (const double*)c->box.z, (const double*)inf.z_prev, (const double*)c->box.y,
                           (const double*)inf.y_prev, (const double*)c->box.rho, (const double*)inf.rho_prev, lo, hi, bs,
                           (const double*)s.rhs, c->box.rhs[(it - 1) & 1], (const double*)rn, c->box.status, c->box.iters,
                           c->box.word, inf.cert_lam, inf.cert_mu, inf.measures, inf.measured_at);
        HIP_TRY(hipGetLastError());
      }
      if (is_check(it + 1)) {  // what the next iteration's check takes its differences against
        HIP_TRY(hipMemcpyAsync(inf.z_prev, c->box.z, sizeof(double) * doubles_z(d), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(inf.y_prev, c->box.y, sizeof(double) * doubles_QR(d), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(inf.rho_prev, c->box.rho, sizeof(double) * (size_t)d.batch, hipMemcpyDeviceToDevice, st));
      }
      if (it % check_every == 0 || it == max_iter || adapt) {
        // 5. one word: how many problems still run; after an adapting update also how many changed their penalty
        HIP_TRY(hipMemcpyAsync(c->box.h_word, c->box.word, (adapt ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (c->box.h_word[0] == 0) break;
        if (adapt && c->box.h_word[1] != 0) {
          // 5a. new penalties: the saved QR shifted by the new vector and factored as above (frozen problems keep their
          // penalty: the same factors again, so their later re-solves reproduce their z)
          uniform = false;
          factored = true;
          e = shifted.reshift(rhov);
          if (!e) e = box_factor(c, st, &not_spd);
          if (e) return e;
          HIP_TRY(hipMemsetAsync(c->box.word + 1, 0, sizeof(int), st));
        }
      }
    }
    // 6. deliver
    hipLaunchKernelGGL(ndlqr::box_finish, dim3(d.N, d.batch), dim3(64), 0, st, d, lo, hi, bs, (const double*)c->box.z, c->box.v,
                       s.z);
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = iterate();
  // 7. restore QR, bookkeeping
  const KeptState shifted_kept = c->kept;  // (close() forgets it for the plain API)
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (!err) {
    c->box.fact = true;
    c->box.rho_uniform = uniform;
    c->box.rho_value = uniform_value;
    c->box.flags = box_flags;
    c->box.kept = shifted_kept;
  } else {
    c->forget_shifted();
    c->box.have_vy = false;
    if (!not_spd) c->state_dirty = true;  // (a failed launch; a non-positive pivot leaves the device state clean)
    if (factored) c->z_invalid = true;    // (the factorisation solved the shifted matrix with the unshifted right-hand side)
    (void)hipStreamSynchronize(st);
    return err;
  }
  note_solution(c);
  c->box.soln_gen = c->soln_gen;
  if (infeas_every > 0) c->infeas.gen = c->soln_gen;
  if (accel_mem > 0) {
    c->accel.gen = c->soln_gen;
    c->accel.mem_solved = accel_mem;
  }
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  c->timing_pending = true;
  err = deliver_iters_status(c, st, c->box.iters, c->box.status, iters, status);
  if (err) return err;
  return ndlqr_hip_synchronize(c);
}

int ndlqr_hip_set_box_infeasibility(NdlqrHipCtx* c, int every, double eps) {
  if (!c || every < 0 || !(eps > 0.0 && eps < HUGE_VAL)) return NDLQR_ERR_INVALID;
  if (every > 0) {  // (switching it off is always possible)
    if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_set_box_infeasibility")) return herr;
    if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_set_box_infeasibility")) return cerr;
  }
  c->infeas.every = every;
  c->infeas.eps = eps;
  return NDLQR_OK;
}

int ndlqr_hip_download_infeasibility_certificate(NdlqrHipCtx* c, double* dlam, double* dmu_x, double* dmu_u) {
  if (!c || (!dlam && !dmu_x && !dmu_u)) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_infeasibility_certificate")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_infeasibility_certificate")) return cerr;
  if (c->infeas.gen == 0 || c->infeas.gen != c->soln_gen || c->box.soln_gen != c->soln_gen)
    return refuse("ndlqr_hip_download_infeasibility_certificate: the resident solution is not that of a constrained solve "
                  "with infeasibility detection on (ndlqr_hip_set_box_infeasibility before the solve)");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nx = (size_t)u.batch * u.N * u.n;
  CallerArrays<3> out = {{dlam, dmu_x, dmu_u}, {nx, nx, (size_t)u.batch * u.N * u.m}};
  int err = out.classify(c, "ndlqr_hip_download_infeasibility_certificate", "an output lies");
  if (err) return err;
  HIP_TRY(c->grad_stage.grow(out.stage));
  HIP_TRY(sync_all(c));
  const BufferSet& s = c->set[0];
  out.place(c);
  hipLaunchKernelGGL(ndlqr::box_certificate_out, dim3(d.N, d.batch), dim3(64), 0, s.stream, u, d, (const double*)c->infeas.cert_lam,
                     (const double*)c->infeas.cert_mu, out.dev[0], out.dev[1], out.dev[2]);
  HIP_TRY(hipGetLastError());
  err = out.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

int ndlqr_hip_download_infeasibility_measures(NdlqrHipCtx* c, double* measures, int* iteration) {
  if (!c || (!measures && !iteration)) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_infeasibility_measures")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_infeasibility_measures")) return cerr;
  if (c->infeas.gen == 0 || c->infeas.gen != c->soln_gen || c->box.soln_gen != c->soln_gen)
    return refuse("ndlqr_hip_download_infeasibility_measures: the resident solution is not that of a constrained solve "
                  "with infeasibility detection on (ndlqr_hip_set_box_infeasibility before the solve)");
  HIP_TRY(hipSetDevice(c->device));
  for (const void* p : {(const void*)measures, (const void*)iteration})
    if (p && where(p, c->device) == Where::OtherDevice)
      return refuse("ndlqr_hip_download_infeasibility_measures: an output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  // (stored in the caller's layout: plain copies, as ndlqr_hip_download_box_penalties)
  const size_t nb = (size_t)c->d.batch;
  if (measures) HIP_TRY(hipMemcpy(measures, c->infeas.measures, sizeof(double) * 4 * nb, hipMemcpyDefault));
  if (iteration) HIP_TRY(hipMemcpy(iteration, c->infeas.measured_at, sizeof(int) * nb, hipMemcpyDefault));
  return NDLQR_OK;
}

int ndlqr_hip_set_box_acceleration(NdlqrHipCtx* c, int mem, double safeguard, double reg) {
  if (!c || mem < 0 || mem > ndlqr::ACCEL_MEM_MAX || !(safeguard > 0.0 && safeguard < HUGE_VAL) || !(reg > 0.0 && reg < HUGE_VAL))
    return NDLQR_ERR_INVALID;
  if (mem > 0) {  // (switching it off is always possible)
    if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_set_box_acceleration")) return herr;
    if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_set_box_acceleration")) return cerr;
  }
  c->accel.mem = mem;
  c->accel.gen = 0;  // (the read-out's gamma has the width of the memory it ran with: a solve with this setting first)
  c->accel.safeguard = safeguard;
  c->accel.reg = reg;
  return NDLQR_OK;
}

int ndlqr_hip_download_box_acceleration(NdlqrHipCtx* c, int* accepted, int* rejected, double* gamma, int* columns) {
  if (!c || (!accepted && !rejected && !gamma && !columns)) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_box_acceleration")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_box_acceleration")) return cerr;
  if (c->accel.gen == 0 || c->accel.gen != c->soln_gen || c->box.soln_gen != c->soln_gen)
    return refuse("ndlqr_hip_download_box_acceleration: the resident solution is not that of a constrained solve with "
                  "acceleration on (ndlqr_hip_set_box_acceleration before the solve)");
  HIP_TRY(hipSetDevice(c->device));
  for (const void* p : {(const void*)accepted, (const void*)rejected, (const void*)gamma, (const void*)columns})
    if (p && where(p, c->device) == Where::OtherDevice)
      return refuse("ndlqr_hip_download_box_acceleration: an output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  // (stored in the caller's layout: plain copies, as ndlqr_hip_download_box_penalties)
  const size_t nb = (size_t)c->d.batch;
  const int* meta = c->accel.meta;
  if (accepted) HIP_TRY(hipMemcpy(accepted, meta + ndlqr::ACCEL_ACCEPTED * nb, sizeof(int) * nb, hipMemcpyDefault));
  if (rejected) HIP_TRY(hipMemcpy(rejected, meta + ndlqr::ACCEL_REJECTED * nb, sizeof(int) * nb, hipMemcpyDefault));
  if (columns) HIP_TRY(hipMemcpy(columns, meta + ndlqr::ACCEL_COLUMNS * nb, sizeof(int) * nb, hipMemcpyDefault));
  if (gamma) HIP_TRY(hipMemcpy(gamma, c->accel.gamma, sizeof(double) * nb * c->accel.mem_solved, hipMemcpyDefault));
  return NDLQR_OK;
}

int ndlqr_hip_download_box_penalties(NdlqrHipCtx* c, double* rho) {
  if (!c || !rho) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_box_penalties")) return cerr;
  if (!c->box.have_vy || !c->box.rho) return refuse("ndlqr_hip_download_box_penalties: no constrained solve yet");
  HIP_TRY(hipSetDevice(c->device));
  if (where(rho, c->device) == Where::OtherDevice)
    return refuse("ndlqr_hip_download_box_penalties: the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(rho, c->box.rho, sizeof(double) * (size_t)c->d.batch, hipMemcpyDefault));
  return NDLQR_OK;
}

// resid [batch][4] of a constrained solve or its adjoint (`who`), stored in the caller's layout: a plain copy
static int download_resid(NdlqrHipCtx* c, const char* who, const double* d_resid, double* resid) {
  HIP_TRY(hipSetDevice(c->device));
  if (where(resid, c->device) == Where::OtherDevice)
    return refuse(std::string(who) + ": the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(resid, d_resid, sizeof(double) * 4 * (size_t)c->d.batch, hipMemcpyDefault));
  return NDLQR_OK;
}

int ndlqr_hip_download_box_residuals(NdlqrHipCtx* c, double* resid) {
  if (!c || !resid) return NDLQR_ERR_INVALID;
  if (c->box.soln_gen == 0 || c->box.soln_gen != c->soln_gen || !c->box.resid)
    return refuse("ndlqr_hip_download_box_residuals: the resident solution is not that of a constrained solve");
  return download_resid(c, "ndlqr_hip_download_box_residuals", c->box.resid, resid);
}

int ndlqr_hip_download_box_adjoint_residuals(NdlqrHipCtx* c, double* resid) {
  if (!c || !resid) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_box_adjoint_residuals")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_box_adjoint_residuals")) return cerr;
  if (c->abox.gen == 0 || c->abox.gen != c->soln_gen || !c->abox.resid)
    return refuse("ndlqr_hip_download_box_adjoint_residuals: no box adjoint of the resident solution "
                  "(ndlqr_hip_solve_box_adjoint after the latest constrained solve)");
  return download_resid(c, "ndlqr_hip_download_box_adjoint_residuals", c->abox.resid, resid);
}

int ndlqr_hip_download_bound_multipliers(NdlqrHipCtx* c, double* mu_x, double* mu_u) {
  if (!c || (!mu_x && !mu_u)) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_bound_multipliers")) return cerr;
  if (!c->box.have_vy || !c->box.y) return refuse("ndlqr_hip_download_bound_multipliers: no constrained solve yet");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<2> out = {{mu_x, mu_u}, {(size_t)u.batch * u.N * u.n, (size_t)u.batch * u.N * u.m}};
  int err = out.classify(c, "ndlqr_hip_download_bound_multipliers", "an output lies");
  if (err) return err;
  HIP_TRY(c->grad_stage.grow(out.stage));
  HIP_TRY(sync_all(c));
  const BufferSet& s = c->set[0];
  out.place(c);
  if (c->pol.soln_gen != 0 && c->pol.soln_gen == c->soln_gen)  // (a polished solution: its mu where the polish succeeded)
    hipLaunchKernelGGL(ndlqr::polish_multipliers, dim3(d.N, d.batch), dim3(64), 0, s.stream, u, d, (const double*)c->box.rho,
                       (const double*)c->box.y, (const int*)c->pol.state, (const double*)c->pol.mu, out.dev[0], out.dev[1]);
  else
    hipLaunchKernelGGL(ndlqr::box_multipliers, dim3(u.N, d.batch), dim3(64), 0, s.stream, u, d, (const double*)c->box.rho,
                       (const double*)c->box.y, out.dev[0], out.dev[1]);
  HIP_TRY(hipGetLastError());
  err = out.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ gradients through the box-constrained solve
// The adjoint of the active-set system (kernels_box_grad.hpp) by the ADMM of the forward on its
// remembered shifted factorisation: QR shifted by the forward's rho on its bounded entries again (restored on every
// exit), the kept records / factors taken as the forward left them -- nothing is factored --, every iteration one
// re-solve into adj.z plus one box_adjoint_update. The right-hand-side columns of the kept records and slots are saved and
// restored around it as for the plain adjoint, so the next warm-started forward finds everything as it was.

int ndlqr_hip_solve_box_adjoint(NdlqrHipCtx* c, const double* g, double alpha, double eps_abs, double eps_rel, int max_iter,
                                int check_every, int* iters, int* status) {
  if (!c || !g || !(alpha > 0.0 && alpha < 2.0) || !(eps_abs >= 0.0) || !(eps_rel >= 0.0) || max_iter < 1 ||
      check_every < 1)
    return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_solve_box_adjoint")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_box_adjoint")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_solve_box_adjoint");
  if (c->pol.soln_gen != 0 && c->pol.soln_gen == c->soln_gen)
    return refuse("ndlqr_hip_solve_box_adjoint: the resident solution was polished (ndlqr_hip_polish_box), which replaced the "
                  "ADMM factorisation: its adjoint is the polished adjoint (ndlqr_hip_solve_polished_adjoint)");
  if (c->box.soln_gen == 0 || c->box.soln_gen != c->soln_gen || !c->box.fact || c->inputs_replaced)
    return refuse("ndlqr_hip_solve_box_adjoint: the resident solution is not that of the latest constrained solve (a solve, "
                  "step, re-solve, new inputs or new bounds came after it)");
  if (c->box.kept.time_shard) return refuse("ndlqr_hip_solve_box_adjoint: not available on a time-axis shard");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<1> ga = {{const_cast<double*>(g)}, {((size_t)u.rows * u.N - u.m) * d.batch}};
  int err = ga.classify(c, "ndlqr_hip_solve_box_adjoint", "g lies");
  if (!err) err = refuse_foreign_iters_status(c, "ndlqr_hip_solve_box_adjoint", iters, status);
  if (err) return err;
  HIP_TRY(c->adj.ensure(d, c->set[0].stream));
  HIP_TRY(c->abox.ensure(d));
  HIP_TRY(c->grad_stage.grow(ga.stage));
  // 1. everything idle, the primary set current; g packed into the adjoint's resident right-hand side
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  ga.place(c);
  err = ga.copy(st, true);
  if (err) return err;
  c->abox.gen = 0;
  c->adj.gen = 0;
  const bool strict = (c->box.flags & NDLQR_FLAG_STRICT_FP) != 0;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  ShiftedQR shifted(c);
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto iterate = [&]() -> int {
    const double* rho = c->box.rho;  // (the forward's final penalties: those of the remembered factorisation)
    hipLaunchKernelGGL(ndlqr::adjoint_rhs_generic, dim3(d.N, d.batch), dim3(64), 0, st, u, d, (const double*)ga.dev[0],
                       c->adj.rhs);
    HIP_TRY(hipGetLastError());
    // 2. shift QR, take up the remembered shifted factorisation, save the right-hand-side columns of the records
    int e = shifted.open(rho, c->box.flags);
    if (e) return e;
    c->kept = c->box.kept;
    e = shifted.save_record_columns();
    if (e) return e;
    // 3. codes, v = y = 0, right-hand sides, status
    const ndlqr::BoxParams P = {alpha, 1.0 - alpha, eps_abs, eps_rel, 0.0, 0.0};
    HIP_TRY(hipMemsetAsync(c->abox.word, 0, sizeof(int), st));
    // (the read-out row of a problem that is not iterated -- forward status 3 or 4 -- is zero)
    HIP_TRY(hipMemsetAsync(c->abox.resid, 0, sizeof(double) * 4 * (size_t)d.batch, st));
    launch_strict(strict, ndlqr::box_adjoint_start, dim3(d.N, d.batch), dim3(64), 0, st, d, rho, (const double*)c->box.lo,
                  (const double*)c->box.hi, c->box.bstride, (const double*)c->box.v, (const int*)c->box.status,
                  (const double*)c->adj.rhs, c->abox.code, c->abox.v, c->abox.y, c->abox.rhs[0], c->abox.rhs[1], c->abox.status,
                  c->abox.iters, c->abox.word);
    HIP_TRY(hipGetLastError());
    // 4. the iterations (none when every problem's forward ended non-finite)
    HIP_TRY(hipMemcpyAsync(&c->box.h_word[4], c->abox.word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const bool any = c->box.h_word[4] > 0;
    for (int it = 1; it <= max_iter && any; ++it) {
      const double* rc = c->abox.rhs[(it - 1) & 1];
      double* rn = c->abox.rhs[it & 1];
      e = launch_resolve(c, rc, c->adj.z, "box adjoint: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
      launch_strict(strict, ndlqr::box_adjoint_update, dim3(d.batch), dim3(256), 0, st, d, it, P, (const double*)c->adj.z,
                    (const unsigned char*)c->abox.code, c->abox.v, c->abox.y, (const double*)c->adj.rhs, rc, rn, rho,
                    c->abox.status, c->abox.iters, c->abox.resid, c->abox.word);
      HIP_TRY(hipGetLastError());
      if (it % check_every == 0 || it == max_iter) {
        HIP_TRY(hipMemcpyAsync(&c->box.h_word[4], c->abox.word, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (c->box.h_word[4] == 0) break;
      }
    }
    if (!any) {  // (no re-solve ran: a defined w all the same -- the re-solve of the packed g)
      e = launch_resolve(c, c->abox.rhs[0], c->adj.z, "box adjoint: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
      HIP_TRY(hipGetLastError());
    }
    // 5. w = [lambda, v]
    hipLaunchKernelGGL(ndlqr::box_adjoint_finish, dim3(d.N, d.batch), dim3(64), 0, st, d, (const unsigned char*)c->abox.code,
                       (const double*)c->abox.v, (const int*)c->abox.status, c->adj.z);
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = iterate();
  // 6. restore the record columns and QR, bookkeeping (the kept state as the constrained solve left it)
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (err) {
    c->state_dirty = true;
    (void)hipStreamSynchronize(st);
    return err;
  }
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = deliver_iters_status(c, st, c->abox.iters, c->abox.status, iters, status);
  if (err) return err;
  note_elapsed(c, s);
  c->adj.gen = c->soln_gen;
  c->abox.gen = c->soln_gen;
  return NDLQR_OK;
}

int ndlqr_hip_bound_gradients(NdlqrHipCtx* c, int summed, double* gxlo, double* gxhi, double* gulo, double* guhi) {
  if (!c) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_bound_gradients")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_bound_gradients")) return cerr;
  const int aerr = need_adjoint(c, "ndlqr_hip_bound_gradients");
  if (aerr) return aerr;
  const bool polished = c->pol.adj_gen != 0 && c->pol.adj_gen == c->soln_gen;  // (nu split by the polish codes, penalty 1)
  if (c->abox.gen != c->soln_gen && !polished)
    return refuse("ndlqr_hip_bound_gradients: no box adjoint of the resident solution (ndlqr_hip_solve_box_adjoint after the "
                  "latest constrained solve, or ndlqr_hip_solve_polished_adjoint after the latest polish)");
  const double* g_rho = polished ? c->pol.ones : c->box.rho;
  const unsigned char* g_code = polished ? c->pol.code : c->abox.code;
  const double* g_y = polished ? c->pol.nu : c->abox.y;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  const size_t P = summed ? 1 : (size_t)d.batch;
  CallerArrays<4> go = {{gxlo, gxhi, gulo, guhi}, {P * u.N * u.n, P * u.N * u.n, P * u.N * u.m, P * u.N * u.m}};
  int err = go.classify(c, "ndlqr_hip_bound_gradients", "an output lies");
  if (err) return err;
  if (!gxlo && !gxhi && !gulo && !guhi) return NDLQR_OK;
  // batch sums: entries of [N][n+m] one per thread, the batch split into about 2048 / ceil(entries / 256) runs of problems
  // added in order, then the runs in order (grad_assemble's scheme: deterministic, no atomics)
  const size_t E = (size_t)u.N * (u.n + u.m);
  const unsigned nblk = (unsigned)((E + 255) / 256);
  int nsplit = 1, ppb = d.batch;
  if (summed) {
    nsplit = (int)(2048 / nblk);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > d.batch) nsplit = d.batch;
    ppb = (d.batch + nsplit - 1) / nsplit;
    nsplit = (d.batch + ppb - 1) / ppb;
  }
  const size_t npart = nsplit > 1 ? (size_t)nsplit * 2 * E : 0;
  HIP_TRY(c->grad_stage.grow(go.stage + npart));
  HIP_TRY(sync_all(c));
  BufferSet& s = c->set[0];
  ndlqr::BoundOut out = {};
  double* part = go.place(c);  // (the partial sums behind the staged outputs)
  if (!npart) part = nullptr;
  for (int k = 0; k < 4; ++k) out.p[k] = go.dev[k];
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  if (!summed) {
    hipLaunchKernelGGL(ndlqr::box_bound_grads, dim3(d.N, d.batch), dim3(64), 0, s.stream, u, d, g_rho, g_code, g_y, out);
    HIP_TRY(hipGetLastError());
  } else {
    hipLaunchKernelGGL(ndlqr::box_bound_grads_sum, dim3(nblk, nsplit), dim3(256), 0, s.stream, u, d,
                       g_rho, ppb, g_code, g_y, out, part);
    HIP_TRY(hipGetLastError());
    if (part) {
      hipLaunchKernelGGL(ndlqr::box_bound_sum_splits, dim3(nblk), dim3(256), 0, s.stream, u, nsplit, (const double*)part, out);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  err = go.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  note_elapsed(c, s);
  return NDLQR_OK;
}

unsigned long long ndlqr_hip_factor_count(const NdlqrHipCtx* c) { return c ? c->factor_count : 0; }

// ------------------------------------------------------------------------------ iterative refinement
// ndlqr_hip_refine (kernels_refine.hpp): the residual of the resident solution (which == 0) or of the
// latest plain adjoint (which == 1) in double-double, then max_steps times: the re-solve of that residual against the kept
// factorisation into delta (record columns / slots saved and restored around it, as for the adjoint solve), the residual of
// z (+) delta over the old one, and the commit for the problems whose residual norm went down at every step so far. The
// host reads nothing back between the steps: acceptance is decided on the device from the norm slots.

// r = b - K (z (+) delta) into c->ref.r on the current set's stream (norms == nullptr: the vector alone)
// (QR: the diagonal to use -- the polish passes the saved, unshifted one --, r: the destination)
static int launch_residual_dd_on(NdlqrHipCtx* c, const double* QR, const double* rhs, const double* z, const double* delta,
                                 double* r, unsigned long long* norms, int nslots, int slot) {
  const ndlqr::Dims& d = c->d;
  const bool staged = ndlqr::refine_lds_bytes(d, true) + 64 <= kLdsMax;  // (+ the kernel's static words)
  const size_t lds = ndlqr::refine_lds_bytes(d, staged);
  if (lds + 64 > kLdsMax) return refuse("double-double residual: two knots of this block size exceed the LDS of a workgroup");
  HIP_TRY(allow_dynamic_lds(&ndlqr::kkt_residual_dd, lds));
  const int threads = d.rows + d.n <= 64 ? 64 : (d.rows + d.n <= 128 ? 128 : 256);
  hipLaunchKernelGGL(ndlqr::kkt_residual_dd, dim3(d.N, d.batch), dim3(threads), lds, c->set[c->cur].stream, c->du, d,
                     (const double*)c->AB, QR, rhs, z, delta, r, norms, nslots, slot, staged ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return NDLQR_OK;
}

// r = b - K (z (+) delta) into c->ref.r on the resident QR
static int launch_residual_dd(NdlqrHipCtx* c, const double* rhs, const double* z, const double* delta,
                              unsigned long long* norms, int nslots, int slot) {
  return launch_residual_dd_on(c, c->QR, rhs, z, delta, c->ref.r, norms, nslots, slot);
}

// per-phase device times of a refinement under NDLQR_FLAG_PROFILE (ndlqr_hip_refine_phase_ms)
struct RefinePhases {
  NdlqrHipCtx* c;
  bool on;
  struct Span { int phase; hipEvent_t start, stop; };
  std::vector<Span> spans;
  explicit RefinePhases(NdlqrHipCtx* ctx) : c(ctx), on((ctx->flags & NDLQR_FLAG_PROFILE) != 0) {}
  void open(int phase) {
    if (!on) return;
    spans.push_back({phase, take_event(c), take_event(c)});
    (void)hipEventRecord(spans.back().start, c->set[0].stream);
  }
  void close() {
    if (on) (void)hipEventRecord(spans.back().stop, c->set[0].stream);
  }
  // (the stream has been synchronised)
  void collect() {
    for (int p = 0; p < 3; ++p) c->ref.phase_ms[p] = 0.0;
    for (const Span& sp : spans) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, sp.start, sp.stop) == hipSuccess) c->ref.phase_ms[sp.phase] += ms;
      c->event_pool.push_back(sp.start);
      c->event_pool.push_back(sp.stop);
    }
    spans.clear();
  }
};

int ndlqr_hip_refine(NdlqrHipCtx* c, int which, int max_steps, int* steps, double* eta_before, double* eta_after) {
  if (!c || which < 0 || which > 1 || max_steps < 1 || max_steps > kRefineMaxSteps) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_refine")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_refine")) return cerr;
  const char* who = which ? "ndlqr_hip_refine (adjoint)" : "ndlqr_hip_refine";
  if (!c->kept.fact_valid && !c->kept.rec_complete)
    return refuse(std::string(who) + ": needs a previous solve with NDLQR_FLAG_KEEP_FACT or NDLQR_FLAG_KEEP_RECORDS (cached "
                  "factorisation) of the resident inputs");
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  if (c->kept.time_shard) return refuse(std::string(who) + ": not available on a time-axis shard");
  if (c->inputs_replaced) return refuse(std::string(who) + ": the inputs were replaced after the factorisation");
  if (c->latest != 0) return refuse(std::string(who) + ": the resident solution is not on the primary buffer set");
  if (which) {
    const int aerr = need_adjoint(c, who);
    if (aerr) return aerr;
    if (c->abox.gen == c->soln_gen || c->pol.adj_gen == c->soln_gen)
      return refuse(std::string(who) + ": the adjoint is that of a constrained solve");
  }
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<2> ea = {{eta_before, eta_after}, {(size_t)d.batch, (size_t)d.batch}};
  int err = ea.classify(c, who, "an output lies");
  if (!err) err = refuse_foreign_iters_status(c, who, steps, nullptr);
  if (err) return err;
  // 1. everything idle, the primary set current with an up-to-date right-hand side
  HIP_TRY(sync_all(c));
  c->cur = 0;
  err = rhs_make_current(c, 0xFu);
  if (err) return err;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  const int nslots = max_steps + 1;
  const size_t norm_bytes = sizeof(unsigned long long) * RefineState::norm_count(d);
  HIP_TRY(c->ref.ensure(d, st));
  HIP_TRY(c->adj.ensure_save(d));
  const double* rhs = which ? c->adj.rhs : s.rhs;
  double* z = which ? c->adj.z : s.z;
  RefinePhases phases(c);
  HIP_TRY(hipEventRecord(s.ev_start, st));
  HIP_TRY(hipMemsetAsync(c->ref.norms, 0, norm_bytes, st));
  // 2. the residual of z as found
  phases.open(0);
  err = launch_residual_dd(c, rhs, z, nullptr, c->ref.norms, nslots, 0);
  phases.close();
  if (err) return err;
  // 3. the steps
  for (int step = 1; step <= max_steps; ++step) {
    phases.open(1);
    HIP_TRY(adjoint_scratch(c, false));
    err = launch_resolve(c, c->ref.r, c->ref.delta,
                         "refinement: this configuration needs NDLQR_FLAG_KEEP_FACT (like the rhs-only solve)");
    if (err) return err;
    HIP_TRY(hipGetLastError());
    HIP_TRY(adjoint_scratch(c, true));
    phases.close();
    phases.open(0);
    err = launch_residual_dd(c, rhs, z, c->ref.delta, c->ref.norms, nslots, step);
    phases.close();
    if (err) return err;
    phases.open(2);
    hipLaunchKernelGGL(ndlqr::refine_commit, dim3((unsigned)((d.N * d.rows + 255) / 256), d.batch), dim3(256), 0, st, d,
                       (const unsigned long long*)c->ref.norms, step, (const double*)c->ref.delta, z);
    phases.close();
    HIP_TRY(hipGetLastError());
  }
  // 4. what the caller asked for
  hipLaunchKernelGGL(ndlqr::refine_report, dim3((d.batch + 255) / 256), dim3(256), 0, st, d.batch, max_steps,
                     (const unsigned long long*)c->ref.norms, c->ref.steps, c->ref.eta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  if (!which) note_solution(c);  // (a refined primal is a new resident solution: an earlier adjoint no longer applies)
  for (int k = 0; k < 2; ++k)
    if (ea.user[k]) {
      if (ea.own[k]) HIP_TRY(hipMemcpyAsync(ea.user[k], c->ref.eta + (size_t)k * d.batch, sizeof(double) * d.batch, hipMemcpyDeviceToDevice, st));
      else HIP_TRY(hipMemcpyAsync(ea.user[k], c->ref.eta + (size_t)k * d.batch, sizeof(double) * d.batch, hipMemcpyDeviceToHost, st));
    }
  if (steps) {
    const bool own = where(steps, c->device) == Where::OwnDevice;
    HIP_TRY(hipMemcpyAsync(steps, c->ref.steps, sizeof(int) * (size_t)d.batch, own ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  note_elapsed(c, s);
  phases.collect();
  return NDLQR_OK;
}

int ndlqr_hip_refine_phase_ms(NdlqrHipCtx* c, double* out3) {
  if (!c || !out3) return NDLQR_ERR_INVALID;
  for (int p = 0; p < 3; ++p) out3[p] = c->ref.phase_ms[p];
  return NDLQR_OK;
}

int ndlqr_hip_kkt_residual_vector(NdlqrHipCtx* c, double* r) {
  if (!c || !r) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_kkt_residual_vector")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_kkt_residual_vector");
  HIP_TRY(hipSetDevice(c->device));
  const Where wr = where(r, c->device);
  if (wr == Where::OtherDevice)
    return refuse("ndlqr_hip_kkt_residual_vector: r lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(c->ref.ensure_r(c->d));
  int err;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  err = launch_residual_dd(c, s.rhs, c->set[c->latest].z, nullptr, nullptr, 0, 0);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, s.stream));
  if (wr != Where::OwnDevice) {
    err = download_packed(c, c->ref.r, 0, c->d.batch, r);
    if (err) return err;
  } else {
    HIP_TRY(launch_pack(c->du, c->d, KnotSlice(), c->ref.r, r, s.stream, c->d.batch));
    HIP_TRY(hipStreamSynchronize(s.stream));
  }
  note_elapsed(c, s);
  return NDLQR_OK;
}


// ------------------------------------------------------------------------------ active-set polish
// ndlqr_hip_polish_box (kernels_box_polish.hpp): the active set read off the latest constrained
// solve, QR shifted by sigma on its entries inside a ShiftedQR scope and factored as box_factor does, then per round up to
// max_steps steps of residual (double-double, on the saved unshifted QR) -> re-solve -> polish_update, the validation of
// every problem's last accepted iterate, and -- while a set changed and rounds remain -- the corrected sets shifted and
// factored again. Nothing is read back between the launches of a step; one word per step tells whether a problem still
// runs, two words per round whether a set changed.

// the steps of one round on the current factorisation
// the accepted iterate and what defines the system of a polish or of its adjoint (lo == nullptr: c = 0)
struct PolishSystem {
  const double* res;  // b
  const double *lo, *hi;
  double *z, *mu, *bt;
  int *state, *here;
};
static int polish_steps(NdlqrHipCtx* c, hipStream_t st, bool strict, int max_steps, const PolishSystem& y) {
  const ndlqr::Dims& d = c->d;
  PolishState& p = c->pol;
  const int nslots = max_steps + 1;
  const double* qr = c->box.qr_save;  // (the unshifted diagonal)
  HIP_TRY(hipMemsetAsync(p.norms, 0, sizeof(unsigned long long) * PolishState::norm_count(d), st));
  int e = launch_residual_dd_on(c, qr, y.bt, y.z, nullptr, p.r, p.norms, nslots, 0);
  if (e) return e;
  for (int step = 1; step <= max_steps + 1; ++step) {
    const int form = step <= max_steps;
    if (form) {
      e = launch_resolve(c, p.r, p.delta, "polish: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
    }
    launch_strict(strict, ndlqr::polish_update, dim3(d.batch), dim3(256), 0, st, d, step, form,
                  (const unsigned long long*)p.norms, (const double*)p.sig, y.lo, y.hi, c->box.bstride,
                  (const unsigned char*)p.code, y.res, (const double*)p.delta, y.z, y.mu, y.bt, p.zc, p.muc, p.btc, y.state,
                  y.here, p.word);
    HIP_TRY(hipGetLastError());
    if (!form) break;
    e = launch_residual_dd_on(c, qr, p.btc, p.zc, nullptr, p.r, p.norms, nslots, step);
    if (e) return e;
    if (step >= 2) {  // one word: how many problems still run
      HIP_TRY(hipMemcpyAsync(p.h_word, p.word, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (p.h_word[0] == 0) break;
    }
  }
  return NDLQR_OK;
}

int ndlqr_hip_polish_box(NdlqrHipCtx* c, double sigma, int max_steps, int max_rounds, int* steps, int* status) {
  if (!c || !(sigma > 0.0) || !(sigma < HUGE_VAL) || max_steps < 1 || max_steps > kPolishMaxSteps || max_rounds < 0)
    return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_polish_box")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_polish_box")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_polish_box");
  if (c->box.soln_gen == 0 || c->box.soln_gen != c->soln_gen || !c->box.have_vy || c->inputs_replaced)
    return refuse("ndlqr_hip_polish_box: the resident solution is not that of the latest constrained solve (a solve, step, "
                  "re-solve, polish, new inputs or new bounds came after it)");
  if (c->box.kept.time_shard) return refuse("ndlqr_hip_polish_box: not available on a time-axis shard");
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  int err = refuse_foreign_iters_status(c, "ndlqr_hip_polish_box", steps, status);
  if (err) return err;
  HIP_TRY(c->pol.ensure(d, c->set[0].stream));
  // 1. everything idle, the primary set current with an up-to-date right-hand side
  HIP_TRY(sync_all(c));
  c->cur = 0;
  err = rhs_make_current(c, 0xFu);
  if (err) return err;
  BufferSet& s = c->set[0];
  PolishState& p = c->pol;
  const hipStream_t st = s.stream;
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  const unsigned pol_flags = c->flags | (strict ? NDLQR_FLAG_KEEP_FACT : NDLQR_FLAG_KEEP_RECORDS);
  const double* lo = c->box.lo;
  const double* hi = c->box.hi;
  const size_t bs = c->box.bstride;
  p.fact = false;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  // 2. sigma, codes, the starting iterate (before the first factorisation overwrites the resident solution)
  hipLaunchKernelGGL(ndlqr::polish_sigma, dim3(d.batch), dim3(256), 0, st, c->du, d, sigma, (const double*)c->QR, p.sig);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(p.word, 0, 2 * sizeof(int), st));
  hipLaunchKernelGGL(ndlqr::polish_start, dim3(d.N, d.batch), dim3(64), 0, st, d, (const double*)c->box.rho, lo, hi, bs,
                     (const double*)c->box.v, (const double*)c->box.y, (const int*)c->box.status, (const double*)s.rhs,
                     (const double*)s.z, p.z0, p.z, p.code, p.mu, p.bt, p.state, p.steps, p.here, p.word);
  HIP_TRY(hipGetLastError());
  bool factored = false;
  int not_spd = NDLQR_OK;
  ShiftedQR shifted(c);
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto rounds = [&]() -> int {
    int e = shifted.open_unshifted(pol_flags);
    if (e) return e;
    for (int round = 0; round <= max_rounds; ++round) {
      // 3. shift by sigma on the active entries, factor
      if (round > 0) {
        e = shifted.restore();
        if (e) return e;
      }
      hipLaunchKernelGGL(ndlqr::polish_shift_qr, dim3(d.N, d.batch), dim3(64), 0, st, d, (const double*)p.sig,
                         (const unsigned char*)p.code, c->QR);
      HIP_TRY(hipGetLastError());
      factored = true;
      e = box_factor(c, st, &not_spd, "ndlqr_hip_polish_box", "Q, R + sigma on the active entries");
      if (e) return e;
      // 4. the steps
      // (word[0]: the problems that run in this round, counted by polish_start / the previous round's validation)
      e = polish_steps(c, st, strict, max_steps, {s.rhs, lo, hi, p.z, p.mu, p.bt, p.state, p.here});
      if (e) return e;
      // 5. validation; the sets that changed
      HIP_TRY(hipMemsetAsync(p.word, 0, 2 * sizeof(int), st));
      hipLaunchKernelGGL(ndlqr::polish_validate, dim3(d.batch), dim3(256), 0, st, d, round == max_rounds ? 1 : 0, lo, hi, bs,
                         (const double*)s.rhs, p.code, p.z, p.mu, p.bt, p.state, p.steps, p.here, p.word);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(p.h_word, p.word, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (p.h_word[1] == 0) break;
    }
    // 6. deliver
    hipLaunchKernelGGL(ndlqr::polish_finish, dim3(d.N, d.batch), dim3(64), 0, st, d, (const double*)c->box.rho,
                       (const int*)p.state, (const unsigned char*)p.code, (const double*)p.z, (const double*)p.mu,
                       (const double*)p.z0, s.z, c->box.v, c->box.y);
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = rounds();
  // 7. restore QR, bookkeeping
  const KeptState shifted_kept = c->kept;  // (close() forgets it for the plain API)
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (err) {
    c->forget_shifted();
    if (!not_spd) c->state_dirty = true;  // (a failed launch; a non-positive pivot leaves the device state clean)
    if (factored) c->z_invalid = true;    // (the factorisation overwrote the resident solution)
    (void)hipStreamSynchronize(st);
    return err;
  }
  note_solution(c);  // (polish_finish wrote the resident solution: whatever belonged to the ADMM solution no longer applies)
  p.soln_gen = p.adj_gen = 0;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = deliver_iters_status(c, st, p.steps, p.state, steps, status);
  if (err) return err;  // (nothing remembered: the caller never learnt which problems were polished)
  note_elapsed(c, s);
  p.fact = true;  // (box_factor dropped the ADMM's)
  p.flags = pol_flags;
  p.kept = shifted_kept;
  p.soln_gen = c->soln_gen;
  return NDLQR_OK;
}

// The adjoint of the polished active-set system, K w + E_A' nu = g, E_A w = 0, on the remembered polish factorisation: the
// loop of the polish with b = the packed g, c = 0, start w = nu = 0, the final codes; nothing is factored, no rounds. The
// right-hand-side columns of the kept records are saved and restored as for the other adjoints.
int ndlqr_hip_solve_polished_adjoint(NdlqrHipCtx* c, const double* g, int max_steps, int* steps, int* status) {
  if (!c || !g || max_steps < 1 || max_steps > kPolishMaxSteps) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_solve_polished_adjoint")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_polished_adjoint")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_solve_polished_adjoint");
  if (c->pol.soln_gen == 0 || c->pol.soln_gen != c->soln_gen || !c->pol.fact || c->inputs_replaced)
    return refuse("ndlqr_hip_solve_polished_adjoint: the resident solution is not that of the latest polish, or its "
                  "factorisation is gone (a solve, step, re-solve, new inputs or new bounds came after it)");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<1> ga = {{const_cast<double*>(g)}, {((size_t)u.rows * u.N - u.m) * d.batch}};
  int err = ga.classify(c, "ndlqr_hip_solve_polished_adjoint", "g lies");
  if (!err) err = refuse_foreign_iters_status(c, "ndlqr_hip_solve_polished_adjoint", steps, status);
  if (err) return err;
  PolishState& p = c->pol;
  HIP_TRY(c->adj.ensure(d, c->set[0].stream));
  HIP_TRY(p.ensure_adjoint(d));
  HIP_TRY(c->grad_stage.grow(ga.stage));
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  ga.place(c);
  err = ga.copy(st, true);
  if (err) return err;
  c->adj.gen = c->abox.gen = p.adj_gen = 0;
  const bool strict = (p.flags & NDLQR_FLAG_STRICT_FP) != 0;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  ShiftedQR shifted(c);
  const auto run = [&]() -> int {
    hipLaunchKernelGGL(ndlqr::adjoint_rhs_generic, dim3(d.N, d.batch), dim3(64), 0, st, u, d, (const double*)ga.dev[0],
                       c->adj.rhs);
    HIP_TRY(hipGetLastError());
    int e = shifted.open_unshifted(p.flags);
    if (e) return e;
    hipLaunchKernelGGL(ndlqr::polish_shift_qr, dim3(d.N, d.batch), dim3(64), 0, st, d, (const double*)p.sig,
                       (const unsigned char*)p.code, c->QR);
    HIP_TRY(hipGetLastError());
    c->kept = p.kept;
    e = shifted.save_record_columns();
    if (e) return e;
    hipLaunchKernelGGL(ndlqr::box_fill_rho, dim3((d.batch + 255) / 256), dim3(256), 0, st, d.batch, 1.0, p.ones);
    HIP_TRY(hipMemsetAsync(p.word, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(ndlqr::polish_adjoint_start, dim3(d.N, d.batch), dim3(64), 0, st, d, (const int*)p.state,
                       (const double*)c->adj.rhs, c->adj.z, p.nu, p.abt, p.astate, p.asteps, p.ahere, p.word);
    HIP_TRY(hipGetLastError());
    e = polish_steps(c, st, strict, max_steps, {c->adj.rhs, nullptr, nullptr, c->adj.z, p.nu, p.abt, p.astate, p.ahere});
    if (e) return e;
    hipLaunchKernelGGL(ndlqr::polish_adjoint_finish, dim3((d.batch + 255) / 256), dim3(256), 0, st, d.batch,
                       (const unsigned long long*)p.norms, p.astate, p.asteps, (const int*)p.ahere);
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = run();
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (err) {
    c->state_dirty = true;
    (void)hipStreamSynchronize(st);
    return err;
  }
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = deliver_iters_status(c, st, p.asteps, p.astate, steps, status);
  if (err) return err;
  note_elapsed(c, s);
  c->adj.gen = c->soln_gen;
  p.adj_gen = c->soln_gen;
  return NDLQR_OK;
}

// developer / test hook: the entry codes of the latest polish in the caller's block sizes, [batch][N][n+m] bytes (host)
int ndlqr_hip_download_polish_codes(NdlqrHipCtx* c, unsigned char* codes) {
  if (!c || !codes) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_polish_codes")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_polish_codes")) return cerr;
  if (c->pol.soln_gen == 0 || c->pol.soln_gen != c->soln_gen)
    return refuse("ndlqr_hip_download_polish_codes: the resident solution is not that of a polish");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  std::vector<unsigned char> h(doubles_QR(d));
  HIP_TRY(hipMemcpy(h.data(), c->pol.code, h.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < d.batch; ++b)
    for (int k = 0; k < d.N; ++k)
      for (int j = 0; j < u.n + u.m; ++j)
        codes[((size_t)b * u.N + k) * (u.n + u.m) + j] = h[((size_t)b * d.N + k) * d.w + (j < u.n ? j : d.n + (j - u.n))];
  return NDLQR_OK;
}


// Several right-hand sides per problem against ONE kept factorisation each (SURVEY.md 8(f)-2 "multiple right-hand
// sides"; the reference's NdData holds a single one, src/nddata.h:70-75): nrhs x batch right-hand sides, flat host arrays
// q, d [nrhs][batch][N][n], r [nrhs][batch][N][m], x0 [nrhs][batch][n] in the layout of ndlqr_BatchSetRhsFlat, solutions
// [nrhs][batch][nvars] into `soln`. Needs the compact records of a solve with NDLQR_FLAG_KEEP_RECORDS on the
// level-per-launch schedule (rec_compact). The right-hand sides are solved in chunks of at most 65 535 / batch sets;
// right-hand side j of a chunk reads the inputs and records of problem j % batch (they stay in the caches when batch is
// small: one problem x 1024 right-hand sides moves the right-hand sides and solutions and little else), its z_sep go to
// an array of their own. Blocking; the device time of the kernels alone is what ndlqr_hip_last_solve_ms reports afterwards.
// nknots == 0: whole solution vectors [nrhs][batch][nvars]; else knots [knot0, knot0 + nknots), blocks of `blocks`,
// [nrhs][batch][nknots][width] -- and only the workgroups of the last launch that hold them run (the rest of a vector is
// never produced: nothing keeps these solutions on the device anyway)
static int solve_multi_rhs(NdlqrHipCtx* c, int nrhs, const double* q, const double* r, const double* dd, const double* x0,
                           const KnotSlice& sel, double* soln) {
  if (!c || nrhs <= 0 || !q || !r || !dd || !x0 || !soln) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, sel.nknots > 0 ? "ndlqr_hip_solve_multi_rhs_slices" : "ndlqr_hip_solve_multi_rhs")) return herr;
  if (const int cerr = need_diagonal_cost(c, sel.nknots > 0 ? "ndlqr_hip_solve_multi_rhs_slices" : "ndlqr_hip_solve_multi_rhs")) return cerr;
  if (sel.nknots > 0 && !sel.valid(c->d.N, 15u)) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& st = c->set[0];
  const SmallInstance* inst = kept_instance(c);
  if (!inst || !c->kept.rec_complete || !c->kept.rec_compact)
    return refuse("multiple right-hand sides need the compact records of a solve with NDLQR_FLAG_KEEP_RECORDS on a "
                  "size-specialised shape (level-per-launch schedule: batch x N / 4 > 2048, or NDLQR_TREE=0)");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  // sets of right-hand sides per chunk: the chunk's count rides on gridDim.y, and its buffers stay within ~2 GB
  size_t per_set = (size_t)d.batch;
  size_t sets = 65535 / per_set;
  const size_t bytes_per = sizeof(double) * (size_t)d.N * (2 * d.rows + d.n + 2 * u.rows);
  while (sets > 1 && sets * per_set * bytes_per > ((size_t)2 << 30)) sets >>= 1;
  if (sets > (size_t)nrhs) sets = (size_t)nrhs;
  if (sets == 0) return NDLQR_ERR_INVALID;
  if (c->multi.ensure(d, u, sets * per_set, st.stream) != hipSuccess) {
    (void)hipGetLastError();
    g_last_error = "buffers of the multiple right-hand sides do not fit on the device";
    return NDLQR_ERR_INVALID;
  }
  double total_ms = 0.0;
  for (size_t s0 = 0; s0 < (size_t)nrhs; s0 += sets) {
    const size_t ns = (size_t)nrhs - s0 < sets ? (size_t)nrhs - s0 : sets, count = ns * per_set;
    ndlqr::Dims uc = u, dc = d;
    uc.batch = dc.batch = (int)count;  // (the pack kernels index problems by their position alone)
    const size_t nq = count * u.N * u.n, nr = count * u.N * u.m, nx = count * u.n;
    double* in = c->multi.in;
    HIP_TRY(hipMemcpyAsync(in, q + s0 * per_set * u.N * u.n, sizeof(double) * nq, hipMemcpyHostToDevice, st.stream));
    HIP_TRY(hipMemcpyAsync(in + nq, r + s0 * per_set * u.N * u.m, sizeof(double) * nr, hipMemcpyHostToDevice, st.stream));
    HIP_TRY(hipMemcpyAsync(in + nq + nr, dd + s0 * per_set * u.N * u.n, sizeof(double) * nq, hipMemcpyHostToDevice, st.stream));
    HIP_TRY(hipMemcpyAsync(in + 2 * nq + nr, x0 + s0 * per_set * u.n, sizeof(double) * nx, hipMemcpyHostToDevice, st.stream));
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<false>, dim3(512), dim3(256), 0, st.stream, uc, dc, (const double*)in,
                       (const double*)(in + nq), (const double*)(in + nq + nr), (const double*)(in + 2 * nq + nr), c->multi.rhs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_start, st.stream));
    const ApplySlice apply_slice(c, sel);
    if (!inst->multi(c, (int)count, c->multi.rhs, c->multi.zsep, c->multi.fsum, c->multi.ytop, c->multi.z)) {
      g_last_error = "multiple right-hand sides: this shape / horizon has no such form";
      return NDLQR_ERR_INVALID;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_stop, st.stream));
    const int derr = deliver(uc, dc, sel, c->multi.z, soln + s0 * per_set * sel.doubles(u), false, c->multi.out,
                             hipMemcpyDeviceToHost, st.stream, (unsigned)count);
    if (derr) return derr;
    HIP_TRY(hipStreamSynchronize(st.stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, st.ev_start, st.ev_stop) == hipSuccess) total_ms += ms;
  }
  c->last_ms = total_ms;
  c->timing_pending = false;
  return NDLQR_OK;
}
int ndlqr_hip_solve_multi_rhs(NdlqrHipCtx* c, int nrhs, const double* q, const double* r, const double* dd,
                              const double* x0, double* soln) {
  return solve_multi_rhs(c, nrhs, q, r, dd, x0, KnotSlice(), soln);
}
int ndlqr_hip_solve_multi_rhs_slices(NdlqrHipCtx* c, int nrhs, const double* q, const double* r, const double* dd,
                                     const double* x0, int knot0, int nknots, unsigned blocks, double* out) {
  if (nknots <= 0) return NDLQR_ERR_INVALID;
  return solve_multi_rhs(c, nrhs, q, r, dd, x0, KnotSlice{knot0, nknots, blocks}, out);
}

int ndlqr_hip_synchronize(NdlqrHipCtx* c) {
  if (!c) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  {
    const hipError_t se = sync_all(c);
    if (se != hipSuccess) { c->state_dirty = true; return fail("hipStreamSynchronize", se); }
  }
  if (c->timing_pending) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->set[c->cur].ev_start, c->set[c->cur].ev_stop));
    c->last_ms = ms;
    c->timing_pending = false;
    // info[batch] = cumulative batch-wide count of non-positive pivots: failures since the last synchronisation
    int seen = 0;  // the counter is cumulative: the larger of the two sets' copies is the newer one
    for (const BufferSet& s : c->set)
      if (s.h_fail && *s.h_fail > seen) seen = *s.h_fail;
    c->last_failures = seen - c->fail_base;
    c->fail_base = seen;
  }
  for (auto& p : c->pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
      c->slot_ms[p.slot] += ms;
      c->slot_launches[p.slot] += 1;
    }
    c->event_pool.push_back(p.start);
    c->event_pool.push_back(p.stop);
  }
  c->pending.clear();
  return NDLQR_OK;
}

double ndlqr_hip_last_solve_ms(NdlqrHipCtx* c) { return c ? c->last_ms : -1.0; }
int ndlqr_hip_cholesky_failures(NdlqrHipCtx* c) { return c ? c->last_failures : NDLQR_ERR_INVALID; }

int ndlqr_hip_profile_slots(NdlqrHipCtx* c) { return c ? (int)SLOT_COUNT : 0; }
int ndlqr_hip_profile_get(NdlqrHipCtx* c, int slot, char* name, int name_cap, double* total_ms, int* launches) {
  if (!c || slot < 0 || slot >= SLOT_COUNT) return NDLQR_ERR_INVALID;
  if (name && name_cap > 0) { strncpy(name, kSlotNames[slot], (size_t)name_cap - 1); name[name_cap - 1] = '\0'; }
  if (total_ms) *total_ms = c->slot_ms[slot];
  if (launches) *launches = c->slot_launches[slot];
  return NDLQR_OK;
}
int ndlqr_hip_profile_reset(NdlqrHipCtx* c) {
  if (!c) return NDLQR_ERR_INVALID;
  memset(c->slot_ms, 0, sizeof(c->slot_ms));
  memset(c->slot_launches, 0, sizeof(c->slot_launches));
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ downloads

// Solutions of problems [p0, p0 + count) as [count][nvars]: a pack kernel gathers them into the transfer staging
// (the device layout carries the unused trailing input slot of every problem, src/solver.c:64), then ONE contiguous
// copy brings them down -- straight into `soln` when that is pinned memory (ndlqr_hip_host_alloc), through two
// pinned 8 MB bounce buffers otherwise (the copy of chunk i overlaps the host memcpy of chunk i-1). The strided
// hipMemcpy2D into pageable memory this replaces ran at 5.4 GB/s.
int ndlqr_hip_download_solutions(NdlqrHipCtx* c, int p0, int count, double* soln) {
  if (!c || !soln || p0 < 0 || count <= 0 || p0 + count > c->d.batch) return NDLQR_ERR_INVALID;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_download_solutions");
  return download_packed(c, c->set[c->latest].z, p0, count, soln);
}
// ... of the blocks [batch][N][2n+m] at zsrc (the latest solution, or the adjoint solution)
static int download_packed(NdlqrHipCtx* c, const double* zsrc, int p0, int count, double* soln) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  HIP_TRY(s.ensure_xfer(c->du));
  const size_t nvars = (size_t)c->du.rows * c->du.N - c->du.m, pitch = (size_t)d.rows * d.N;
  hipStream_t st = s.stream;
  HIP_TRY(launch_pack(c->du, d, KnotSlice(), zsrc + p0 * pitch, s.xfer, st, count));
  if (c->cost.dense) HIP_TRY(cost_map_back(c, s.xfer, p0, count, st));  // the reduced variables -> the caller's, in the staging
  const size_t total = nvars * count;
  if (where(soln, c->device) == Where::Pinned) {
    HIP_TRY(hipMemcpyAsync(soln, s.xfer, sizeof(double) * total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NDLQR_OK;
  }
  const size_t chunk = (8u << 20) / sizeof(double);
  if (total <= chunk / 8) {  // small: one synchronous copy (the runtime stages it)
    HIP_TRY(hipMemcpyAsync(soln, s.xfer, sizeof(double) * total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NDLQR_OK;
  }
  for (int i = 0; i < 2; ++i)
    HIP_TRY(c->h_stage[i].ensure(chunk));
  hipEvent_t done[2] = {take_event(c), take_event(c)};
  const size_t nchunks = (total + chunk - 1) / chunk;
  hipError_t e = hipSuccess;
  for (size_t i = 0; i <= nchunks && e == hipSuccess; ++i) {
    if (i < nchunks) {  // (buffer i & 1 held chunk i - 2, which the previous iteration copied out)
      const size_t off = i * chunk, len = total - off < chunk ? total - off : chunk;
      e = hipMemcpyAsync(c->h_stage[i & 1], s.xfer + off, sizeof(double) * len, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipEventRecord(done[i & 1], st);
    }
    if (i > 0 && e == hipSuccess) {
      const size_t off = (i - 1) * chunk, len = total - off < chunk ? total - off : chunk;
      e = hipEventSynchronize(done[(i - 1) & 1]);
      if (e == hipSuccess) memcpy(soln + off, c->h_stage[(i - 1) & 1], sizeof(double) * len);
    }
  }
  c->event_pool.push_back(done[0]);
  c->event_pool.push_back(done[1]);
  if (e != hipSuccess) return fail("ndlqr_hip_download_solutions", e);
  return NDLQR_OK;
}

const char* ndlqr_hip_schedule(const NdlqrHipCtx* c) { return c ? c->kept.schedule : "none"; }

int ndlqr_hip_factors_valid(const NdlqrHipCtx* c) { return c && c->kept.fact_valid ? 1 : 0; }

int ndlqr_hip_pack_solutions_device(NdlqrHipCtx* c, double* dst) {
  if (!c || !dst) return NDLQR_ERR_INVALID;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_pack_solutions_device");
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  // on the stream of the latest solve: ordered behind it, asynchronous for the caller
  HIP_TRY(launch_pack(c->du, d, KnotSlice(), c->set[c->latest].z, dst, c->set[c->latest].stream, d.batch));
  if (c->cost.dense) HIP_TRY(cost_map_back(c, dst, 0, d.batch, c->set[c->latest].stream));
  return NDLQR_OK;
}

int ndlqr_hip_kkt_residual(NdlqrHipCtx* c, double* res, double* bnorm) {
  if (!c || !res) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_kkt_residual")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_kkt_residual");
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->kkt_out.ensure(2 * (size_t)d.batch));
  double* out = c->kkt_out;
  HIP_TRY(sync_all(c));
  hipLaunchKernelGGL(ndlqr::kkt_residual_generic, dim3(d.batch), dim3(256), 0, s.stream, d, c->AB, c->QR, s.rhs,
                     c->set[c->latest].z, out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(res, out, sizeof(double) * d.batch, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess && bnorm)
    e = hipMemcpyAsync(bnorm, out + d.batch, sizeof(double) * d.batch, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  if (e != hipSuccess) return fail("ndlqr_hip_kkt_residual", e);
  return NDLQR_OK;
}

int ndlqr_hip_download_rhs_blocks(NdlqrHipCtx* c, int p, double* z_full) {
  if (!c || !z_full || p < 0 || p >= c->d.batch) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_rhs_blocks")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_rhs_blocks")) return cerr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_download_rhs_blocks");
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  const size_t pitch = (size_t)d.rows * d.N;
  HIP_TRY(sync_all(c));
  const double* zp = c->set[c->latest].z + p * pitch;
  if (c->padded) {
    const size_t upitch = (size_t)c->du.rows * d.N;
    HIP_TRY(c->grow_pad_stage(upitch));
    hipLaunchKernelGGL(ndlqr::unpad_blocks_generic, dim3(d.N), dim3(64), 0, s.stream, c->du, d, zp, c->pad_stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(z_full, c->pad_stage, sizeof(double) * upitch, hipMemcpyDeviceToHost, s.stream));
  } else {
    HIP_TRY(hipMemcpyAsync(z_full, zp, sizeof(double) * pitch, hipMemcpyDeviceToHost, s.stream));
  }
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

int ndlqr_hip_download_factors(NdlqrHipCtx* c, int p, double* fact) {
  if (!c || !fact || p < 0 || p >= c->d.batch) return NDLQR_ERR_INVALID;
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_download_factors")) return herr;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_download_factors")) return cerr;
  if (!c->kept.fact_valid) return refuse("factor download needs NDLQR_FLAG_KEEP_FACT set before the solve");
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  const size_t count = (size_t)d.K * d.N * d.fb;
  std::vector<double> tmp(count);
  HIP_TRY(hipMemcpyAsync(tmp.data(), c->F + p * count, sizeof(double) * count, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  // device: [level][knot][row][col] row-major -> reference: block (k,level) at (k + N*level)*fb,
  // sub-blocks lambda (n x n), state (n x n), input (m x n), each column-major (src/nddata.c:40-53)
  // (a padded shape: the device blocks have np >= n columns and rows lambda [0, np), state [np, 2 np), input
  //  [2 np, 2 np + mp); the caller gets the real rows and columns)
  const int n = c->du.n, m = c->du.m, np = d.n;
  const size_t ufb = c->du.fb;
  for (int lvl = 0; lvl < d.K; ++lvl)
    for (int k = 0; k < d.N; ++k) {
      const double* src = tmp.data() + ((size_t)lvl * d.N + k) * d.fb;
      double* dst = fact + ((size_t)k + (size_t)d.N * lvl) * ufb;
      for (int j = 0; j < n; ++j) {
        for (int i = 0; i < n; ++i) dst[i + n * j] = src[i * np + j];
        for (int i = 0; i < n; ++i) dst[n * n + i + n * j] = src[(np + i) * np + j];
        for (int i = 0; i < m; ++i) dst[2 * n * n + i + m * j] = src[(2 * np + i) * np + j];
      }
    }
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ dense helpers

// Host matrices in, host matrices out (the reference's Matrix* layer, src/linalg.c:55-190). One call = one
// packed H2D copy of the operands, one kernel, one D2H copy of the result, all on the stream of a pooled
// scratch (a device buffer + a pinned staging buffer, grown on demand): no allocation and no blocking
// null-stream copy per call, and calls from different host threads (the reference's tests call these from
// an OpenMP team, test/parallel_test.c:30-239) run side by side on different scratches.
namespace {
struct DenseScratch {
  DevBuf<double> dev;       // both of one capacity, grown on demand
  PinnedBuf<double> host;
  hipStream_t stream = nullptr;
  int device = -1;  // the device its stream and buffer live on: leased only to calls whose current device is this one
};
std::mutex g_dense_mu;
std::vector<DenseScratch*> g_dense_pool;  // idle scratches; never freed (bounded by the peak concurrency)

struct DenseLease {
  DenseScratch* s = nullptr;
  DenseLease() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::lock_guard<std::mutex> lock(g_dense_mu);
    for (size_t i = g_dense_pool.size(); i-- > 0;)
      if (g_dense_pool[i]->device == dev) {
        s = g_dense_pool[i];
        g_dense_pool.erase(g_dense_pool.begin() + (long)i);
        return;
      }
    s = new DenseScratch();
    s->device = dev;
  }
  ~DenseLease() {
    std::lock_guard<std::mutex> lock(g_dense_mu);
    g_dense_pool.push_back(s);
  }
  int ensure(size_t doubles) {
    if (!s->stream) HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    size_t cap = s->host.count() ? s->host.count() : 4096;
    while (cap < doubles) cap *= 2;
    HIP_TRY(s->dev.grow(cap));
    HIP_TRY(s->host.grow(cap));
    return NDLQR_OK;
  }
};
}  // namespace

static int dense_ready() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    g_last_error = "no HIP device for the dense Matrix* helpers (no CPU fallback)";
    fprintf(stderr, "ndlqr_hip: %s\n", g_last_error.c_str());
    return NDLQR_ERR_NO_DEVICE;
  }
  return NDLQR_OK;
}

int ndlqr_hip_gemm(int tA, int tB, int m, int n, int k, double alpha, const double* A, int lda,
                   const double* B, int ldb, double beta, double* C, int ldc) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (m <= 0 || n <= 0 || k < 0 || !A || !B || !C) return NDLQR_ERR_INVALID;
  // stored shapes: A is (Ar x Ac) with leading dimension lda, ...; the last column ends after its rows
  const int Ar = tA ? k : m, Ac = tA ? m : k, Br = tB ? n : k, Bc = tB ? k : n;
  if (k > 0 && (lda < Ar || ldb < Br)) return NDLQR_ERR_INVALID;
  if (ldc < m) return NDLQR_ERR_INVALID;
  const size_t nA = k > 0 ? (size_t)lda * (Ac - 1) + Ar : 0, nB = k > 0 ? (size_t)ldb * (Bc - 1) + Br : 0,
               nC = (size_t)ldc * (n - 1) + m;
  DenseLease L;
  const int err = L.ensure(nA + nB + nC);
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, A, sizeof(double) * nA);
  memcpy(s->host + nA, B, sizeof(double) * nB);
  memcpy(s->host + nA + nB, C, sizeof(double) * nC);
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nA + nB + nC), hipMemcpyHostToDevice, s->stream));
  const int total = m * n;
  hipLaunchKernelGGL(ndlqr::dense_gemm, dim3((total + 255) / 256), dim3(256), 0, s->stream, tA, tB, m, n, k, alpha,
                     s->dev, lda, s->dev + nA, ldb, beta, s->dev + nA + nB, ldc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host + nA + nB, s->dev + nA + nB, sizeof(double) * nC, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(C, s->host + nA + nB, sizeof(double) * nC);
  return NDLQR_OK;
}

int ndlqr_hip_potrf_lower(int n, double* A, int lda) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (n <= 0 || !A) return NDLQR_ERR_INVALID;
  if (lda < n) return NDLQR_ERR_INVALID;
  const size_t nA = (size_t)lda * (n - 1) + n;
  DenseLease L;
  const int err = L.ensure(nA + 1);  // + one slot for the failure word
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, A, sizeof(double) * nA);
  s->host[nA] = 0.0;  // (all-zero bits: the int the kernel writes into starts at 0)
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nA + 1), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(ndlqr::dense_potrf, dim3(1), dim3(256), 0, s->stream, n, s->dev, lda,
                     reinterpret_cast<int*>(s->dev + nA));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host, s->dev, sizeof(double) * (nA + 1), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(A, s->host, sizeof(double) * nA);
  int info = 0;
  memcpy(&info, s->host + nA, sizeof(int));
  return info ? -1 : 0;
}

// which: 0 = L L' x = b (both substitutions), 1 = L x = b, 2 = L' x = b
static int dense_tri_solve(int which, int n, int nrhs, const double* Lm, int ldl, double* B, int ldb) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (n <= 0 || nrhs <= 0 || !Lm || !B) return NDLQR_ERR_INVALID;
  if (ldl < n || ldb < n) return NDLQR_ERR_INVALID;
  const size_t nL = (size_t)ldl * (n - 1) + n, nB = (size_t)ldb * (nrhs - 1) + n;
  DenseLease L;
  const int err = L.ensure(nL + nB);
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, Lm, sizeof(double) * nL);
  memcpy(s->host + nL, B, sizeof(double) * nB);
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nL + nB), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(ndlqr::dense_potrs, dim3((nrhs + 63) / 64), dim3(64), 0, s->stream, n, nrhs, s->dev, ldl,
                     s->dev + nL, ldb, which);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host + nL, s->dev + nL, sizeof(double) * nB, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(B, s->host + nL, sizeof(double) * nB);
  return NDLQR_OK;
}

int ndlqr_hip_potrs_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb) {
  return dense_tri_solve(0, n, nrhs, L, ldl, B, ldb);
}

int ndlqr_hip_trsv_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb, int transposed) {
  return dense_tri_solve(transposed ? 2 : 1, n, nrhs, L, ldl, B, ldb);
}

// developer hook (tools/debug_compare.py; not part of include/*.h): raw copy of an internal array,
// which = 0: separator records [batch][N][2 n^2 + n], 1: accumulator slots of the separator-only schedule
extern "C" long ndlqr_hip_debug_download(NdlqrHipCtx* c, int which, double* host, long count) {
  if (!c || !host) return -1;
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  const double* src = which == 0 ? s.rec : s.red;
  const size_t slot_doubles = ((size_t)d.n * (d.n + 1) + 2 * (size_t)d.n * d.n + 2 * d.n + 15) / 16 * 16;  // RedSlot<NX>::SIZE
  const size_t have = which == 0 ? (size_t)d.batch * d.N * (2 * d.n * d.n + d.n) : (size_t)d.batch * (d.N / 4) * slot_doubles;
  if (!src) return -1;
  const size_t n = (size_t)count < have ? (size_t)count : have;
  if (hipStreamSynchronize(s.stream) != hipSuccess) return -1;
  if (hipMemcpy(host, src, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long)n;
}

#ifdef NDLQR_SEGTIME
// developer instrumentation only (tools/segtime.py): read / clear the per-segment cycle sums
extern "C" int ndlqr_hip_debug_segments(unsigned long long* out, int n, int reset) {
  unsigned long long host[128];
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ndlqr::ndlqr_seg), sizeof(host)) != hipSuccess) return -1;
  for (int i = 0; i < n && i < 128; ++i) out[i] = host[i];
  if (reset) {
    for (int i = 0; i < 128; ++i) host[i] = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(ndlqr::ndlqr_seg), host, sizeof(host)) != hipSuccess) return -1;
  }
  return 128;
}
#endif
