// ndlqr_hip.hip -- gfx950 (MI355X, CDNA4) implementation of the device boundary in include/ndlqr_hip.h, the core
// unit: errors, context and memory management, the two-deep pipeline, uploads and packing, the SolvePlan and the launch
// sequences of the three kernel families, staged solve, time shard, steps and slices, rhs-only and multi-rhs re-solves,
// synchronisation, profile and downloads. Its kernels: kernels_generic.hpp, kernels_mfma.hpp (any n, m), the re-solve
// and back-substitution of kernels_reduced_solve.hpp; the size-specialised family is instantiated per block size in
// small_instance.hip (launch_small.hpp) and the separators of the runtime-sized separator-only family per tile count
// in reduced_instance.hip (launch_reduced.hpp). The optional features have a unit each (hip_grad.hip, hip_box.hip,
// hip_refine.hip, hip_cost.hip, hip_dense.hip); hip_host.hpp declares what they share with this one.
//
// Written for wave64 / gfx950 only; built with -ffp-contract=off so that every fused
// multiply-add in the kernels is an explicit fma() (fast mode) or an explicit mul + add
// (NDLQR_FLAG_STRICT_FP, which reproduces the reference's default CPU build bit for bit).
#include "hip_host.hpp"
#include "kernels_generic.hpp"
#include "kernels_mfma.hpp"
#include "launch_reduced.hpp"        // (ReducedInstance; its templates are instantiated in reduced_instance.hip)
#include "kernels_reduced_solve.hpp"
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
int fail(const char* what, hipError_t e) { return ndlqr_hip_fail(what, e); }
// records the message for ndlqr_hip_last_error(), prints it, returns NDLQR_ERR_INVALID
int refuse(const std::string& msg) {
  g_last_error = msg;
  fprintf(stderr, "ndlqr_hip: %s\n", g_last_error.c_str());
  return NDLQR_ERR_INVALID;
}

// Padded horizon (ndlqr_hip_create_ex): an entry point that is not carried through refuses here -- it would index the
// caller's arrays, which have du.N knots, with the device's d.N
int need_unpadded_horizon(const NdlqrHipCtx* c, const char* who) {
  if (c->du.N == c->d.N) return NDLQR_OK;
  return refuse(std::string(who) + ": not available for a padded horizon (horizon " + std::to_string(c->du.N) +
                " runs as " + std::to_string(c->d.N) + " knots); use a power-of-two horizon");
}

// Dense-cost mode (ndlqr_hip_init_dense): the resident problem is the unit-cost reduction of the
// caller's. An entry point that is not carried through refuses here -- the rows, records and arrays it would work on are
// those of the reduced system
int need_diagonal_cost(const NdlqrHipCtx* c, const char* who) {
  if (!c->cost.dense) return NDLQR_OK;
  return refuse(std::string(who) + ": not available in dense-cost mode (the resident problem is the unit-cost reduction "
                "ndlqr_InitializeBatchFlatDense left); use a diagonal initialiser");
}

Where where(const void* p, int device) {
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
  onoff("NDLQR_COMPACT1", &k.compact1);          // unset: by instance (launch_small)
  onoff("NDLQR_PAIR1", &k.pair1);                // unset: by instance (launch_small)
  onoff("NDLQR_BOTTOM_LDS16", &k.bottom_lds16);  // unset: by instance (launch_small)
  onoff("NDLQR_TOP_CHAIN", &k.top_chain);        // unset: by instance (launch_small)
  k.no_mfma = getenv("NDLQR_NO_MFMA") != nullptr;
  k.no_top = getenv("NDLQR_NO_TOP") != nullptr;
  k.top_levels_set = getenv("NDLQR_TOP_LEVELS") != nullptr;
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
void note_solution(NdlqrHipCtx* c) {
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
int need_full_solution(const NdlqrHipCtx* c, const char* who) {
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
hipError_t sync_all(NdlqrHipCtx* c) {
  hipError_t e = hipSuccess;
  for (const BufferSet& s : c->set)
    if (s.stream) { const hipError_t e2 = hipStreamSynchronize(s.stream); if (e == hipSuccess) e = e2; }
  return e;
}

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
// everything is idle and the current set's whole right-hand side has just been rewritten
void note_new_rhs(NdlqrHipCtx* c) {
  rhs_written_cur(c, 0xFu);
  next_solve_on_current_set(c);
}
// rhs_make_current: the current set's copy is brought up to date in the parts of `need` before a solve reads it. Only a
// change of flow gets here with something to do (full MPC steps followed by x0-only steps, a plain solve behind steps,
// the first solve on the other set after an upload): everything in flight is waited for, the stale parts are copied
// from the other set on this set's stream, and the other set's stream waits for that copy before it may rewrite its own.
int rhs_make_current(NdlqrHipCtx* c, unsigned need) {
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
  c->lin.active = false;
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
  c->lin.active = false;           // (... and ndlqr_hip_init_constrained this one)
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
  // a four-wavefront workgroup whose phases are mostly serial at this size; else the wider form, where there is one
  // (kReducedThreads, launch_reduced.hpp)
  p.threads = wpad <= kReducedThreads[p.nb][0] ? kReducedThreads[p.nb][0] : kReducedThreads[p.nb][1];
  if (wpad > p.threads) return p;  // one weight / rhs entry per thread (0: no wider form beyond 64 states)
  p.lds = sizeof(double) * (size_t)ndlqr::reduced_lds_doubles(npad, wpad, p.threads == kReducedThreads[p.nb][0]);
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

// ---- the separator launch of every tile count: one translation unit each (reduced_instance.hip); developer builds with
//      NDLQR_SINGLE_TU (tools/segtime.py) hold every instance here
#ifdef NDLQR_SINGLE_TU
#define NDLQR_REDUCED_INSTANCE(NB_) static const ReducedInstance NDLQR_REDUCED_NAME(NB_) = make_reduced_instance<NB_>();
#else
#define NDLQR_REDUCED_INSTANCE(NB_) extern const ReducedInstance NDLQR_REDUCED_NAME(NB_) __attribute__((visibility("hidden")));
#endif
NDLQR_REDUCED_INSTANCES
#undef NDLQR_REDUCED_INSTANCE
static const ReducedInstance* const kReducedInstances[kReducedMaxNB + 1] = {nullptr,
#define NDLQR_REDUCED_INSTANCE(NB_) &NDLQR_REDUCED_NAME(NB_),
    NDLQR_REDUCED_INSTANCES
#undef NDLQR_REDUCED_INSTANCE
};

static int launch_reduced_generic(NdlqrHipCtx* c, const ReducedGenericPlan& p) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  for (int l = 0; l < d.K; ++l) {
    ScopedSlot t(c, SLOT_SEP);
    kReducedInstances[p.nb]->separator(c, p, l);
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
    p.kept.rec1_compact = p.small.compact1;
    p.kept.level1_paired = p.small.pair1;
    p.kept.bottom_lds16 = p.small.lds16;
    p.kept.top_chain = p.small.chain;
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
hipError_t launch_pack(const ndlqr::Dims& u, const ndlqr::Dims& d, const KnotSlice& sel, const double* z, double* dst,
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
int launch_resolve(NdlqrHipCtx* c, const double* rhs, double* z, const char* refusal) {
  if (try_launch_rhs_records(c, rhs, z)) return NDLQR_OK;
  if (!c->kept.fact_valid) return refuse(refusal);
  if (c->flags & NDLQR_FLAG_STRICT_FP) launch_rhs_sweep<true>(c, rhs, z); else launch_rhs_sweep<false>(c, rhs, z);
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

// the flat q, r, d, x0 (this device's memory, or a device-side view of pinned memory; null: a part that is not replaced)
// packed into the current set's right-hand side, on its stream
hipError_t launch_pack_rhs(NdlqrHipCtx* c, const double* q, const double* r, const double* d, const double* x0) {
  BufferSet& s = c->set[c->cur];
  if (c->du.N != c->d.N)  // (a padded horizon: the per-entry guards)
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<true>, dim3(512), dim3(256), 0, s.stream, c->du, c->d, q, r, d, x0, s.rhs.get());
  else
    hipLaunchKernelGGL(ndlqr::pack_rhs_stream_generic<false>, dim3(512), dim3(256), 0, s.stream, c->du, c->d, q, r, d, x0, s.rhs.get());
  return hipGetLastError();
}

// ... in dense-cost mode: the slice `sel` of the reduced solutions at z through S (cost_deliver_slice), or the whole vectors
// packed and mapped back where they land (pack_solutions_generic + cost_apply) -- no CostPhase: a step never waits
static int deliver_dense(NdlqrHipCtx* c, const KnotSlice& sel, const double* z, double* dst, bool own, double* stage,
                         hipMemcpyKind kind, hipStream_t st) {
  double* tgt = own ? dst : stage;
  if (sel.nknots > 0) {
    HIP_TRY(cost_deliver_slice_on(c, sel, z, tgt, st));
  } else {
    HIP_TRY(launch_pack(c->du, c->d, sel, z, tgt, st, c->d.batch));
    HIP_TRY(cost_apply_on(c, tgt, 0, c->d.batch, st));
  }
  if (!own) HIP_TRY(hipMemcpyAsync(dst, stage, sizeof(double) * sel.doubles(c->du) * c->d.batch, kind, st));
  return NDLQR_OK;
}

// what the dense-cost twins of the step and slice functions refuse, `who` opening the message
static int need_dense_step(const NdlqrHipCtx* c, const char* who) {
  if (!c->cost.dense)
    return refuse(std::string(who) + ": the solver is not in dense-cost mode (ndlqr_InitializeBatchFlatDense); a "
                  "diagonal-cost problem takes the plain function");
  if (c->lin.active)
    return refuse(std::string(who) + ": not available in constrained mode (ndlqr_InitializeBatchFlatConstrained)");
  if (c->kept.time_shard) return refuse(std::string(who) + ": not available on a time-axis shard");
  return NDLQR_OK;
}
// ... and a slice that is none (`allowed`: KnotSlice::valid)
static int need_dense_slice(const NdlqrHipCtx* c, const char* who, const KnotSlice& sel, unsigned allowed) {
  if (sel.valid(c->du.N, allowed)) return NDLQR_OK;
  return refuse(std::string(who) + ": knots [" + std::to_string(sel.knot0) + ", " + std::to_string(sel.knot0 + sel.nknots) +
                "), blocks " + std::to_string(sel.blocks) + " is not a slice of a horizon of " + std::to_string(c->du.N) + " knots");
}
// ... and an array in another device's memory
static int need_own_memory(const NdlqrHipCtx* c, const char* who, std::initializer_list<const void*> arrays) {
  for (const void* p : arrays)
    if (p && where(p, c->device) == Where::OtherDevice)
      return refuse(std::string(who) + ": an array lies in the memory of another device than the solver's");
  return NDLQR_OK;
}

// One step: the parts q, r, dd, x0 (null: not replaced) of the right-hand side up, factor + solve (or the re-solve on
// kept records), `sel` of the solutions down into `soln`, all on the stream of the step's buffer set. dense: the arrays
// are in the caller's variables of a dense-cost problem -- S' on the way up and S on the way down, by the two kernels
// that work between the caller's arrays and the device layout (kernels_cost.hpp); everything else is the same step.
static int step_on_set(NdlqrHipCtx* c, const double* q, const double* r, const double* dd, const double* x0,
                       const KnotSlice& sel, double* soln, bool dense) {
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
  if (dense) HIP_TRY(cost_pack_rhs_on(c, written, view[0], view[1], view[2], view[3], s.rhs, st));
  else HIP_TRY(launch_pack_rhs(c, view[0], view[1], view[2], view[3]));
  rhs_written_cur(c, written);
  // NDLQR_SOLN_ONLY: nothing but the selected knots is wanted
  const ApplySlice apply_slice(c, sel, (sel.blocks & NDLQR_SOLN_ONLY) != 0);
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
  const bool own = where(soln, c->device) == Where::OwnDevice;
  err = dense ? deliver_dense(c, sel, s.z, soln, own, s.xfer, hipMemcpyDefault, st)
              : deliver(u, d, sel, s.z, soln, own, s.xfer, hipMemcpyDefault, st, d.batch);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  HIP_TRY(hipEventRecord(c->ev_step[c->step_count & 1u], st));
  c->step_set[c->step_count & 1u] = c->cur;
  ++c->step_count;
  c->timing_pending = true;
  c->state_dirty = false;
  return NDLQR_OK;
}

int ndlqr_hip_step_async(NdlqrHipCtx* c, const double* q, const double* r, const double* dd, const double* x0,
                         double* soln) {
  if (!c || !x0 || !soln) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_step_async")) return cerr;
  return step_on_set(c, q, r, dd, x0, c->sel, soln, false);
}

// The step of a dense-cost problem (ndlqr.h: ndlqr_BatchStepAsyncDense): q, r, d, x0 in the caller's variables, q and r
// together or neither; the slice is an argument (nknots == 0: the whole vectors), not the selection of the plain step.
int ndlqr_hip_step_dense_async(NdlqrHipCtx* c, const double* q, const double* r, const double* dd, const double* x0, int knot0,
                               int nknots, unsigned blocks, double* out) {
  static const char* const who = "ndlqr_hip_step_dense_async";
  if (!c) return NDLQR_ERR_INVALID;
  if (const int merr = need_dense_step(c, who)) return merr;
  if (!x0 || !out) return refuse(std::string(who) + ": x0 and the output are required");
  if ((q == nullptr) != (r == nullptr))
    return refuse(std::string(who) + ": q and r are replaced together or not at all (the reduced q needs both: q~ = L^-1 (q - G' r))");
  KnotSlice sel;  // (the whole vectors)
  if (nknots != 0) {
    sel = KnotSlice{knot0, nknots, blocks};
    if (const int serr = need_dense_slice(c, who, sel, 15u)) return serr;
  }
  if (const int oerr = need_own_memory(c, who, {q, r, dd, x0, out})) return oerr;
  return step_on_set(c, q, r, dd, x0, sel, out, true);
}

// Factor + solve of the resident problems, of which knots [knot0, knot0 + nknots) -- blocks `blocks` -- are computed by the
// last launch and written to `out` ([batch][nknots][width]; host, pinned or this device's memory), asynchronously: the
// solve of a loop that replaces A, B, Q, R as well (ndlqr_hip_pack_flat_device / uploads) and consumes u of knot 0.
// Consecutive calls alternate between the buffer sets like ndlqr_hip_solve_async; complete after ndlqr_hip_synchronize.
// (dense: the slice goes through S on its way out)
static int solve_slices_on_set(NdlqrHipCtx* c, const KnotSlice& sel, double* out, bool dense) {
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
  const bool own = where(out, c->device) == Where::OwnDevice;
  err = dense ? deliver_dense(c, sel, s.z, out, own, s.xfer, hipMemcpyDefault, st)
              : deliver(c->du, d, sel, s.z, out, own, s.xfer, hipMemcpyDefault, st, d.batch);
  if (err) return err;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  c->timing_pending = true;
  c->state_dirty = false;
  return NDLQR_OK;
}
int ndlqr_hip_solve_slices_async(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks, double* out) {
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!c || !out || !sel.valid(c->du.N, 15u)) return NDLQR_ERR_INVALID;
  if (const int cerr = need_diagonal_cost(c, "ndlqr_hip_solve_slices_async")) return cerr;
  return solve_slices_on_set(c, sel, out, false);
}
// everything the dense-cost twins of the two slice functions refuse by name
static int need_dense_slice_call(const NdlqrHipCtx* c, const char* who, const KnotSlice& sel, unsigned allowed, const double* out) {
  if (const int merr = need_dense_step(c, who)) return merr;
  if (!out) return refuse(std::string(who) + ": the output is required");
  if (const int serr = need_dense_slice(c, who, sel, allowed)) return serr;
  return need_own_memory(c, who, {out});
}
// ... of a dense-cost problem (ndlqr.h: ndlqr_SolveBatchSlicesAsyncDense)
int ndlqr_hip_solve_slices_dense_async(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks, double* out) {
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!c) return NDLQR_ERR_INVALID;
  if (const int serr = need_dense_slice_call(c, "ndlqr_hip_solve_slices_dense_async", sel, 15u, out)) return serr;
  return solve_slices_on_set(c, sel, out, true);
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
// ... of a dense-cost problem (ndlqr.h: ndlqr_CopyBatchSolutionSlicesDense): the slice in the caller's variables
int ndlqr_hip_download_selection_dense(NdlqrHipCtx* c, int knot0, int nknots, unsigned blocks, double* out) {
  static const char* const who = "ndlqr_hip_download_selection_dense";
  const KnotSlice sel = {knot0, nknots, blocks};
  if (!c) return NDLQR_ERR_INVALID;
  if (const int serr = need_dense_slice_call(c, who, sel, 7u, out)) return serr;
  BufferSet& s = c->set[c->cur];
  if (c->z_invalid || (c->z_partial && (knot0 < 8 * c->z_blk0 || knot0 + nknots > 8 * (c->z_blk0 + c->z_nblk))))
    return need_full_solution(c, who);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  HIP_TRY(s.ensure_xfer(c->du));
  const bool own = where(out, c->device) == Where::OwnDevice;
  const int derr = deliver_dense(c, sel, c->set[c->latest].z, out, own, s.xfer, hipMemcpyDefault, s.stream);
  if (derr) return derr;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

// Read-out for the tests: the latest right-hand side as it lies on the device, [batch][d.N][d.rows] doubles in the device's
// block sizes and horizon (ndlqr_hip_rhs_raw_doubles of them), into HOST memory -- the pad rows and the tail knots of a
// padded horizon included. Waits for everything in flight and brings the current buffer set's copy up to date first.
// Every mode.
size_t ndlqr_hip_rhs_raw_doubles(const NdlqrHipCtx* c) { return c ? doubles_z(c->d) : 0; }
int ndlqr_hip_download_rhs_raw(NdlqrHipCtx* c, double* out) {
  if (!c || !out) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  if (const int merr = rhs_make_current(c, 0xFu)) return merr;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipMemcpyAsync(out, s.rhs.get(), bytes_z(c->d), hipMemcpyDeviceToHost, s.stream));
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
  note_new_rhs(c);
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

// ------------------------------------------------------------------------------ services of the feature units (hip_host.hpp)

// the device time between the events of the (synchronised) set, for ndlqr_hip_last_solve_ms
void note_elapsed(NdlqrHipCtx* c, const BufferSet& s) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s.ev_start, s.ev_stop) == hipSuccess) c->last_ms = ms;
}

// The re-solves of the kept records write what depends on the right-hand side into them (z_sep / y~: the last n entries
// of every record) and, on the runtime-sized schedule, into the slots (gL | gR). Every re-solve recomputes those before
// it reads them; the adjoint solve still leaves them as it found them: saved before, restored after (2 n doubles per
// knot instead of the whole records).
hipError_t adjoint_scratch(NdlqrHipCtx* c, bool restore) {
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

// is there an adjoint of the resident solution of the resident inputs?
int need_adjoint(const NdlqrHipCtx* c, const char* who) {
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  if (c->adj.gen == 0 || c->adj.gen != c->soln_gen)
    return refuse(std::string(who) + ": no adjoint of the resident solution (ndlqr_hip_solve_adjoint after the latest solve)");
  if (c->inputs_replaced) return refuse(std::string(who) + ": the inputs were replaced after the factorisation");
  return NDLQR_OK;
}

// What is resident factored on the primary set as a plain solve does it (the resident solution is overwritten), with
// the pivot check: *not_spd = NDLQR_ERR_NOT_SPD, which is returned, when a pivot was not positive.
// (who, what: the entry point and the matrix, for the message)
int factor_resident(NdlqrHipCtx* c, hipStream_t st, int* not_spd, const char* who, const char* what) {
  c->forget_shifted();
  SolvePlan plan;
  int err = prepare_solve(c, &plan);  // (KEEP_*: stream-ordered on the primary set)
  if (!err) err = launch_solve(c, plan);
  if (err) return err;
  c->state_dirty = false;
  HIP_TRY(hipStreamSynchronize(st));
  // a non-positive pivot (of a shifted factorisation: e.g. Q or R <= 0 on an unbounded entry)
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

// iters / status of a constrained solve or its adjoint (`who`) go to host memory or this device's
int refuse_foreign_iters_status(const NdlqrHipCtx* c, const char* who, const int* iters, const int* status) {
  for (const int* p : {iters, status})
    if (p && where(p, c->device) == Where::OtherDevice)
      return refuse(std::string(who) + ": iters / status lie in the memory of another device than the solver's");
  return NDLQR_OK;
}

// The per-problem iteration counts and status words behind everything enqueued on st, for the caller (null: not asked
// for); a problem still running at max_iter (0) reports 2: the last iterate. Synchronises st.
int deliver_iters_status(const NdlqrHipCtx* c, hipStream_t st, const int* d_iters, const int* d_status, int* iters,
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

unsigned long long ndlqr_hip_factor_count(const NdlqrHipCtx* c) { return c ? c->factor_count : 0; }

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
// info[0 .. batch): the per-problem words as the device holds them (cumulative; zeroed at creation and by the recovery
// of prepare_solve). Waits for everything in flight; touches neither last_failures nor fail_base.
int ndlqr_hip_download_failure_counts(NdlqrHipCtx* c, int* counts) {
  if (!c || !counts) return NDLQR_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  {
    const hipError_t se = sync_all(c);
    if (se != hipSuccess) { c->state_dirty = true; return fail("hipStreamSynchronize", se); }
  }
  HIP_TRY(hipMemcpy(counts, c->info.get(), sizeof(int) * (size_t)c->d.batch, hipMemcpyDeviceToHost));
  return NDLQR_OK;
}

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
int download_packed(NdlqrHipCtx* c, const double* zsrc, int p0, int count, double* soln) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  HIP_TRY(s.ensure_xfer(c->du));
  const size_t nvars = (size_t)c->du.rows * c->du.N - c->du.m, pitch = (size_t)d.rows * d.N;
  hipStream_t st = s.stream;
  HIP_TRY(launch_pack(c->du, d, KnotSlice(), zsrc + p0 * pitch, s.xfer, st, count));
  // the reduced variables -> the caller's, in the staging (a constrained solve's solution is in the caller's already)
  // (... and so is w of a constrained adjoint)
  const bool in_callers = (zsrc == c->set[c->latest].z && c->cost.mapped(c->soln_gen)) || (zsrc == c->adj.z && c->lin_adjoint_resident());
  if (c->cost.dense && !in_callers) HIP_TRY(cost_map_back(c, s.xfer, p0, count, st));
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

int ndlqr_hip_compact_level1(const NdlqrHipCtx* c) { return c && c->kept.rec1_compact ? 1 : 0; }

int ndlqr_hip_level1_paired(const NdlqrHipCtx* c) { return c && c->kept.level1_paired ? 1 : 0; }
int ndlqr_hip_bottom_lds16(const NdlqrHipCtx* c) { return c && c->kept.bottom_lds16 ? 1 : 0; }
int ndlqr_hip_top_chain(const NdlqrHipCtx* c) { return c && c->kept.top_chain ? 1 : 0; }

int ndlqr_hip_factors_valid(const NdlqrHipCtx* c) { return c && c->kept.fact_valid ? 1 : 0; }

int ndlqr_hip_pack_solutions_device(NdlqrHipCtx* c, double* dst) {
  if (!c || !dst) return NDLQR_ERR_INVALID;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, "ndlqr_hip_pack_solutions_device");
  const ndlqr::Dims& d = c->d;
  HIP_TRY(hipSetDevice(c->device));
  // on the stream of the latest solve: ordered behind it, asynchronous for the caller
  HIP_TRY(launch_pack(c->du, d, KnotSlice(), c->set[c->latest].z, dst, c->set[c->latest].stream, d.batch));
  if (c->cost.dense && !c->cost.mapped(c->soln_gen)) HIP_TRY(cost_map_back(c, dst, 0, d.batch, c->set[c->latest].stream));
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
