// hip_refine.hip -- iterative refinement with a double-double residual (ndlqr_hip_refine,
// ndlqr_hip_kkt_residual_vector): the host side, the kernels of kernels_refine.hpp.
#include "hip_host.hpp"
#include "kernels_refine.hpp"

// ------------------------------------------------------------------------------ iterative refinement
// ndlqr_hip_refine (kernels_refine.hpp): the residual of the resident solution (which == 0) or of the
// latest plain adjoint (which == 1) in double-double, then max_steps times: the re-solve of that residual against the kept
// factorisation into delta (record columns / slots saved and restored around it, as for the adjoint solve), the residual of
// z (+) delta over the old one, and the commit for the problems whose residual norm went down at every step so far. The
// host reads nothing back between the steps: acceptance is decided on the device from the norm slots.

// r = b - K (z (+) delta) into c->ref.r on the current set's stream (norms == nullptr: the vector alone)
// (QR: the diagonal to use -- the polish passes the saved, unshifted one --, r: the destination)
int launch_residual_dd_on(NdlqrHipCtx* c, const double* QR, const double* rhs, const double* z, const double* delta,
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
