// hip_lin_polish.hip -- the active-set polish of the solve with linear inequality constraints
// (ndlqr_hip_polish_constrained, ndlqr_hip_download_constraint_polish_codes and the two read-outs for the tests;
// DESIGN.md section 3.23): the host side, the kernels of kernels_lin_polish.hpp.
//
// The active rows are read off the latest constrained solve; per round the costs are shifted by sigma_p on those rows
// (lin_polish_shift_cost into LinState's Qs, Hs, Rs), reduced (cost_reduce_problem into LinState's records, A~, B~), put
// in force inside a ShiftedReduction scope and factored by factor_resident; then up to max_steps steps of
//     lin_polish_residual -> lin_polish_apply_t -> re-solve -> lin_polish_update,
// the validation of every problem's last accepted iterate, and -- while a set changed and rounds remain -- the corrected
// sets shifted, reduced and factored again. Nothing is read back between the launches of a step; one word per step tells
// whether a problem still runs, two words per round whether a set changed. The polish uses LinState's shifted-cost,
// record and reduced-problem buffers: the ADMM's factorisation is dropped.
#include "hip_lin_host.hpp"
#include "kernels_lin_polish.hpp"

static size_t lin_polish_residual_bytes(const ndlqr::Dims& u, int p) {
  return sizeof(double) * ndlqr::lin_polish_residual_lds(u.n, u.m, p);
}
static size_t lin_polish_wave_bytes(const ndlqr::Dims& u, int p) { return sizeof(double) * ndlqr::lin_polish_wave_lds(u.n, u.m, p); }

// the residual of (z, mu) under the current codes into lin_pol.r, rc and slot `slot` of the norms (norms may be null)
static int launch_lin_polish_residual(NdlqrHipCtx* c, hipStream_t st, const double* z, const double* mu, const int* state,
                                      unsigned long long* norms, int nslots, int slot) {
  const ndlqr::Dims& u = c->du;
  const ndlqr::Dims& d = c->d;
  const LinState& k = c->lin;
  LinPolishState& lp = c->lin_pol;
  const size_t lds = lin_polish_residual_bytes(u, k.p);
  HIP_TRY(allow_lin_lds(ndlqr::lin_polish_residual, lds, lp.lds_asked[1]));
  hipLaunchKernelGGL(ndlqr::lin_polish_residual, dim3(d.N, d.batch), dim3(64), lds, st, u, d, k.p, (const double*)lp.sig,
                     (const double*)k.A, (const double*)k.B, (const double*)k.Q, k.has_H ? (const double*)k.H : nullptr,
                     (const double*)k.R, (const double*)k.q, (const double*)k.r, (const double*)k.d, (const double*)k.x0,
                     (const double*)k.C, (const double*)k.D, (const double*)k.lo, (const double*)k.hi, k.bstride,
                     (const unsigned char*)lp.code, z, mu, state, lp.r.get(), lp.rc.get(), norms, nslots, slot);
  HIP_TRY(hipGetLastError());
  return NDLQR_OK;
}

// per-phase device times of a polish under NDLQR_FLAG_PROFILE (ndlqr_hip_constraint_polish_phase_ms): 0 the residual, 1 S^'
// and the re-solve, 2 the update
struct LinPolishPhases {
  NdlqrHipCtx* c;
  bool on;
  struct Span { int phase; hipEvent_t start, stop; };
  std::vector<Span> spans;
  explicit LinPolishPhases(NdlqrHipCtx* ctx) : c(ctx), on((ctx->flags & NDLQR_FLAG_PROFILE) != 0) {}
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
    LinPolishState& lp = c->lin_pol;
    for (int p = 0; p < 3; ++p) { lp.phase_ms[p] = 0.0; lp.phase_spans[p] = 0; }
    for (const Span& sp : spans) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, sp.start, sp.stop) == hipSuccess) lp.phase_ms[sp.phase] += ms;
      ++lp.phase_spans[sp.phase];
      c->event_pool.push_back(sp.start);
      c->event_pool.push_back(sp.stop);
    }
    spans.clear();
  }
};

// the steps of one round on the current factorisation
static int lin_polish_steps(NdlqrHipCtx* c, hipStream_t st, bool strict, int max_steps, LinPolishPhases& phases) {
  const ndlqr::Dims& u = c->du;
  const ndlqr::Dims& d = c->d;
  const LinState& k = c->lin;
  LinPolishState& lp = c->lin_pol;
  const int nslots = max_steps + 1, p = k.p;
  const size_t wlds = lin_polish_wave_bytes(u, p);
  HIP_TRY(allow_lin_lds(ndlqr::lin_polish_apply_t, wlds, lp.lds_asked[2]));
  if (strict) HIP_TRY(allow_lin_lds(ndlqr::lin_polish_update<true>, 4 * wlds, lp.lds_asked[3]));
  else HIP_TRY(allow_lin_lds(ndlqr::lin_polish_update<false>, 4 * wlds, lp.lds_asked[4]));
  HIP_TRY(hipMemsetAsync(lp.norms, 0, sizeof(unsigned long long) * LinPolishState::norm_count(d), st));
  phases.open(0);
  int e = launch_lin_polish_residual(c, st, lp.z, lp.mu, lp.state, lp.norms, nslots, 0);
  phases.close();
  if (e) return e;
  for (int step = 1; step <= max_steps + 1; ++step) {
    const int form = step <= max_steps;
    if (form) {
      phases.open(1);
      hipLaunchKernelGGL(ndlqr::lin_polish_apply_t, dim3(d.N, d.batch), dim3(64), wlds, st, u, d, p, (const double*)k.rec,
                         (const double*)lp.r, (const int*)lp.state, lp.rt.get());
      HIP_TRY(hipGetLastError());
      e = launch_resolve(c, lp.rt, lp.delta, "constrained polish: this configuration needs NDLQR_FLAG_KEEP_FACT");
      phases.close();
      if (e) return e;
    }
    phases.open(2);
    launch_strict(strict, ndlqr::lin_polish_update, dim3(d.batch), dim3(256), 4 * wlds, st, u, d, p, step, form,
                  (const unsigned long long*)lp.norms, (const double*)lp.sig, (const double*)k.rec, (const double*)k.C,
                  (const double*)k.D, (const unsigned char*)lp.code, (const double*)lp.rc, (const double*)lp.delta, lp.z.get(),
                  lp.mu.get(), lp.zc.get(), lp.muc.get(), lp.state.get(), lp.here.get(), lp.word.get());
    phases.close();
    HIP_TRY(hipGetLastError());
    if (!form) break;
    phases.open(0);
    e = launch_lin_polish_residual(c, st, lp.zc, lp.muc, lp.state, lp.norms, nslots, step);
    phases.close();
    if (e) return e;
    if (step >= 2) {  // one word: how many problems still run
      HIP_TRY(hipMemcpyAsync(lp.h_word, lp.word, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (lp.h_word[0] == 0) break;
    }
  }
  return NDLQR_OK;
}

// what the kernels of the polish stage per workgroup, refused by name beyond the LDS of one
static int refuse_lin_polish_lds(const NdlqrHipCtx* c, const char* who) {
  const ndlqr::Dims& u = c->du;
  const int p = c->lin.p;
  const size_t rbytes = lin_polish_residual_bytes(u, p) + 16, ubytes = 4 * lin_polish_wave_bytes(u, p) + sizeof(double) * 256 + 16;
  const char* const which = rbytes > kLdsMax ? "lin_polish_residual" : "lin_polish_update";
  const size_t bytes = rbytes > kLdsMax ? rbytes : ubytes;
  if (bytes <= kLdsMax) return NDLQR_OK;
  return refuse(std::string(who) + ": " + which + " stages " + std::to_string(bytes) + " bytes per workgroup at (" +
                std::to_string(u.n) + "," + std::to_string(u.m) + ") with " + std::to_string(p) + " rows, beyond the " +
                std::to_string(kLdsMax) + " bytes of LDS of a workgroup");
}

// is the resident solution that of the latest constrained solve, with its right-hand side and bounds?
static int need_lin_polish_start(const NdlqrHipCtx* c, const char* who) {
  if (const int merr = need_constrained(c, who)) return merr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  const LinState& k = c->lin;
  if (k.soln_gen == 0 || k.soln_gen != c->soln_gen || !k.have_vy || k.rhs_new)
    return refuse(std::string(who) + ": the resident solution is not that of the latest constrained solve "
                  "(ndlqr_hip_solve_constrained first; a solve, a polish, new inputs, a new right-hand side or new bounds came "
                  "after it)");
  if (k.kept.time_shard) return refuse(std::string(who) + ": not available on a time-axis shard");
  return refuse_lin_polish_lds(c, who);
}

int ndlqr_hip_polish_constrained(NdlqrHipCtx* c, double sigma, int max_steps, int max_rounds, int* steps, int* status) {
  if (!c || !(sigma > 0.0) || !(sigma < HUGE_VAL) || max_steps < 1 || max_steps > kPolishMaxSteps || max_rounds < 0)
    return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_polish_constrained";
  if (const int serr = need_lin_polish_start(c, who)) return serr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  LinState& k = c->lin;
  LinPolishState& lp = c->lin_pol;
  HIP_TRY(hipSetDevice(c->device));
  int err = refuse_foreign_iters_status(c, who, steps, status);
  if (err) return err;
  HIP_TRY(lp.ensure(u, d, k.p, c->set[0].stream));
  // 1. everything idle, the primary set current
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  const unsigned pol_flags = c->flags | (strict ? NDLQR_FLAG_KEEP_FACT : NDLQR_FLAG_KEEP_RECORDS);
  const int p = k.p;
  const double* Hk = k.has_H ? k.H.get() : nullptr;
  lp.soln_gen = 0;
  lp.rounds = 0;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  // 2. sigma_p, codes, the starting iterate (before the first factorisation overwrites the resident solution)
  hipLaunchKernelGGL(ndlqr::lin_polish_sigma, dim3(u.batch), dim3(256), 0, st, u, p, sigma, (const double*)k.Q, (const double*)k.R,
                     (const double*)k.C, (const double*)k.D, (const double*)k.lo, (const double*)k.hi, k.bstride, lp.sig.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(lp.word, 0, 2 * sizeof(int), st));
  hipLaunchKernelGGL(ndlqr::lin_polish_start, dim3(d.N, d.batch), dim3(64), 0, st, u, d, p, (const double*)k.rho, (const double*)k.lo,
                     (const double*)k.hi, k.bstride, (const double*)k.v, (const double*)k.y, (const int*)k.status,
                     (const double*)s.z, lp.z0.get(), lp.z.get(), lp.code.get(), lp.mu.get(), lp.state.get(), lp.steps.get(),
                     lp.here.get(), lp.word.get());
  HIP_TRY(hipGetLastError());
  bool factored = false;
  int not_spd = NDLQR_OK;
  LinPolishPhases phases(c);
  ShiftedReduction shifted(c);
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto rounds = [&]() -> int {
    const size_t slds = sizeof(double) * ndlqr::lin_shift_lds(u.n, u.m, p);
    HIP_TRY(allow_lin_lds(ndlqr::lin_polish_shift_cost, slds, lp.lds_asked[0]));
    for (int round = 0; round <= max_rounds; ++round) {
      // 3. the costs shifted by sigma_p on the active rows, reduced, put in force and factored
      hipLaunchKernelGGL(ndlqr::lin_polish_shift_cost, dim3(u.N, u.batch), dim3(64), slds, st, u.n, u.m, u.N, p,
                         (const double*)lp.sig, (const unsigned char*)lp.code, (const double*)k.Q, Hk, (const double*)k.R,
                         (const double*)k.C, (const double*)k.D, k.Qs.get(), k.Hs.get(), k.Rs.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(cost_reduce_problem(c, k.A, k.B, k.Qs, k.Hs, k.Rs, k.rec, k.At, k.Bt, st));
      int e = round == 0 ? shifted.open(pol_flags) : shifted.repack();
      if (e) return e;
      factored = true;
      ++lp.rounds;
      e = factor_resident(c, st, &not_spd, who, "the reduction of Q + sigma C_A'C_A, H + sigma C_A'D_A, R + sigma D_A'D_A");
      if (e) return e;
      // 4. the steps
      // (word[0]: the problems that run in this round, counted by lin_polish_start / the previous round's validation)
      e = lin_polish_steps(c, st, strict, max_steps, phases);
      if (e) return e;
      // 5. validation; the sets that changed
      HIP_TRY(hipMemsetAsync(lp.word, 0, 2 * sizeof(int), st));
      hipLaunchKernelGGL(ndlqr::lin_polish_validate, dim3(u.batch), dim3(256), 0, st, u, d, p, round == max_rounds ? 1 : 0,
                         (const double*)k.C, (const double*)k.D, (const double*)k.lo, (const double*)k.hi, k.bstride,
                         lp.code.get(), (const double*)lp.z, lp.mu.get(), lp.state.get(), lp.steps.get(), lp.here.get(),
                         lp.word.get());
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(lp.h_word, lp.word, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (lp.h_word[1] == 0) break;
    }
    // 6. deliver
    hipLaunchKernelGGL(ndlqr::lin_polish_finish, dim3(d.N, d.batch), dim3(64), 0, st, u, d, p, (const double*)k.rho,
                       (const int*)lp.state, (const unsigned char*)lp.code, (const double*)k.C, (const double*)k.D,
                       (const double*)k.lo, (const double*)k.hi, k.bstride, (const double*)lp.z, (const double*)lp.mu,
                       (const double*)lp.z0, s.z.get(), k.v.get(), k.y.get());
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = rounds();
  // 7. the plain reduced problem again, bookkeeping
  const int cerr = shifted.close();
  if (!err) err = cerr;
  c->forget_shifted();  // (the shifted records and the reduced problem are the polish's now: nothing of the ADMM's is remembered)
  if (err) {
    if (not_spd) {
      // (a non-positive pivot leaves the device state clean: the solutions as the constrained solve left them)
      if (hipMemcpyAsync(s.z, lp.z0, sizeof(double) * doubles_z(d), hipMemcpyDeviceToDevice, st) != hipSuccess) c->z_invalid = true;
    } else {
      c->state_dirty = true;              // (a failed launch)
      if (factored) c->z_invalid = true;  // (the factorisation overwrote the resident solution)
    }
    (void)hipStreamSynchronize(st);
    return err;
  }
  note_solution(c);  // (lin_polish_finish wrote the resident solution: whatever belonged to the ADMM solution no longer applies)
  c->cost.mapped_gen = c->soln_gen;  // (in the caller's variables already: the delivery must not apply the plain records to it)
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = deliver_iters_status(c, st, lp.steps, lp.state, steps, status);
  phases.collect();
  if (err) return err;  // (nothing remembered: the caller never learnt which problems were polished)
  note_elapsed(c, s);
  lp.soln_gen = c->soln_gen;
  return NDLQR_OK;
}

// under NDLQR_FLAG_PROFILE: device time of the latest polish's residuals | S^' + re-solves | updates, and how many of each
// it added up
int ndlqr_hip_constraint_polish_phase_ms(NdlqrHipCtx* c, double* out3, int* launches3) {
  if (!c || !out3) return NDLQR_ERR_INVALID;
  for (int p = 0; p < 3; ++p) {
    out3[p] = c->lin_pol.phase_ms[p];
    if (launches3) launches3[p] = c->lin_pol.phase_spans[p];
  }
  return NDLQR_OK;
}

hipError_t launch_lin_polish_multipliers(NdlqrHipCtx* c, double* out, hipStream_t st) {
  const LinState& k = c->lin;
  const LinPolishState& lp = c->lin_pol;
  const int per = c->du.N * k.p;
  hipLaunchKernelGGL(ndlqr::lin_polish_multipliers, dim3((per + 255) / 256, c->du.batch), dim3(256), 0, st, per,
                     (const double*)k.rho, (const double*)k.y, (const int*)lp.state, (const double*)lp.mu, out);
  return hipGetLastError();
}

static int need_lin_polished(const NdlqrHipCtx* c, const char* who) {
  if (const int merr = need_constrained(c, who)) return merr;
  if (!c->lin_polished()) return refuse(std::string(who) + ": the resident solution is not that of a constrained polish");
  return NDLQR_OK;
}

// the row codes [batch][N][p] bytes of the latest polish, into host memory or this device's
int ndlqr_hip_download_constraint_polish_codes(NdlqrHipCtx* c, unsigned char* codes) {
  if (!c || !codes) return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_download_constraint_polish_codes";
  if (const int perr = need_lin_polished(c, who)) return perr;
  HIP_TRY(hipSetDevice(c->device));
  if (where(codes, c->device) == Where::OtherDevice)
    return refuse(std::string(who) + ": the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(codes, c->lin_pol.code, (size_t)c->du.batch * c->du.N * c->lin.p, hipMemcpyDefault));
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ read-outs for the tests (HOST memory)
// packed [batch][nvars] vectors in [lambda x u] order <-> the device layout [batch][d.N][2 d.n + d.m]
static void lin_polish_unpack(const ndlqr::Dims& u, const ndlqr::Dims& d, const double* packed, std::vector<double>& dev) {
  const size_t nvars = (size_t)u.rows * u.N - u.m;
  for (int b = 0; b < u.batch; ++b)
    for (int k = 0; k < u.N; ++k)
      for (int r = 0; r < u.rows; ++r) {
        if (k == u.N - 1 && r >= 2 * u.n) break;
        const int blk = r < u.n ? 0 : (r < 2 * u.n ? 1 : 2), i = r - blk * u.n;
        dev[((size_t)b * d.N + k) * d.rows + (size_t)blk * d.n + i] = packed[b * nvars + (size_t)k * u.rows + r];
      }
}
static void lin_polish_pack(const ndlqr::Dims& u, const ndlqr::Dims& d, const std::vector<double>& dev, double* packed) {
  const size_t nvars = (size_t)u.rows * u.N - u.m;
  for (int b = 0; b < u.batch; ++b)
    for (int k = 0; k < u.N; ++k)
      for (int r = 0; r < u.rows; ++r) {
        if (k == u.N - 1 && r >= 2 * u.n) break;
        const int blk = r < u.n ? 0 : (r < 2 * u.n ? 1 : 2), i = r - blk * u.n;
        packed[b * nvars + (size_t)k * u.rows + r] = dev[((size_t)b * d.N + k) * d.rows + (size_t)blk * d.n + i];
      }
}

// lin_polish_residual alone, on given z [batch][nvars] (packed, the caller's variables), mu [batch][N][p], codes
// [batch][N][p] bytes and sigma_p [batch]: r [batch][nvars] gets the right-hand side of the correction, rc [batch][N][p]
// the constraint residual, norms [2][batch] the two maxima (any of the three may be null). poison_pad != 0: the pad
// entries and the pad knots of the device's z hold NaN instead of zero -- nothing of them may reach an output. The polish
// state is scratch: whatever a polish left there is overwritten (its solution generation is dropped).
int ndlqr_hip_constraint_polish_residual(NdlqrHipCtx* c, const double* z, const double* mu, const unsigned char* codes,
                                         const double* sig, int poison_pad, double* r, double* rc, double* norms) {
  if (!c || !z || !mu || !codes || !sig) return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_constraint_polish_residual";
  if (const int merr = need_constrained(c, who)) return merr;
  if (const int lerr = refuse_lin_polish_lds(c, who)) return lerr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  const LinState& k = c->lin;
  LinPolishState& lp = c->lin_pol;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(lp.ensure(u, d, k.p, c->set[0].stream));
  HIP_TRY(sync_all(c));
  lp.soln_gen = 0;
  const hipStream_t st = c->set[0].stream;
  const size_t np = (size_t)u.batch * u.N * k.p, nz = doubles_z(d), nb = (size_t)u.batch;
  std::vector<double> dev(nz, poison_pad ? (double)NAN : 0.0);
  lin_polish_unpack(u, d, z, dev);
  HIP_TRY(hipMemcpyAsync(lp.z, dev.data(), sizeof(double) * nz, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(lp.mu, mu, sizeof(double) * np, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(lp.code, codes, np, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(lp.sig, sig, sizeof(double) * nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(lp.norms, 0, sizeof(unsigned long long) * LinPolishState::norm_count(d), st));
  if (const int e = launch_lin_polish_residual(c, st, lp.z, lp.mu, nullptr, lp.norms, 1, 0)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  if (r) {
    HIP_TRY(hipMemcpy(dev.data(), lp.r, sizeof(double) * nz, hipMemcpyDeviceToHost));
    lin_polish_pack(u, d, dev, r);
  }
  if (rc) HIP_TRY(hipMemcpy(rc, lp.rc, sizeof(double) * np, hipMemcpyDeviceToHost));
  if (norms) HIP_TRY(hipMemcpy(norms, lp.norms, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost));
  return NDLQR_OK;
}

// What the latest polish left beside its solution: the candidate zc [batch][nvars] (packed) and muc [batch][N][p] of its
// last formed step, the norm slots of its last round [2][33][batch] as doubles, sigma_p [batch] and the number of its
// factorisations; any pointer may be null.
int ndlqr_hip_download_constraint_polish_state(NdlqrHipCtx* c, double* zc, double* muc, double* norms, double* sig, int* rounds) {
  if (!c) return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_download_constraint_polish_state";
  if (const int perr = need_lin_polished(c, who)) return perr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  const LinPolishState& lp = c->lin_pol;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  const size_t np = (size_t)u.batch * u.N * c->lin.p, nz = doubles_z(d), nb = (size_t)u.batch;
  if (zc) {
    std::vector<double> dev(nz);
    HIP_TRY(hipMemcpy(dev.data(), lp.zc, sizeof(double) * nz, hipMemcpyDeviceToHost));
    lin_polish_pack(u, d, dev, zc);
  }
  if (muc) HIP_TRY(hipMemcpy(muc, lp.muc, sizeof(double) * np, hipMemcpyDeviceToHost));
  if (norms) HIP_TRY(hipMemcpy(norms, lp.norms, sizeof(double) * LinPolishState::norm_count(d), hipMemcpyDeviceToHost));
  if (sig) HIP_TRY(hipMemcpy(sig, lp.sig, sizeof(double) * nb, hipMemcpyDeviceToHost));
  if (rounds) *rounds = lp.rounds;
  return NDLQR_OK;
}
