// hip_cost.hip -- dense cost matrices and state-input cross terms (ndlqr_hip_init_dense): the
// host side of the reduction to a unit-cost problem, the kernels of kernels_cost.hpp.
#include "hip_host.hpp"
#include "kernels_cost.hpp"

// ------------------------------------------------------------------------------ dense cost matrices
// Layered ABOVE the plain entry points: the dense-cost problem is reduced on the device to a unit-cost problem of the same
// shape (kernels_cost.hpp), whose flat arrays -- device-resident, in the caller's layout -- go to ndlqr_hip_pack_flat_device
// and the right-hand-side pack kernel like any caller's. The solve kernels, their schedules and captured graphs never
// learn of it; solutions and adjoints are mapped back where they are packed for the caller (cost_map_back).

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
hipError_t cost_map_back(NdlqrHipCtx* c, double* vec, int p0, unsigned count, hipStream_t st) {
  CostPhase phase(c, st, 2);
  const hipError_t e = cost_apply_on(c, vec, p0, count, st);
  phase.stop();
  return e;
}
// ... the launch alone, for the asynchronous step: no phase timing, nothing waits
hipError_t cost_apply_on(NdlqrHipCtx* c, double* vec, int p0, unsigned count, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  return launch_cost(ndlqr::cost_apply, ndlqr::cost_apply_lds(u.n, u.m), u, count, st, u.n, u.m, u.N,
                     c->cost.rec + (size_t)p0 * u.N * CostState::record_doubles(u), vec);
}
// The asynchronous step's way up: S' of the parts `parts` (bits q 1, r 2 -- together --, d 4, x0 8) of the caller's flat
// q, r, d, x0 (device-readable) straight into the device right-hand side `rhs` of one buffer set, on `st`. One knot per
// problem where x0 alone is replaced.
hipError_t cost_pack_rhs_on(NdlqrHipCtx* c, unsigned parts, const double* q, const double* r, const double* d, const double* x0,
                            double* rhs, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  const size_t lds = sizeof(double) * ndlqr::cost_apply_lds(u.n, u.m);
  const hipError_t e = allow_dynamic_lds(ndlqr::cost_pack_rhs, lds);
  if (e != hipSuccess) return e;
  const unsigned knots = (parts & 7u) ? (unsigned)u.N : 1u;
  hipLaunchKernelGGL(ndlqr::cost_pack_rhs, dim3(knots, u.batch), dim3(64), lds, st, u, c->d, parts, (const double*)c->cost.rec.get(),
                     q, r, d, x0, rhs);
  return hipGetLastError();
}
// ... and its way down: S of the slice `sel` (non-empty) of the reduced solutions z (device layout) into dst
// [batch][nknots][width] (this device's memory), on `st`
hipError_t cost_deliver_slice_on(NdlqrHipCtx* c, const KnotSlice& sel, const double* z, double* dst, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  const size_t lds = sizeof(double) * ndlqr::cost_apply_lds(u.n, u.m);
  const hipError_t e = allow_dynamic_lds(ndlqr::cost_deliver_slice, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ndlqr::cost_deliver_slice, dim3(sel.nknots, u.batch), dim3(64), lds, st, u, c->d, sel.knot0, sel.nknots,
                     sel.blocks & 7u, (const double*)c->cost.rec.get(), z, dst);
  return hipGetLastError();
}
// ... and the packed [batch][nvars] vector `vec` in the caller's variables becomes S' vec (in place): the adjoint's g
hipError_t cost_reduce_vector(NdlqrHipCtx* c, double* vec, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  return launch_cost(ndlqr::cost_apply_t, ndlqr::cost_apply_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, c->cost.rec.get(),
                     nullptr, nullptr, nullptr, nullptr, vec, nullptr, nullptr, nullptr, nullptr, vec);
}

// S' (records `rec`) of the flat right-hand side at q, r, d, x0 (device) into the flat arrays qt, rt, dt, x0t, on `st`
hipError_t cost_reduce_rhs_to(NdlqrHipCtx* c, const double* rec, const double* q, const double* r, const double* d,
                              const double* x0, double* qt, double* rt, double* dt, double* x0t, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  CostPhase phase(c, st, 1);
  const hipError_t e = launch_cost(ndlqr::cost_apply_t, ndlqr::cost_apply_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, rec, q, r,
                                   d, x0, nullptr, qt, rt, dt, x0t, nullptr);
  phase.stop();
  return e;
}
// ... into the reduced flat arrays of the plain problem
static hipError_t cost_reduce_rhs(NdlqrHipCtx* c, const double* q, const double* r, const double* d, const double* x0,
                                  hipStream_t st) {
  CostState& k = c->cost;
  return cost_reduce_rhs_to(c, k.rec, q, r, d, x0, k.qt, k.rt, k.dt, k.x0t, st);
}
// The reduction of the dense costs Q, H (null: zero), R and of A, B (device, the caller's flat layout): the records into
// `rec`, A~, B~ into At, Bt, on `st`
hipError_t cost_reduce_problem(NdlqrHipCtx* c, const double* A, const double* B, const double* Q, const double* H,
                               const double* R, double* rec, double* At, double* Bt, hipStream_t st) {
  const ndlqr::Dims& u = c->du;
  CostPhase phase(c, st, 0);
  hipError_t e = launch_cost(ndlqr::cost_factor, ndlqr::cost_factor_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, u.batch, Q, H, R,
                             rec, c->info.get());
  if (e == hipSuccess)
    e = launch_cost(ndlqr::cost_transform, ndlqr::cost_transform_lds(u.n, u.m), u, u.batch, st, u.n, u.m, u.N, A, B,
                    (const double*)rec, At, Bt);
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
  HIP_TRY(cost_reduce_problem(c, ca.dev[0], ca.dev[1], ca.dev[2], ca.dev[3], ca.dev[4], k.rec, k.At, k.Bt, st));
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
  if (c->lin.active) {  // constrained mode retains the caller's right-hand side: the shifted S' of the next constrained solve reads it
    double* const keep[4] = {c->lin.q, c->lin.r, c->lin.d, c->lin.x0};
    for (int i = 0; i < 4; ++i)
      HIP_TRY(hipMemcpyAsync(keep[i], ca.dev[i], sizeof(double) * ca.cnt[i], hipMemcpyDeviceToDevice, s.stream));
    c->lin.rhs_new = true;
  }
  const CostState& k = c->cost;
  HIP_TRY(launch_pack_rhs(c, k.qt, k.rt, k.dt, k.x0t));
  HIP_TRY(hipStreamSynchronize(s.stream));
  note_new_rhs(c);
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
