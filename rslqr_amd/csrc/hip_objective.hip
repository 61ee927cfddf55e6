// hip_objective.hip -- the objective value of every problem at its resident solution, and its stage costs
// (ndlqr_hip_objective): the host side, the kernels of kernels_objective.hpp.
#include "hip_host.hpp"
#include "kernels_objective.hpp"

int ndlqr_hip_objective_constants(int* out2) {
  if (!out2) return NDLQR_ERR_INVALID;
  out2[0] = ndlqr::kObjKnots;
  out2[1] = ndlqr::kObjThreads;
  return NDLQR_OK;
}

// A read-out: nothing of the solver's state moves but the device time of the last call. Which form serves which state:
//   z in the caller's variables of a constrained-mode problem (cost.mapped: a constrained solve or its polish)
//       -> objective_dense on the retained Q, H, R, q, r of LinState;
//   everything else -> objective_diag on QR and the right-hand side of the set that holds the solution: the caller's
//       diagonal problem (after a box-constrained solve or polish QR is the unshifted one again), or the unit-cost
//       reduction of a dense-cost problem with z in its reduced variables -- in constrained mode too, where every entry
//       point leaves the plain, unshifted reduction resident (ShiftedReduction::close).
int ndlqr_hip_objective(NdlqrHipCtx* c, double* J, double* stage) {
  static const char* const who = "ndlqr_hip_objective";
  if (!c) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  if (!J) return refuse(std::string(who) + ": J is null");
  if (c->kept.time_shard) return refuse(std::string(who) + ": not available on a time-axis shard");
  if (c->soln_gen == 0) return refuse(std::string(who) + ": there is no resident solution yet; run a solve first");
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  const bool mapped = c->cost.mapped(c->soln_gen);
  if (mapped && !c->lin.active)
    return refuse(std::string(who) + ": the resident solution is that of a constrained-mode problem that has been replaced; "
                                     "run a solve first");
  const size_t lds = sizeof(double) * (mapped ? ndlqr::objective_dense_lds(u.w) : ndlqr::objective_diag_lds(u.w));
  if (lds > kLdsMax)
    return refuse(std::string(who) + ": " + (mapped ? "objective_dense" : "objective_diag") + " needs " + std::to_string(lds) +
                  " bytes of LDS at (" + std::to_string(u.n) + "," + std::to_string(u.m) + "), beyond the " +
                  std::to_string(kLdsMax) + " bytes of a workgroup");
  HIP_TRY(hipSetDevice(c->device));
  const size_t kn = (size_t)u.batch * u.N;
  CallerArrays<2> ca = {{J, stage}, {(size_t)u.batch, kn}};
  int err = ca.classify(c, who, "an output lies");
  if (err) return err;
  // (a solve still in flight is completed as ndlqr_hip_synchronize completes it: its device time and failure count are
  //  taken before this call's events replace the set's)
  if (c->timing_pending) {
    err = ndlqr_hip_synchronize(c);
    if (err) return err;
  }
  HIP_TRY(sync_all(c));
  HIP_TRY(c->grad_stage.grow(ca.stage + 2 * kn));  // behind the staged outputs: the knots' partials, hi | lo
  double* part = ca.place(c);
  // the set that holds the latest solution holds the right-hand side that produced it: a step replaces the right-hand side
  // of its own set alone, and brings the parts it does not replace up to date before it solves (rhs_make_current)
  BufferSet& s = c->set[c->latest];
  const hipStream_t st = s.stream;
  const dim3 grid((u.N + ndlqr::kObjKnots - 1) / ndlqr::kObjKnots, u.batch);
  HIP_TRY(hipEventRecord(s.ev_start, st));
  if (mapped) {
    const LinState& k = c->lin;
    HIP_TRY(allow_dynamic_lds(&ndlqr::objective_dense, lds));
    hipLaunchKernelGGL(ndlqr::objective_dense, grid, dim3(ndlqr::kObjThreads), lds, st, u, d, (const double*)k.Q,
                       k.has_H ? (const double*)k.H : (const double*)nullptr, (const double*)k.R, (const double*)k.q,
                       (const double*)k.r, (const double*)s.z, part);
  } else {
    HIP_TRY(allow_dynamic_lds(&ndlqr::objective_diag, lds));
    hipLaunchKernelGGL(ndlqr::objective_diag, grid, dim3(ndlqr::kObjThreads), lds, st, u, d, (const double*)c->QR,
                       (const double*)s.rhs, (const double*)s.z, part);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ndlqr::objective_finish, dim3(u.batch), dim3(64), 0, st, u.N, (const double*)part, ca.dev[0], ca.dev[1]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = ca.copy(st, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(st));
  note_elapsed(c, s);
  return NDLQR_OK;
}
