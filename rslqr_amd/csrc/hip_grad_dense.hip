// hip_grad_dense.hip -- parameter gradients of dense-cost and constrained batch solves (ndlqr_hip_gradients_dense;
// DESIGN.md section 3.21): the host side, the kernels of kernels_grad_dense.hpp.
#include "hip_host.hpp"
#include "kernels_grad_dense.hpp"

int ndlqr_hip_gradients_dense(NdlqrHipCtx* c, unsigned sum_mask, double* gA, double* gB, double* gQ, double* gH, double* gR,
                              double* gq, double* gr, double* gd, double* gx0) {
  static const char* const who = "ndlqr_hip_gradients_dense";
  if (!c) return NDLQR_ERR_INVALID;
  if (sum_mask & ~0x1FFu) return refuse(std::string(who) + ": sum_mask has bits beyond the nine outputs (NDLQR_GRADD_*)");
  if (!c->cost.dense)
    return refuse(std::string(who) + ": the solver is not in dense-cost mode; the gradients of a diagonal-cost solve are "
                                     "ndlqr_BatchGradients'");
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  // Which adjoint: the resident solution of a constrained solve is in the caller's variables (cost.mapped) and so is w of
  // its constrained adjoint; everything else is a plain solve's, both in the reduced variables.
  const bool lin_soln = c->cost.mapped(c->soln_gen);
  if (lin_soln) {
    if (!c->lin_adjoint_resident())
      return refuse(std::string(who) + ": no constrained adjoint of the resident constrained solution "
                                       "(ndlqr_hip_solve_constrained_adjoint after the latest constrained solve, right-hand "
                                       "side and bounds)");
  } else if (const int aerr = need_adjoint(c, who)) {
    return aerr;
  }
  if (c->adj.rhs_stamp != c->rhs_stamp())
    return refuse(std::string(who) + ": the right-hand side was replaced after the adjoint solve; the resident solution "
                                     "and adjoint are not those of the resident inputs (solve and take the adjoint again)");
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  const int n = u.n, m = u.m, N = u.N, batch = u.batch;
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<ndlqr::GRADD_COUNT> ga = {{gA, gB, gQ, gH, gR, gq, gr, gd, gx0}, {}};
  double* const* user = ga.user;
  size_t total = 0;
  ndlqr::GradDenseOut out = {};
  int wsum = 0;
  for (int o = 0; o < ndlqr::GRADD_COUNT; ++o) {
    if (!user[o]) continue;
    const bool summed = (sum_mask >> o) & 1u;
    const int W = ndlqr::grad_dense_width(n, m, o);
    const size_t per = o == ndlqr::GRADD_x0 ? (size_t)n : (size_t)N * W;
    ga.cnt[o] = summed ? per : per * batch;
    if (summed) { out.off[o] = total; total += per; wsum += W; }
  }
  int err = ga.classify(c, who, "an output lies");
  if (err) return err;
  out.sum = sum_mask;
  out.total = total;
  // The chunk of knots per workgroup, the slices of its accumulators and the split of the batch: the rules of
  // ndlqr_hip_gradients, on the packed run of a chunk -- KC (2n+m) + n doubles of z and of w.
  int KC = ndlqr::kGradDenseChunk;
  while (KC > 1 && (KC > N || sizeof(double) * ((size_t)KC * wsum + 2 * ((size_t)KC * u.rows + n)) > 48 * 1024)) KC >>= 1;
  const size_t lds_max = kLdsMax / sizeof(double), zw = 2 * ((size_t)KC * u.rows + n), nacc = (size_t)KC * wsum;
  if (zw >= lds_max) return refuse(std::string(who) + ": z and w of two knots of this block size exceed the LDS of a workgroup");
  int nslice = (int)((nacc + (lds_max - zw) - 1) / (lds_max - zw));
  if (nslice < 1) nslice = 1;
  const size_t EC = (nacc + nslice - 1) / nslice;
  const size_t lds = sizeof(double) * (EC + zw);
  const int nchunks = (N + KC - 1) / KC;
  int ppb = 1, nsplit = batch;
  if (total > 0) {
    nsplit = ndlqr::kGradDenseWorkgroups / (nchunks * nslice);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > batch) nsplit = batch;
    while (nsplit > 1 && (size_t)nsplit * total > ((size_t)64 << 20)) nsplit >>= 1;  // partial sums within 512 MB
    ppb = (batch + nsplit - 1) / nsplit;
    nsplit = (batch + ppb - 1) / ppb;
  }
  const size_t npart = nsplit > 1 ? (size_t)nsplit * total : 0;
  const size_t nvars = (size_t)u.rows * N - m, npack = nvars * batch;
  HIP_TRY(c->grad_stage.grow(ga.stage + npart + 2 * npack));
  HIP_TRY(sync_all(c));
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  double* part = ga.place(c);  // (the partial sums behind the staged outputs, the packed z | w behind those)
  double* zp = part + npart;
  double* wp = zp + npack;
  if (!npart) part = nullptr;
  for (int o = 0; o < ndlqr::GRADD_COUNT; ++o) out.p[o] = ga.dev[o];
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  HIP_TRY(strict ? allow_dynamic_lds(&ndlqr::grad_assemble_dense<true>, lds)
                 : allow_dynamic_lds(&ndlqr::grad_assemble_dense<false>, lds));
  HIP_TRY(hipEventRecord(s.ev_start, st));
  // z and w as ndlqr_hip_download_solutions and ndlqr_hip_download_adjoint deliver them: packed copies, mapped to the
  // caller's variables where the resident vectors are in the reduced ones (those are never mapped in place)
  HIP_TRY(launch_pack(u, d, KnotSlice(), c->set[c->latest].z, zp, st, batch));
  if (!lin_soln) HIP_TRY(cost_map_back(c, zp, 0, batch, st));
  HIP_TRY(launch_pack(u, d, KnotSlice(), c->adj.z, wp, st, batch));
  if (!lin_soln) HIP_TRY(cost_map_back(c, wp, 0, batch, st));
  const int* skip = lin_soln ? c->alin.status.get() : nullptr;
  launch_strict(strict, ndlqr::grad_assemble_dense, dim3(nchunks, nsplit, nslice), dim3(256), lds, st, n, m, N, batch, KC, ppb,
                (int)EC, (const double*)zp, (const double*)wp, skip, out, part);
  HIP_TRY(hipGetLastError());
  if (part) {
    hipLaunchKernelGGL(ndlqr::grad_dense_sum_splits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, nsplit,
                       (const double*)part);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = ga.copy(st, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(st));
  note_elapsed(c, s);
  return NDLQR_OK;
}

// the constants of the batch split, for the tests: [0] workgroups the split aims at, [1] knots per chunk at most
int ndlqr_hip_gradients_dense_constants(int* out2) {
  if (!out2) return NDLQR_ERR_INVALID;
  out2[0] = ndlqr::kGradDenseWorkgroups;
  out2[1] = ndlqr::kGradDenseChunk;
  return NDLQR_OK;
}
