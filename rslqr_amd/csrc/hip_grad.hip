// hip_grad.hip -- adjoint solve and parameter gradients (ndlqr_hip_solve_adjoint, ndlqr_hip_download_adjoint,
// ndlqr_hip_gradients): the host side, the kernels of kernels_grad.hpp.
#include "hip_host.hpp"
#include "kernels_grad.hpp"

// the caller's packed g [batch][nvars] (this device's memory) into the adjoint's resident right-hand side
hipError_t launch_adjoint_rhs(NdlqrHipCtx* c, const double* g, hipStream_t st) {
  hipLaunchKernelGGL(ndlqr::adjoint_rhs_generic, dim3(c->d.N, c->d.batch), dim3(64), 0, st, c->du, c->d, g, c->adj.rhs.get());
  return hipGetLastError();
}

int ndlqr_hip_solve_adjoint(NdlqrHipCtx* c, const double* g) {
  if (!c || !g) return NDLQR_ERR_INVALID;
  if (c->lin.soln_gen != 0 && c->lin.soln_gen == c->soln_gen)
    return refuse("ndlqr_hip_solve_adjoint: the resident solution is that of a solve with linear inequality constraints "
                  "(ndlqr_hip_solve_constrained), whose adjoint is ndlqr_hip_solve_constrained_adjoint; a plain solve gives "
                  "the unconstrained one");
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
    HIP_TRY(cost_reduce_vector(c, c->cost.stage, st));
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
  HIP_TRY(launch_adjoint_rhs(c, ga.dev[0], s.stream));
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
  c->adj.rhs_stamp = c->rhs_stamp();
  return NDLQR_OK;
}

int ndlqr_hip_download_adjoint(NdlqrHipCtx* c, double* w) {
  if (!c || !w) return NDLQR_ERR_INVALID;
  // (w of a constrained adjoint: the scope of the shifted reduction repacked the inputs, which is no replacement)
  const bool lin_adj = c->lin_adjoint_resident() && !c->z_partial && !c->z_invalid;
  const int aerr = lin_adj ? NDLQR_OK : need_adjoint(c, "ndlqr_hip_download_adjoint");
  if (aerr) return aerr;
  HIP_TRY(hipSetDevice(c->device));
  const Where ww = where(w, c->device);
  if (ww == Where::OtherDevice) return refuse("ndlqr_hip_download_adjoint: w lies in the memory of another device than the solver's");
  if (ww != Where::OwnDevice) return download_packed(c, c->adj.z, 0, c->d.batch, w);
  const BufferSet& s = c->set[0];
  HIP_TRY(sync_all(c));
  HIP_TRY(launch_pack(c->du, c->d, KnotSlice(), c->adj.z, w, s.stream, c->d.batch));
  if (c->cost.dense && !lin_adj) HIP_TRY(cost_map_back(c, w, 0, c->d.batch, s.stream));
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
