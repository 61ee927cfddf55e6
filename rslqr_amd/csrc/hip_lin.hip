// hip_lin.hip -- general linear inequality constraints lo <= C x + D u <= hi (ndlqr_hip_init_constrained,
// ndlqr_hip_set_constraint_bounds, ndlqr_hip_solve_constrained and their read-outs) and the
// gradients through that solve (ndlqr_hip_solve_constrained_adjoint, ndlqr_hip_constraint_gradients; section 3.18): the
// host side, the kernels of kernels_lin.hpp and kernels_lin_grad.hpp. The reduction kernels it needs belong to hip_cost.hip (cost_reduce_problem,
// cost_reduce_rhs_to). Infeasibility detection of that solve (ndlqr_hip_set_constraint_infeasibility and its two read-outs;
// section 3.20, kernels_lin_infeas.hpp) lives in its loop and at the end of this file.
#include "hip_lin_host.hpp"
#include "kernels_lin_grad.hpp"
#include "kernels_lin_infeas.hpp"

// ------------------------------------------------------------------------------ constrained mode
// A dense-cost mode with constraints: ndlqr_hip_init_constrained retains the caller's A, B, Q, H, R, q, r, d, x0 and C, D
// on the device and then runs ndlqr_hip_init_dense on the retained copies, so the plain API sees exactly what the dense
// initialiser leaves. A constrained solve shifts the retained costs by rho C'MC, rho C'MD, rho D'MD, reduces the shifted
// problem into buffers of its own (LinState: records, A~, B~, right-hand side), puts it in force (ShiftedReduction),
// factors it once and iterates: one re-solve into lin.z plus one lin_update per iteration; the host reads the running
// count every check_every iterations. On the way out the plain reduced problem of CostState is packed again.
// The penalty is a device vector, lin.rho [batch]. With ndlqr_hip_set_constraint_adaptation(every > 0) (DESIGN.md section
// 3.19) lin_update may move a problem's penalty at every every-th iteration; the host then reads the count of moved
// problems with the running count and, when it is not zero, shifts, reduces, packs and factors the whole batch again and
// lets lin_start rewrite the right-hand sides of the moved problems -- one factorisation serves every problem that moved
// in that round, and the deterministic kernels give every other problem its old records and factors back.
// Infeasibility detection (ndlqr_hip_set_constraint_infeasibility(every > 0)): the iteration before a
// check leaves lambda of its re-solve in the caller's variables (lin_lambda_out) and mu = rho y (lin_multipliers) behind
// lin_update and before any refactorisation; the check iteration forms its own lambda the same way and lin_certify judges
// the differences. A certified problem is frozen as status 4 and leaves the running count the host reads anyway. With
// every == 0 nothing of this is allocated, copied or launched.

static size_t lin_update_lds_bytes(const ndlqr::Dims& u, int p) { return sizeof(double) * 4 * ndlqr::lin_wave_lds(u.n, u.m, p); }

// Bounds lo, hi [P][N][p] of the caller (P = batch, or 1 when shared): checked (lo <= hi, no NaN) before anything is
// replaced; with `commit` then copied to the device and their bounded pattern compared with the one in force.
static int lin_take_bounds(NdlqrHipCtx* c, const char* who, const double* lo, const double* hi, int shared, bool commit) {
  const ndlqr::Dims& u = c->du;
  LinState& k = c->lin;
  const int P = shared ? 1 : u.batch;
  const size_t cnt = (size_t)P * u.N * k.p;
  CallerArrays<2> in = {{const_cast<double*>(lo), const_cast<double*>(hi)}, {cnt, cnt}};
  int err = in.classify(c, who, "bounds lie");
  if (err) return err;
  BufferSet& s = c->set[0];
  HIP_TRY(c->grad_stage.grow(in.stage));
  HIP_TRY(sync_all(c));
  in.place(c);
  err = in.copy(s.stream, true);
  if (err) return err;
  HIP_TRY(hipMemsetAsync(k.word, 0, 3 * sizeof(int), s.stream));
  for (int pass = 0; pass < (commit ? 2 : 1); ++pass) {
    hipLaunchKernelGGL(ndlqr::lin_bounds, dim3(u.N, P), dim3(64), 0, s.stream, u.N, k.p, (const double*)in.dev[0],
                       (const double*)in.dev[1], pass, k.lo.get(), k.hi.get(), k.mask.get(), k.word + 1, k.word + 2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(k.h_word, k.word, 3 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (k.h_word[1]) return refuse(std::string(who) + ": a lower bound exceeds its upper bound (or is NaN)");
  }
  if (!commit) return NDLQR_OK;
  // (the pattern lives in mask per problem: a change between shared and per-problem bounds always counts as a new one)
  if (k.h_word[2] || (shared != 0) != k.shared) k.fact = false;
  k.shared = shared != 0;
  k.bstride = shared ? 0 : (size_t)u.N * k.p;
  k.soln_gen = 0;
  c->alin.gen = 0;
  return NDLQR_OK;
}

int ndlqr_hip_init_constrained(NdlqrHipCtx* c, const double* A, const double* B, const double* Q, const double* H,
                               const double* R, const double* q, const double* r, const double* d, const double* x0, int p,
                               const double* C, const double* D, const double* lo, const double* hi, int shared) {
  if (!c) return NDLQR_ERR_INVALID;
  if (p < 1) return refuse("ndlqr_hip_init_constrained: p = " + std::to_string(p) + " rows per knot (p >= 1)");
  if (!A || !B || !Q || !R || !q || !r || !d || !x0 || !C || !D || !lo || !hi) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& u = c->du;
  const size_t lds = lin_update_lds_bytes(u, p) + sizeof(double) * 5 * 256 + 16;
  if (lds > kLdsMax)
    return refuse("ndlqr_hip_init_constrained: lin_update stages " + std::to_string(lds) + " bytes per workgroup at (" +
                  std::to_string(u.n) + "," + std::to_string(u.m) + ") with " + std::to_string(p) + " rows, beyond the " +
                  std::to_string(kLdsMax) + " bytes of LDS of a workgroup");
  HIP_TRY(hipSetDevice(c->device));
  const size_t kn = (size_t)u.batch * u.N, n = (size_t)u.n, m = (size_t)u.m;
  CallerArrays<11> ca = {{const_cast<double*>(A), const_cast<double*>(B), const_cast<double*>(Q), const_cast<double*>(H),
                          const_cast<double*>(R), const_cast<double*>(q), const_cast<double*>(r), const_cast<double*>(d),
                          const_cast<double*>(x0), const_cast<double*>(C), const_cast<double*>(D)},
                         {kn * n * n, kn * n * m, kn * n * n, kn * n * m, kn * m * m, kn * n, kn * m, kn * n, (size_t)u.batch * n,
                          kn * p * n, kn * p * m}};
  int err = ca.classify(c, "ndlqr_hip_init_constrained", "an input lies");
  if (err) return err;
  HIP_TRY(sync_all(c));  // solves in flight still read what is replaced here
  LinState& k = c->lin;
  const hipStream_t st = c->set[0].stream;
  // (from here on the retained state is being replaced: a refusal or failure below leaves constrained mode -- the plain
  //  dense-cost mode, if the context was in one, stays valid)
  k.active = false;
  k.fact = false;
  c->alin.gen = 0;
  HIP_TRY(k.ensure(u, c->d, p, st));
  err = lin_take_bounds(c, "ndlqr_hip_init_constrained", lo, hi, shared, false);
  if (err) return err;
  // the retained copies (host memory: straight into them; the caller's arrays are free again when this returns)
  double* const keep[11] = {k.A, k.B, k.Q, k.H, k.R, k.q, k.r, k.d, k.x0, k.C, k.D};
  for (int i = 0; i < 11; ++i)
    if (ca.user[i]) HIP_TRY(hipMemcpyAsync(keep[i], ca.user[i], sizeof(double) * ca.cnt[i], hipMemcpyDefault, st));
  HIP_TRY(hipStreamSynchronize(st));
  k.has_H = H != nullptr;
  k.fact = false;
  k.have_vy = false;
  k.rhs_new = true;
  k.soln_gen = 0;
  // the context enters dense-cost mode exactly as the dense initialiser leaves it
  err = ndlqr_hip_init_dense(c, k.A, k.B, k.Q, k.has_H ? k.H.get() : nullptr, k.R, k.q, k.r, k.d, k.x0);
  if (err) return err;
  HIP_TRY(hipMemsetAsync(k.mask, 0, kn * p, st));  // (no pattern in force: the first solve factors whatever the bounds are)
  err = lin_take_bounds(c, "ndlqr_hip_init_constrained", lo, hi, shared, true);
  if (err) return err;
  k.fact = false;
  k.active = true;
  return NDLQR_OK;
}

int ndlqr_hip_is_constrained(const NdlqrHipCtx* c) { return c && c->lin.active ? 1 : 0; }

int ndlqr_hip_set_constraint_bounds(NdlqrHipCtx* c, const double* lo, const double* hi, int shared) {
  if (!c || !lo || !hi) return NDLQR_ERR_INVALID;
  if (const int merr = need_constrained(c, "ndlqr_hip_set_constraint_bounds")) return merr;
  HIP_TRY(hipSetDevice(c->device));
  return lin_take_bounds(c, "ndlqr_hip_set_constraint_bounds", lo, hi, shared, true);
}

int ndlqr_hip_solve_constrained(NdlqrHipCtx* c, double rho, double alpha, double eps_abs, double eps_rel, int max_iter,
                                int check_every, int warm_start, int adapt_every, int* iters, int* status) {
  if (!c || adapt_every < 0 || !(rho > 0.0 && rho < HUGE_VAL) || !(alpha > 0.0 && alpha < 2.0) || !(eps_abs >= 0.0) || !(eps_rel >= 0.0) ||
      max_iter < 1 || check_every < 1)
    return NDLQR_ERR_INVALID;
  if (adapt_every > 0)
    return refuse("ndlqr_hip_solve_constrained: the adaptive penalty (adapt_every > 0) of the settings is the box solve's; "
                  "ndlqr_hip_set_constraint_adaptation (ndlqr_BatchSetConstraintPenaltyAdaptation) switches it on here");
  if (const int merr = need_constrained(c, "ndlqr_hip_solve_constrained")) return merr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  LinState& k = c->lin;
  HIP_TRY(hipSetDevice(c->device));
  int err = refuse_foreign_iters_status(c, "ndlqr_hip_solve_constrained", iters, status);
  if (err) return err;
  LinInfeasState& inf = c->lin_infeas;
  const int infeas_every = inf.every;
  const size_t lam_lds = sizeof(double) * ndlqr::lin_lambda_lds(u.n), cert_lds = ndlqr::lin_certify_lds_bytes(u, k.p);
  if (infeas_every > 0) {
    if (cert_lds + sizeof(double) * 5 * 256 + 16 > kLdsMax)
      return refuse("ndlqr_hip_solve_constrained: lin_certify stages " + std::to_string(cert_lds) + " bytes per workgroup at (" +
                    std::to_string(u.n) + "," + std::to_string(u.m) + ") with " + std::to_string(k.p) +
                    " rows, beyond the LDS of a workgroup (ndlqr_hip_set_constraint_infeasibility(0) switches detection off)");
    HIP_TRY(inf.ensure(u, k.p));
  }
  inf.gen = 0;
  // 1. everything idle, the primary set current
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  const bool strict = (c->flags & NDLQR_FLAG_STRICT_FP) != 0;
  const unsigned lin_flags = c->flags | (strict ? NDLQR_FLAG_KEEP_FACT : NDLQR_FLAG_KEEP_RECORDS);
  // the remembered factorisation applies to an adaptive warm start whatever its penalties are (the settings' rho is
  // ignored, as in the box solve); everywhere else only when they are all the settings' rho
  const int every = k.adapt_every;
  const bool usable = k.fact && k.flags == lin_flags;
  const bool keep_rho = usable && every > 0 && warm_start;
  const bool reuse = keep_rho || (usable && k.rho_uniform && k.rho_value == rho);
  bool uniform = keep_rho ? k.rho_uniform : true;
  const double uniform_value = keep_rho ? k.rho_value : rho;
  const int p = k.p;
  const size_t lds = lin_update_lds_bytes(u, p);
  HIP_TRY(hipEventRecord(s.ev_start, st));
  bool factored = false;
  int not_spd = NDLQR_OK;
  ShiftedReduction shifted(c);
  const double* Hk = k.has_H ? k.H.get() : nullptr;
  const double* rhov = k.rho;
  // the costs shifted by the penalties as they stand, and their reduction
  const auto shift_and_reduce = [&]() -> int {
    const size_t slds = sizeof(double) * ndlqr::lin_shift_lds(u.n, u.m, p);
    HIP_TRY(allow_lin_lds(ndlqr::lin_shift_cost, slds, k.lds_asked[0]));
    hipLaunchKernelGGL(ndlqr::lin_shift_cost, dim3(u.N, u.batch), dim3(64), slds, st, u.n, u.m, u.N, p, rhov,
                       (const double*)k.Q, Hk, (const double*)k.R, (const double*)k.C, (const double*)k.D, (const double*)k.lo,
                       (const double*)k.hi, k.bstride, k.Qs.get(), k.Hs.get(), k.Rs.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(cost_reduce_problem(c, k.A, k.B, k.Qs, k.Hs, k.Rs, k.rec, k.At, k.Bt, st));
    return NDLQR_OK;
  };
  const auto start = [&](int mode) -> int {
    hipLaunchKernelGGL(ndlqr::lin_start, dim3(u.batch), dim3(256), lds, st, u, d, p, mode, rhov, (const double*)k.rec,
                       (const double*)k.C, (const double*)k.D, (const double*)k.lo, (const double*)k.hi, k.bstride,
                       (const double*)s.rhs, (const int*)k.status, k.v.get(), k.y.get(), k.rhs[0].get(), k.rhs[1].get(),
                       k.moved.get());
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  const auto is_check = [&](int i) { return infeas_every > 0 && i >= 2 && i <= max_iter && i % infeas_every == 0; };
  const char* const what = "the reduction of Q + rho C'MC, H + rho C'MD, R + rho D'MD";
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto iterate = [&]() -> int {
    // 2. the penalties, the shifted costs and their reduction, unless the remembered ones apply; S^' of the right-hand
    // side when either is new
    if (!reuse) {
      hipLaunchKernelGGL(ndlqr::lin_fill_rho, dim3((u.batch + 255) / 256), dim3(256), 0, st, u.batch, rho, k.rho.get());
      HIP_TRY(hipGetLastError());
      if (const int se = shift_and_reduce()) return se;
    }
    if (!reuse || k.rhs_new) HIP_TRY(cost_reduce_rhs_to(c, k.rec, k.q, k.r, k.d, k.x0, k.qt, k.rt, k.dt, k.x0t, st));
    // 3. the shifted reduced problem in force; factored, unless the remembered factorisation applies
    int e = shifted.open(lin_flags);
    if (e) return e;
    if (reuse) {
      c->kept = k.kept;
    } else {
      factored = true;
      e = factor_resident(c, st, &not_spd, "ndlqr_hip_solve_constrained", what);
      if (e) return e;
    }
    // 4. the iterations
    const ndlqr::BoxParams P = {alpha, 1.0 - alpha, eps_abs, eps_rel, k.rho_min, k.rho_max};
    HIP_TRY(allow_lin_lds(ndlqr::lin_start, lds, k.lds_asked[1]));
    if (strict) HIP_TRY(allow_lin_lds(ndlqr::lin_update<true>, lds, k.lds_asked[2]));
    else HIP_TRY(allow_lin_lds(ndlqr::lin_update<false>, lds, k.lds_asked[3]));
    e = start(warm_start && k.have_vy ? ndlqr::LIN_START_WARM : ndlqr::LIN_START_COLD);
    if (e) return e;
    k.have_vy = true;
    k.h_word[0] = u.batch;
    k.h_word[1] = 0;
    HIP_TRY(hipMemcpyAsync(k.word, k.h_word, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(k.status, 0, sizeof(int) * (size_t)u.batch, st));
    HIP_TRY(hipMemsetAsync(k.moved, 0, sizeof(int) * (size_t)u.batch, st));
    const size_t nlam = (size_t)u.batch * u.N * u.n, nmu = (size_t)u.batch * u.N * p;
    if (infeas_every > 0) {  // (the certificate rows of the problems that do not end as 4 are zero)
      HIP_TRY(allow_lin_lds(ndlqr::lin_lambda_out, lam_lds, inf.lds_asked[0]));
      HIP_TRY(allow_lin_lds(ndlqr::lin_certify, cert_lds, inf.lds_asked[1]));
      for (DevBuf<double>* buf : {&inf.lam_prev, &inf.lam_cur, &inf.cert_lam}) HIP_TRY(hipMemsetAsync(*buf, 0, sizeof(double) * nlam, st));
      for (DevBuf<double>* buf : {&inf.mu_prev, &inf.cert_mu}) HIP_TRY(hipMemsetAsync(*buf, 0, sizeof(double) * nmu, st));
      HIP_TRY(hipMemsetAsync(inf.measures, 0, sizeof(double) * 4 * (size_t)u.batch, st));
      HIP_TRY(hipMemsetAsync(inf.measured_at, 0, sizeof(int) * (size_t)u.batch, st));
    }
    for (int it = 1; it <= max_iter; ++it) {
      const double* rc = k.rhs[(it - 1) & 1];
      double* rn = k.rhs[it & 1];
      e = launch_resolve(c, rc, k.z, "constrained solve: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
      const int adapt = every > 0 && it % every == 0 && it < max_iter;
      launch_strict(strict, ndlqr::lin_update, dim3(u.batch), dim3(256), lds, st, u, d, p, it, adapt, P, (const double*)k.z,
                    (const double*)k.rec, (const double*)k.C, (const double*)k.D, (const double*)k.lo, (const double*)k.hi,
                    k.bstride, k.v.get(), k.y.get(), (const double*)s.rhs, rc, rn, k.rho.get(), k.status.get(),
                    k.iters.get(), k.resid.get(), k.word.get(), k.moved.get());
      HIP_TRY(hipGetLastError());
      const bool check = is_check(it), before_check = is_check(it + 1);
      if (check || before_check) {
        // 4a. lambda of this re-solve in the caller's variables, under the records it used (a refactorisation comes later)
        hipLaunchKernelGGL(ndlqr::lin_lambda_out, dim3(u.N, u.batch), dim3(64), lam_lds, st, u, d, (const double*)k.rec,
                           (const double*)k.z, check ? inf.lam_cur.get() : inf.lam_prev.get());
        HIP_TRY(hipGetLastError());
      }
      if (check) {  // the differences over this iteration: a certificate?
        hipLaunchKernelGGL(ndlqr::lin_certify, dim3(u.batch), dim3(256), cert_lds, st, u, d, p, it, inf.eps, (const double*)k.A,
                           (const double*)k.B, (const double*)k.C, (const double*)k.D, (const double*)k.d, (const double*)k.x0,
                           (const double*)k.lo, (const double*)k.hi, k.bstride, (const double*)inf.lam_cur,
                           (const double*)inf.lam_prev, (const double*)k.y, (const double*)inf.mu_prev, (const double*)k.rho,
                           k.rhs[(it - 1) & 1].get(), (const double*)rn, k.status.get(), k.iters.get(), k.word.get(),
                           inf.cert_lam.get(), inf.cert_mu.get(), inf.measures.get(), inf.measured_at.get());
        HIP_TRY(hipGetLastError());
      }
      if (before_check) {  // what the next iteration's check takes its differences against
        if (check) HIP_TRY(hipMemcpyAsync(inf.lam_prev, inf.lam_cur, sizeof(double) * nlam, hipMemcpyDeviceToDevice, st));
        const int per = u.N * p;
        hipLaunchKernelGGL(ndlqr::lin_multipliers, dim3((per + 255) / 256, u.batch), dim3(256), 0, st, per, (const double*)k.rho,
                           (const double*)k.y, inf.mu_prev.get());
        HIP_TRY(hipGetLastError());
      }
      if (it % check_every == 0 || it == max_iter || adapt) {
        // 5. one word: how many problems still run; after an adapting update also how many moved their penalty
        HIP_TRY(hipMemcpyAsync(k.h_word, k.word, (adapt ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // (a problem that moved its penalty goes on -- unless the check behind the same update certified it: its move
        //  stands, and 5a. runs for it as for any other)
        if (k.h_word[0] == 0 && !(adapt && k.h_word[1] != 0)) break;
        if (adapt && k.h_word[1] != 0) {
          // 5a. new penalties: the whole batch shifted, reduced, packed and factored as above (a problem that did not move
          // gets its records, its res~ and its factors back bit for bit), then both right-hand sides of the moved problems
          uniform = false;
          factored = true;
          if (const int se = shift_and_reduce()) return se;
          HIP_TRY(cost_reduce_rhs_to(c, k.rec, k.q, k.r, k.d, k.x0, k.qt, k.rt, k.dt, k.x0t, st));
          e = shifted.repack();
          if (!e) e = factor_resident(c, st, &not_spd, "ndlqr_hip_solve_constrained", what);
          if (!e) e = start(ndlqr::LIN_START_MOVED);
          if (e) return e;
          HIP_TRY(hipMemsetAsync(k.word + 1, 0, sizeof(int), st));
          if (k.h_word[0] == 0) {
            // (the batch ended with that certificate: one more re-solve, so that z~ belongs to the records in force --
            //  every other problem is frozen and gets its z~ back bit for bit)
            e = launch_resolve(c, rn, k.z, "constrained solve: this configuration needs NDLQR_FLAG_KEEP_FACT");
            if (e) return e;
            break;
          }
        }
      }
    }
    // 6. deliver: S^ z~ of the last re-solve, in the caller's variables
    const size_t flds = sizeof(double) * ndlqr::lin_wave_lds(u.n, u.m, p);
    HIP_TRY(allow_lin_lds(ndlqr::lin_finish, flds, k.lds_asked[4]));
    hipLaunchKernelGGL(ndlqr::lin_finish, dim3(d.N, d.batch), dim3(64), flds, st, u, d, p, (const double*)k.rec,
                       (const double*)k.z, s.z.get());
    HIP_TRY(hipGetLastError());
    return NDLQR_OK;
  };
  err = iterate();
  // 7. the plain reduced problem again, bookkeeping
  const KeptState shifted_kept = c->kept;  // (close() forgets it for the plain API)
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (err) {
    k.fact = false;
    k.have_vy = false;
    if (!not_spd) c->state_dirty = true;  // (a failed launch; a non-positive pivot leaves the device state clean)
    if (factored) c->z_invalid = true;    // (the factorisation overwrote the resident solution)
    (void)hipStreamSynchronize(st);
    return err;
  }
  k.fact = true;  // (the initialiser inside the scope dropped it)
  k.rho_uniform = uniform;
  k.rho_value = uniform_value;
  k.flags = lin_flags;
  k.kept = shifted_kept;
  k.rhs_new = false;
  note_solution(c);
  k.soln_gen = c->soln_gen;
  if (infeas_every > 0) inf.gen = c->soln_gen;
  c->cost.mapped_gen = c->soln_gen;  // (the delivery must not apply the plain records to it)
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  c->timing_pending = true;
  err = deliver_iters_status(c, st, k.iters, k.status, iters, status);
  if (err) return err;
  return ndlqr_hip_synchronize(c);
}

int ndlqr_hip_set_constraint_adaptation(NdlqrHipCtx* c, int every, double rho_min, double rho_max) {
  if (!c) return NDLQR_ERR_INVALID;
  if (every < 0 || !(rho_min > 0.0 && rho_min <= rho_max && rho_max < HUGE_VAL))
    return refuse("ndlqr_hip_set_constraint_adaptation: bad argument (every >= 0, 0 < rho_min <= rho_max, finite)");
  c->lin.adapt_every = every;
  c->lin.rho_min = rho_min;
  c->lin.rho_max = rho_max;
  return NDLQR_OK;
}

int ndlqr_hip_set_constraint_infeasibility(NdlqrHipCtx* c, int every, double eps) {
  if (!c) return NDLQR_ERR_INVALID;
  if (every < 0 || !(eps > 0.0 && eps < HUGE_VAL))
    return refuse("ndlqr_hip_set_constraint_infeasibility: bad argument (every >= 0, eps > 0 and finite)");
  c->lin_infeas.every = every;
  c->lin_infeas.eps = eps;
  return NDLQR_OK;
}

// is the resident solution that of the latest constrained solve, and did that solve run with detection on?
static int need_constraint_infeasibility(const NdlqrHipCtx* c, const char* who) {
  if (const int merr = need_constrained(c, who)) return merr;
  const unsigned long long gen = c->lin_infeas.gen;
  if (gen == 0 || gen != c->soln_gen || c->lin.soln_gen != c->soln_gen)
    return refuse(std::string(who) + ": the resident solution is not that of a constrained solve with infeasibility detection "
                  "on (ndlqr_hip_set_constraint_infeasibility before ndlqr_hip_solve_constrained)");
  return NDLQR_OK;
}

// dlam [batch][N][n], dmu [batch][N][p] of every status-4 problem of the latest constrained solve (zero rows elsewhere),
// into host memory or this device's; either may be null. (Stored in the caller's layout: plain copies.)
int ndlqr_hip_download_constraint_infeasibility_certificate(NdlqrHipCtx* c, double* dlam, double* dmu) {
  if (!c || (!dlam && !dmu)) return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_download_constraint_infeasibility_certificate";
  if (const int serr = need_constraint_infeasibility(c, who)) return serr;
  const ndlqr::Dims& u = c->du;
  HIP_TRY(hipSetDevice(c->device));
  for (const void* o : {(const void*)dlam, (const void*)dmu})
    if (o && where(o, c->device) == Where::OtherDevice)
      return refuse(std::string(who) + ": an output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  const size_t kn = (size_t)u.batch * u.N;
  if (dlam) HIP_TRY(hipMemcpy(dlam, c->lin_infeas.cert_lam, sizeof(double) * kn * u.n, hipMemcpyDefault));
  if (dmu) HIP_TRY(hipMemcpy(dmu, c->lin_infeas.cert_mu, sizeof(double) * kn * c->lin.p, hipMemcpyDefault));
  return NDLQR_OK;
}

// measures [batch][4] = ||e||_inf | D | the maximum toward an infinite bound | S of every problem's latest check and the
// iteration it ran at (zero for a problem no check examined), as ndlqr_hip_download_infeasibility_measures
int ndlqr_hip_download_constraint_infeasibility_measures(NdlqrHipCtx* c, double* measures, int* iteration) {
  if (!c || (!measures && !iteration)) return NDLQR_ERR_INVALID;
  const char* const who = "ndlqr_hip_download_constraint_infeasibility_measures";
  if (const int serr = need_constraint_infeasibility(c, who)) return serr;
  HIP_TRY(hipSetDevice(c->device));
  for (const void* o : {(const void*)measures, (const void*)iteration})
    if (o && where(o, c->device) == Where::OtherDevice)
      return refuse(std::string(who) + ": an output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  const size_t nb = (size_t)c->du.batch;
  if (measures) HIP_TRY(hipMemcpy(measures, c->lin_infeas.measures, sizeof(double) * 4 * nb, hipMemcpyDefault));
  if (iteration) HIP_TRY(hipMemcpy(iteration, c->lin_infeas.measured_at, sizeof(int) * nb, hipMemcpyDefault));
  return NDLQR_OK;
}

// rho [batch] of the latest constrained solve, into host memory or this device's
int ndlqr_hip_download_constraint_penalties(NdlqrHipCtx* c, double* rho) {
  if (!c || !rho) return NDLQR_ERR_INVALID;
  if (const int merr = need_constrained(c, "ndlqr_hip_download_constraint_penalties")) return merr;
  if (!c->lin.have_vy) return refuse("ndlqr_hip_download_constraint_penalties: no constrained solve yet");
  HIP_TRY(hipSetDevice(c->device));
  if (where(rho, c->device) == Where::OtherDevice)
    return refuse("ndlqr_hip_download_constraint_penalties: the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(rho, c->lin.rho, sizeof(double) * (size_t)c->du.batch, hipMemcpyDefault));
  return NDLQR_OK;
}

// mu = rho[b] y [batch][N][p], into host memory or this device's
int ndlqr_hip_download_constraint_multipliers(NdlqrHipCtx* c, double* mu) {
  if (!c || !mu) return NDLQR_ERR_INVALID;
  if (const int merr = need_constrained(c, "ndlqr_hip_download_constraint_multipliers")) return merr;
  if (!c->lin.have_vy) return refuse("ndlqr_hip_download_constraint_multipliers: no constrained solve yet");
  const ndlqr::Dims& u = c->du;
  LinState& k = c->lin;
  HIP_TRY(hipSetDevice(c->device));
  const int per = u.N * k.p;
  CallerArrays<1> out = {{mu}, {(size_t)u.batch * per}};
  int err = out.classify(c, "ndlqr_hip_download_constraint_multipliers", "the output lies");
  if (err) return err;
  HIP_TRY(c->grad_stage.grow(out.stage));
  HIP_TRY(sync_all(c));
  const BufferSet& s = c->set[0];
  out.place(c);
  if (c->lin_polished()) {  // (a polished solution: its mu where the polish succeeded)
    HIP_TRY(launch_lin_polish_multipliers(c, out.dev[0], s.stream));
  } else {
    hipLaunchKernelGGL(ndlqr::lin_multipliers, dim3((per + 255) / 256, u.batch), dim3(256), 0, s.stream, per,
                       (const double*)k.rho, (const double*)k.y, out.dev[0]);
    HIP_TRY(hipGetLastError());
  }
  err = out.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

// resid [batch][4] = r_prim | r_dual | sp | sd of every problem's last update, as ndlqr_hip_download_box_residuals
int ndlqr_hip_download_constraint_residuals(NdlqrHipCtx* c, double* resid) {
  if (!c || !resid) return NDLQR_ERR_INVALID;
  if (const int merr = need_constrained(c, "ndlqr_hip_download_constraint_residuals")) return merr;
  if (c->lin.soln_gen == 0 || c->lin.soln_gen != c->soln_gen)
    return refuse("ndlqr_hip_download_constraint_residuals: the resident solution is not that of a constrained solve");
  HIP_TRY(hipSetDevice(c->device));
  if (where(resid, c->device) == Where::OtherDevice)
    return refuse("ndlqr_hip_download_constraint_residuals: the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(resid, c->lin.resid, sizeof(double) * 4 * (size_t)c->du.batch, hipMemcpyDefault));
  return NDLQR_OK;
}

// Read-out for the tests, the counterpart of ndlqr_hip_download_cost_reduction: the shifted costs, the shifted records and
// the shifted reduced problem of the latest constrained solve in the caller's flat layout, and its iterates v, y
// [batch][N][p], into HOST memory; any pointer may be null.
int ndlqr_hip_download_constraint_reduction(NdlqrHipCtx* c, double* Qs, double* Hs, double* Rs, double* L, double* LR, double* G,
                                            double* At, double* Bt, double* qt, double* rt, double* dt, double* x0t, double* v,
                                            double* y) {
  if (!c) return NDLQR_ERR_INVALID;
  if (const int merr = need_constrained(c, "ndlqr_hip_download_constraint_reduction")) return merr;
  if (!c->lin.have_vy) return refuse("ndlqr_hip_download_constraint_reduction: no constrained solve yet");
  const ndlqr::Dims& u = c->du;
  const LinState& k = c->lin;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(sync_all(c));
  const size_t kn = (size_t)u.batch * u.N, n = (size_t)u.n, m = (size_t)u.m, recd = n * n + m * m + m * n;
  double* const part[3] = {L, LR, G};
  const size_t width[3] = {n * n, m * m, m * n};
  size_t off = 0;
  for (int i = 0; i < 3; off += width[i], ++i)
    if (part[i])
      HIP_TRY(hipMemcpy2D(part[i], sizeof(double) * width[i], k.rec + off, sizeof(double) * recd, sizeof(double) * width[i], kn,
                          hipMemcpyDeviceToHost));
  double* const dst[11] = {Qs, Hs, Rs, At, Bt, qt, rt, dt, x0t, v, y};
  const double* const src[11] = {k.Qs, k.Hs, k.Rs, k.At, k.Bt, k.qt, k.rt, k.dt, k.x0t, k.v, k.y};
  const size_t cnt[11] = {kn * n * n, kn * n * m, kn * m * m, kn * n * n, kn * n * m, kn * n, kn * m, kn * n, (size_t)u.batch * n,
                          kn * k.p, kn * k.p};
  for (int i = 0; i < 11; ++i)
    if (dst[i]) HIP_TRY(hipMemcpy(dst[i], src[i], sizeof(double) * cnt[i], hipMemcpyDeviceToHost));
  return NDLQR_OK;
}

// ------------------------------------------------------------------------------ gradients through the constrained solve
// The adjoint of the active-set system K w + G_A' nu = g, G_A w = 0 (kernels_lin_grad.hpp) by the
// ADMM of the forward on its remembered shifted reduction and factorisation: the shifted reduced problem in force again
// (ShiftedReduction, restored on every exit), the kept records / factors taken as the forward left them -- nothing is
// factored --, every iteration one re-solve into lin.z plus one lin_adjoint_update, the host reading the running count
// every check_every iterations. The right-hand-side columns of the kept records are saved and restored around it as for
// the plain adjoint. Afterwards the forward's bookkeeping is put back as its own epilogue leaves it.

// is the resident solution that of the latest constrained solve, with its factorisation, right-hand side and bounds?
static int need_constrained_solution(const NdlqrHipCtx* c, const char* who) {
  if (const int merr = need_constrained(c, who)) return merr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  const LinState& k = c->lin;
  if (c->lin_polished())
    return refuse(std::string(who) + ": the resident solution was polished (ndlqr_hip_polish_constrained), which replaced the "
                  "ADMM factorisation and v, y: refused until the next ndlqr_hip_solve_constrained");
  if (k.soln_gen == 0 || k.soln_gen != c->soln_gen || !k.fact || !k.have_vy || k.rhs_new)
    return refuse(std::string(who) + ": the resident solution is not that of the latest constrained solve "
                  "(ndlqr_hip_solve_constrained first; a solve, new inputs, a new right-hand side or new bounds came after it)");
  return NDLQR_OK;
}

int ndlqr_hip_solve_constrained_adjoint(NdlqrHipCtx* c, const double* g, double alpha, double eps_abs, double eps_rel,
                                        int max_iter, int check_every, int* iters, int* status) {
  if (!c) return NDLQR_ERR_INVALID;
  if (!g || !(alpha > 0.0 && alpha < 2.0) || !(eps_abs >= 0.0) || !(eps_rel >= 0.0) || max_iter < 1 || check_every < 1)
    return refuse("ndlqr_hip_solve_constrained_adjoint: bad argument (g, 0 < alpha < 2, eps_abs >= 0, eps_rel >= 0, "
                  "max_iter >= 1, check_every >= 1)");
  if (const int serr = need_constrained_solution(c, "ndlqr_hip_solve_constrained_adjoint")) return serr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  LinState& k = c->lin;
  LinAdjointState& a = c->alin;
  if (k.kept.time_shard) return refuse("ndlqr_hip_solve_constrained_adjoint: not available on a time-axis shard");
  HIP_TRY(hipSetDevice(c->device));
  CallerArrays<1> ga = {{const_cast<double*>(g)}, {((size_t)u.rows * u.N - u.m) * d.batch}};
  int err = ga.classify(c, "ndlqr_hip_solve_constrained_adjoint", "g lies");
  if (!err) err = refuse_foreign_iters_status(c, "ndlqr_hip_solve_constrained_adjoint", iters, status);
  if (err) return err;
  HIP_TRY(c->adj.ensure(d, c->set[0].stream));
  HIP_TRY(a.ensure(u, d, k.p));
  HIP_TRY(c->grad_stage.grow(ga.stage));
  // 1. everything idle, the primary set current; g packed into the adjoint's resident right-hand side
  HIP_TRY(sync_all(c));
  c->cur = 0;
  BufferSet& s = c->set[0];
  const hipStream_t st = s.stream;
  ga.place(c);
  err = ga.copy(st, true);
  if (err) return err;
  a.gen = 0;
  c->adj.gen = 0;
  const bool strict = (k.flags & NDLQR_FLAG_STRICT_FP) != 0;
  const int p = k.p;
  const double* rhov = k.rho;  // (the vector the forward ended with: nothing here moves it)
  const size_t lds = lin_update_lds_bytes(u, p), flds = sizeof(double) * ndlqr::lin_wave_lds(u.n, u.m, p);
  // what the scope's initialiser drops and the forward's epilogue had left
  const KeptState fwd_kept = k.kept;
  const unsigned fwd_flags = k.flags;
  const bool fwd_inputs_replaced = c->inputs_replaced;
  HIP_TRY(hipEventRecord(s.ev_start, st));
  ShiftedReduction shifted(c);
  // (a lambda for its early returns: every one of them arrives at close() and the bookkeeping behind it)
  const auto iterate = [&]() -> int {
    HIP_TRY(launch_adjoint_rhs(c, ga.dev[0], st));
    // 2. the shifted reduced problem in force, the remembered factorisation taken up, its record columns saved
    int e = shifted.open(fwd_flags);
    if (e) return e;
    c->kept = fwd_kept;
    HIP_TRY(adjoint_scratch(c, false));
    // 3. codes, v = y = 0, S^' g and both right-hand sides, status
    const ndlqr::BoxParams P = {alpha, 1.0 - alpha, eps_abs, eps_rel, 0.0, 0.0};
    HIP_TRY(allow_lin_lds(ndlqr::lin_adjoint_start, flds, a.lds_asked[0]));
    if (strict) HIP_TRY(allow_lin_lds(ndlqr::lin_adjoint_update<true>, lds, a.lds_asked[1]));
    else HIP_TRY(allow_lin_lds(ndlqr::lin_adjoint_update<false>, lds, a.lds_asked[2]));
    HIP_TRY(allow_lin_lds(ndlqr::lin_adjoint_finish, flds, a.lds_asked[3]));
    HIP_TRY(hipMemsetAsync(a.word, 0, sizeof(int), st));
    // (the read-out row of a problem that is not iterated -- forward status 3 -- is zero)
    HIP_TRY(hipMemsetAsync(a.resid, 0, sizeof(double) * 4 * (size_t)u.batch, st));
    hipLaunchKernelGGL(ndlqr::lin_adjoint_start, dim3(d.N, d.batch), dim3(64), flds, st, u, d, p, (const double*)k.rec,
                       (const double*)k.lo, (const double*)k.hi, k.bstride, (const double*)k.v, (const int*)k.status,
                       c->adj.rhs.get(), a.code.get(), a.v.get(), a.y.get(), a.rhs[0].get(), a.rhs[1].get(), a.status.get(),
                       a.iters.get(), a.word.get());
    HIP_TRY(hipGetLastError());
    // 4. the iterations (none when every problem's forward ended non-finite)
    HIP_TRY(hipMemcpyAsync(a.h_word, a.word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const bool any = a.h_word[0] > 0;
    for (int it = 1; it <= max_iter && any; ++it) {
      const double* rc = a.rhs[(it - 1) & 1];
      double* rn = a.rhs[it & 1];
      e = launch_resolve(c, rc, k.z, "constrained adjoint: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
      launch_strict(strict, ndlqr::lin_adjoint_update, dim3(u.batch), dim3(256), lds, st, u, d, p, it, P, (const double*)k.z,
                    (const double*)k.rec, (const double*)k.C, (const double*)k.D, (const unsigned char*)a.code, a.v.get(),
                    a.y.get(), (const double*)c->adj.rhs, rc, rn, rhov, a.status.get(), a.iters.get(), a.resid.get(),
                    a.word.get());
      HIP_TRY(hipGetLastError());
      if (it % check_every == 0 || it == max_iter) {
        HIP_TRY(hipMemcpyAsync(a.h_word, a.word, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (a.h_word[0] == 0) break;
      }
    }
    if (!any) {  // (no re-solve ran: lin.z defined all the same -- the re-solve of S^' g)
      e = launch_resolve(c, a.rhs[0], k.z, "constrained adjoint: this configuration needs NDLQR_FLAG_KEEP_FACT");
      if (e) return e;
    }
    // 5. w = S^ w~ of the last re-solve, in the caller's variables
    hipLaunchKernelGGL(ndlqr::lin_adjoint_finish, dim3(d.N, d.batch), dim3(64), flds, st, u, d, p, (const double*)k.rec,
                       (const double*)k.z, (const int*)a.status, c->adj.z.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(adjoint_scratch(c, true));
    return NDLQR_OK;
  };
  err = iterate();
  // 6. the plain reduced problem again; the forward's bookkeeping as its epilogue left it
  const int cerr = shifted.close();
  if (!err) err = cerr;
  if (err) {
    k.fact = false;
    c->state_dirty = true;
    (void)hipStreamSynchronize(st);
    return err;
  }
  k.fact = true;  // (the initialiser inside the scope dropped it; the penalties, flags and kept were never touched)
  k.kept = fwd_kept;
  k.flags = fwd_flags;
  c->inputs_replaced = fwd_inputs_replaced;
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = deliver_iters_status(c, st, a.iters, a.status, iters, status);
  if (err) return err;
  note_elapsed(c, s);
  c->adj.gen = c->soln_gen;
  c->adj.rhs_stamp = c->rhs_stamp();
  a.gen = c->soln_gen;
  return NDLQR_OK;
}

// is there a constrained adjoint of the resident solution?
static int need_constrained_adjoint(const NdlqrHipCtx* c, const char* who) {
  if (const int merr = need_constrained(c, who)) return merr;
  if (c->z_partial || c->z_invalid) return need_full_solution(c, who);
  if (c->lin_polished())
    return refuse(std::string(who) + ": the resident solution was polished (ndlqr_hip_polish_constrained), which replaced the "
                  "ADMM factorisation and v, y: refused until the next ndlqr_hip_solve_constrained");
  if (!c->lin_adjoint_resident())
    return refuse(std::string(who) + ": no constrained adjoint of the resident solution (ndlqr_hip_solve_constrained_adjoint "
                  "after the latest constrained solve)");
  return NDLQR_OK;
}

int ndlqr_hip_constraint_gradients(NdlqrHipCtx* c, int summed, double* gC, double* gD, double* glo, double* ghi) {
  if (!c) return NDLQR_ERR_INVALID;
  if (const int aerr = need_constrained_adjoint(c, "ndlqr_hip_constraint_gradients")) return aerr;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  const LinState& k = c->lin;
  const LinAdjointState& a = c->alin;
  const int p = k.p;
  HIP_TRY(hipSetDevice(c->device));
  const size_t P = summed ? 1 : (size_t)u.batch, kn = P * u.N;
  CallerArrays<4> go = {{gC, gD, glo, ghi}, {kn * p * u.n, kn * p * u.m, kn * p, kn * p}};
  int err = go.classify(c, "ndlqr_hip_constraint_gradients", "an output lies");
  if (err) return err;
  if (!gC && !gD && !glo && !ghi) return NDLQR_OK;
  // batch sums: entries of [N][W] one per thread, the batch split into about 2048 / ceil(entries / 256) runs of problems
  // added in order, then the runs in order (ndlqr_hip_bound_gradients' scheme: deterministic, no atomics)
  const size_t E = (size_t)u.N * ndlqr::lin_grad_width(u.n, u.m, p);
  const unsigned nblk = (unsigned)((E + 255) / 256);
  int nsplit = 1, ppb = u.batch;
  if (summed) {
    nsplit = (int)(2048 / nblk);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > u.batch) nsplit = u.batch;
    ppb = (u.batch + nsplit - 1) / nsplit;
    nsplit = (u.batch + ppb - 1) / ppb;
  }
  const size_t npart = nsplit > 1 ? (size_t)nsplit * E : 0;
  HIP_TRY(c->grad_stage.grow(go.stage + npart));
  HIP_TRY(sync_all(c));
  BufferSet& s = c->set[0];
  ndlqr::LinGradOut out = {};
  double* part = go.place(c);  // (the partial sums behind the staged outputs)
  if (!npart) part = nullptr;
  for (int i = 0; i < 4; ++i) out.p[i] = go.dev[i];
  const bool strict = (k.flags & NDLQR_FLAG_STRICT_FP) != 0;
  const double* z = c->set[c->latest].z;
  HIP_TRY(hipEventRecord(s.ev_start, s.stream));
  if (!summed) {
    launch_strict(strict, ndlqr::lin_constraint_grads, dim3(u.N, u.batch), dim3(64), 0, s.stream, u, d, p, (const double*)k.rho,
                  (const unsigned char*)a.code, (const double*)k.y, (const double*)a.y, (const int*)a.status, z,
                  (const double*)c->adj.z, out);
    HIP_TRY(hipGetLastError());
  } else {
    launch_strict(strict, ndlqr::lin_constraint_grads_sum, dim3(nblk, nsplit), dim3(256), 0, s.stream, u, d, p, (const double*)k.rho, ppb,
                  (const unsigned char*)a.code, (const double*)k.y, (const double*)a.y, (const int*)a.status, z,
                  (const double*)c->adj.z, out, part);
    HIP_TRY(hipGetLastError());
    if (part) {
      hipLaunchKernelGGL(ndlqr::lin_grad_sum_splits, dim3(nblk), dim3(256), 0, s.stream, u, p, nsplit, (const double*)part, out);
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

// nu = rho y of the latest constrained adjoint [batch][N][p] (0 outside the active set), into host memory or this device's
int ndlqr_hip_download_constraint_adjoint_multipliers(NdlqrHipCtx* c, double* nu) {
  if (!c || !nu) return NDLQR_ERR_INVALID;
  if (const int aerr = need_constrained_adjoint(c, "ndlqr_hip_download_constraint_adjoint_multipliers")) return aerr;
  const ndlqr::Dims& u = c->du;
  const LinAdjointState& a = c->alin;
  HIP_TRY(hipSetDevice(c->device));
  const int per = u.N * c->lin.p;
  CallerArrays<1> out = {{nu}, {(size_t)u.batch * per}};
  int err = out.classify(c, "ndlqr_hip_download_constraint_adjoint_multipliers", "the output lies");
  if (err) return err;
  HIP_TRY(c->grad_stage.grow(out.stage));
  HIP_TRY(sync_all(c));
  const BufferSet& s = c->set[0];
  out.place(c);
  hipLaunchKernelGGL(ndlqr::lin_adjoint_multipliers, dim3((per + 255) / 256, u.batch), dim3(256), 0, s.stream, per,
                     (const double*)c->lin.rho, (const unsigned char*)a.code, (const double*)a.y, out.dev[0]);
  HIP_TRY(hipGetLastError());
  err = out.copy(s.stream, false);
  if (err) return err;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return NDLQR_OK;
}

// resid [batch][4] of every problem's last adjoint update (a row of zeros for a problem that was not iterated)
int ndlqr_hip_download_constraint_adjoint_residuals(NdlqrHipCtx* c, double* resid) {
  if (!c || !resid) return NDLQR_ERR_INVALID;
  if (const int aerr = need_constrained_adjoint(c, "ndlqr_hip_download_constraint_adjoint_residuals")) return aerr;
  HIP_TRY(hipSetDevice(c->device));
  if (where(resid, c->device) == Where::OtherDevice)
    return refuse("ndlqr_hip_download_constraint_adjoint_residuals: the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  HIP_TRY(hipMemcpy(resid, c->alin.resid, sizeof(double) * 4 * (size_t)c->du.batch, hipMemcpyDefault));
  return NDLQR_OK;
}

// the row codes [batch][N][p] bytes of the latest constrained adjoint (0 unbounded, 1 free, 2 fixed at the lower bound,
// 3 at the upper), into host memory or this device's; v: the adjoint's own projected iterate (read-out for the tests,
// HOST memory, may be null)
int ndlqr_hip_download_constraint_codes(NdlqrHipCtx* c, unsigned char* codes, double* v) {
  if (!c || (!codes && !v)) return NDLQR_ERR_INVALID;
  if (const int aerr = need_constrained_adjoint(c, "ndlqr_hip_download_constraint_codes")) return aerr;
  HIP_TRY(hipSetDevice(c->device));
  if (codes && where(codes, c->device) == Where::OtherDevice)
    return refuse("ndlqr_hip_download_constraint_codes: the output lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  const size_t np = (size_t)c->du.batch * c->du.N * c->lin.p;
  if (codes) HIP_TRY(hipMemcpy(codes, c->alin.code, np, hipMemcpyDefault));
  if (v) HIP_TRY(hipMemcpy(v, c->alin.v, sizeof(double) * np, hipMemcpyDeviceToHost));
  return NDLQR_OK;
}
