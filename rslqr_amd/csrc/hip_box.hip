// hip_box.hip -- the box-constrained solve (ndlqr_hip_set_bounds, ndlqr_hip_solve_box) with infeasibility detection
// and Anderson acceleration, its read-outs, its adjoint and bound gradients, and the active-set polish with its adjoint:
// the host side, the kernels of kernels_box*.hpp. The polish lives here because it shares ShiftedQR with the ADMM.
#include "hip_host.hpp"
#include "kernels_box.hpp"
#include "kernels_box_accel.hpp"
#include "kernels_box_grad.hpp"
#include "kernels_box_infeas.hpp"
#include "kernels_box_polish.hpp"

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
    HIP_TRY(hipMemcpyAsync(c->box.qr_save, c->QR, sizeof(double) * doubles_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream));
    open_ = true;
    c->flags = flags;
    return NDLQR_OK;
  }
  // the saved QR again
  int restore() {
    HIP_TRY(hipMemcpyAsync(c->QR, c->box.qr_save, sizeof(double) * doubles_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream));
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
    const hipError_t qe = hipMemcpyAsync(c->QR, c->box.qr_save, sizeof(double) * doubles_QR(c->d), hipMemcpyDeviceToDevice, c->set[0].stream);
    c->flags = user_flags;
    c->kept.forget_factorisation();
    if (ce != hipSuccess) return fail("restoring the record columns", ce);
    return qe != hipSuccess ? fail("restoring QR", qe) : NDLQR_OK;
  }
};

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
      e = factor_resident(c, st, &not_spd, "ndlqr_hip_solve_box", "Q + rho M, R + rho M");
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
          if (!e) e = factor_resident(c, st, &not_spd, "ndlqr_hip_solve_box", "Q + rho M, R + rho M");
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
    HIP_TRY(launch_adjoint_rhs(c, ga.dev[0], st));
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

// ------------------------------------------------------------------------------ active-set polish
// ndlqr_hip_polish_box (kernels_box_polish.hpp): the active set read off the latest constrained
// solve, QR shifted by sigma on its entries inside a ShiftedQR scope and factored by factor_resident, then per round up to
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
  if (c->cost.dense)
    return refuse("ndlqr_hip_polish_box: not available in dense-cost mode, constrained mode included: bounds on a dense-cost "
                  "problem are rows of ndlqr_InitializeBatchFlatConstrained, and the polish of that solve is "
                  "ndlqr_hip_polish_constrained (ndlqr_PolishBatchLinConstrained)");
  if (const int herr = need_unpadded_horizon(c, "ndlqr_hip_polish_box")) return herr;
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
      e = factor_resident(c, st, &not_spd, "ndlqr_hip_polish_box", "Q, R + sigma on the active entries");
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
  p.fact = true;  // (factor_resident dropped the ADMM's)
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
    HIP_TRY(launch_adjoint_rhs(c, ga.dev[0], st));
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

