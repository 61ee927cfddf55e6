// hip_gain.hip -- feedback gains and cost-to-go matrices of the resident problems (ndlqr_hip_feedback_gains; DESIGN.md
// section 3.22): the host side, the kernels of kernels_gain.hpp.
#include "hip_host.hpp"
#include "kernels_gain.hpp"

// Workgroup size of gain_sweep: 256 threads at every block size. They cover the n (n + m) entries of the two products from
// (12,4) up, and measured faster than one or two wavefronts down to n + m = 16 as well, where a single wavefront would
// have free barriers (2.2 against 3.0 ms at (12,4,256) x 1024; DESIGN.md section 3.22 has the table).
// NDLQR_GAIN_THREADS (developer: 64, 128, 256) overrides it for an A/B.
static int gain_threads() {
  if (const char* e = getenv("NDLQR_GAIN_THREADS")) {
    const int t = atoi(e);
    if (t == 64 || t == 128 || t == 256) return t;
  }
  return 256;
}
// does the sweep run with the second buffer? (NDLQR_GAIN_PREFETCH=0, developer: never)
static bool gain_prefetch(const ndlqr::Dims& u, int threads) {
  if (const char* e = getenv("NDLQR_GAIN_PREFETCH"))
    if (atoi(e) == 0) return false;
  return ndlqr::gain_prefetch_fits(u.n, u.m, threads) && sizeof(double) * ndlqr::gain_layout(u.n, u.m, true).total <= kLdsMax;
}

// dynamic LDS (bytes) of gain_sweep at (n, m): with the second buffer, or without it
size_t ndlqr_hip_feedback_gains_lds(int n, int m, int second) {
  return n > 0 && m > 0 ? sizeof(double) * ndlqr::gain_layout(n, m, second != 0).total : 0;
}

int ndlqr_hip_feedback_gains(NdlqrHipCtx* c, int knot0, int nknots, double* K, double* kff, double* P, double* p, int* fails) {
  static const char* const who = "ndlqr_hip_feedback_gains";
  if (!c) return NDLQR_ERR_INVALID;
  const ndlqr::Dims& d = c->d;
  const ndlqr::Dims& u = c->du;
  const int n = u.n, m = u.m, N = u.N, batch = u.batch;
  if (c->lin.active)
    return refuse(std::string(who) + ": not available in constrained (linear-inequality) mode: the resident problem is the "
                                     "rho-shifted one, its gains are not those of the caller's problem");
  if (c->kept.time_shard) return refuse(std::string(who) + ": not available on a time-axis shard");
  if (knot0 < 0 || nknots <= 0 || knot0 > N - nknots)
    return refuse(std::string(who) + ": knots [" + std::to_string(knot0) + ", " + std::to_string((long long)knot0 + nknots) +
                  ") are not a non-empty range within the " + std::to_string(N) + " knots of the horizon");
  if (!K && !kff && !P && !p) return refuse(std::string(who) + ": no output asked for (K, kff, P, p are all null)");
  const bool dense = c->cost.dense;
  const int threads = gain_threads();
  const bool second = gain_prefetch(u, threads);
  const size_t lds = sizeof(double) * ndlqr::gain_layout(n, m, second).total;
  const size_t lds_back = dense ? sizeof(double) * ndlqr::gain_map_back_lds(n, m) : 0;
  if (lds > kLdsMax || lds_back > kLdsMax)
    return refuse(std::string(who) + ": " + (lds > kLdsMax ? "gain_sweep" : "gain_map_back") + " needs " +
                  std::to_string(lds > kLdsMax ? lds : lds_back) + " bytes of LDS at (" + std::to_string(n) + "," +
                  std::to_string(m) + "), beyond the " + std::to_string(kLdsMax) + " bytes of a workgroup");
  HIP_TRY(hipSetDevice(c->device));
  const size_t kn = (size_t)batch * nknots, cnt[4] = {kn * m * n, kn * m, kn * n * n, kn * n};
  CallerArrays<4> ca = {{K, kff, P, p}, {cnt[0], cnt[1], cnt[2], cnt[3]}};
  int err = ca.classify(c, who, "an output lies");
  if (err) return err;
  const Where wf = fails ? where(fails, c->device) : Where::Pageable;
  if (wf == Where::OtherDevice) return refuse(std::string(who) + ": fails lies in the memory of another device than the solver's");
  HIP_TRY(sync_all(c));
  err = rhs_make_current(c, 0xFu);
  if (err) return err;
  // behind the staged outputs: in dense-cost mode the sweep's four outputs on the reduced problem, then the pivot counts
  const size_t nred = dense ? cnt[0] + cnt[1] + cnt[2] + cnt[3] : 0;
  HIP_TRY(c->grad_stage.grow(ca.stage + nred + ((size_t)batch + 1) / 2));
  double* red = ca.place(c);
  int* d_fails = reinterpret_cast<int*>(red + nred);
  double* out[4];
  for (int o = 0; o < 4; ++o) out[o] = ca.dev[o];
  if (dense) {
    size_t at = 0;
    for (int o = 0; o < 4; at += cnt[o], ++o) out[o] = red + at;
  }
  BufferSet& s = c->set[c->cur];
  const hipStream_t st = s.stream;
  HIP_TRY(second ? allow_dynamic_lds(&ndlqr::gain_sweep<true>, lds) : allow_dynamic_lds(&ndlqr::gain_sweep<false>, lds));
  HIP_TRY(hipEventRecord(s.ev_start, st));
  if (second)
    hipLaunchKernelGGL(ndlqr::gain_sweep<true>, dim3(batch), dim3(threads), lds, st, u, d, (const double*)c->AB,
                       (const double*)c->QR, (const double*)s.rhs, knot0, nknots, out[0], out[1], out[2], out[3], d_fails);
  else
    hipLaunchKernelGGL(ndlqr::gain_sweep<false>, dim3(batch), dim3(threads), lds, st, u, d, (const double*)c->AB,
                       (const double*)c->QR, (const double*)s.rhs, knot0, nknots, out[0], out[1], out[2], out[3], d_fails);
  HIP_TRY(hipGetLastError());
  if (dense) {
    HIP_TRY(allow_dynamic_lds(&ndlqr::gain_map_back, lds_back));
    hipLaunchKernelGGL(ndlqr::gain_map_back, dim3(nknots, batch), dim3(64), lds_back, st, n, m, N, knot0, nknots,
                       (const double*)c->cost.rec, (const double*)out[0], (const double*)out[1], (const double*)out[2],
                       (const double*)out[3], ca.dev[0], ca.dev[1], ca.dev[2], ca.dev[3]);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s.ev_stop, st));
  err = ca.copy(st, false);
  if (err) return err;
  std::vector<int> h_fails(batch);
  HIP_TRY(hipMemcpyAsync(h_fails.data(), d_fails, sizeof(int) * batch, hipMemcpyDeviceToHost, st));
  if (fails && wf == Where::OwnDevice)
    HIP_TRY(hipMemcpyAsync(fails, d_fails, sizeof(int) * batch, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  note_elapsed(c, s);
  int total = 0;
  for (int b = 0; b < batch; ++b) total += h_fails[b] != 0;
  if (fails && wf != Where::OwnDevice) memcpy(fails, h_fails.data(), sizeof(int) * batch);
  return total ? NDLQR_ERR_NOT_SPD : NDLQR_OK;
}
