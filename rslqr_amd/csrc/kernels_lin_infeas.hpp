// kernels_lin_infeas.hpp -- internal: primal infeasibility detection of the solve with linear inequality constraints
// (ndlqr_hip_set_constraint_infeasibility, ndlqr_hip_download_constraint_infeasibility_certificate).
//
// Section 3.14 carried to the rows lo_k <= C_k x_k + D_k u_k <= hi_k. With lambda^i the multipliers of re-solve i IN THE
// CALLER'S VARIABLES (lambda_k = L^_k lambda~_k under the shifted records that re-solve used) and mu^i = rho^i y^i after
// the update of iteration i, the differences over one ADMM iteration
//     dlam = lambda^it - lambda^(it-1),   dmu = mu^it - mu^(it-1)   ([N][p], 0 on the unbounded rows)
// are a Farkas certificate of "dynamics + rows has no point" when, with
//     e_x,k = -dlam_k + A_k' dlam_(k+1) + C_k' dmu_k     e_u,k = B_k' dlam_(k+1) + D_k' dmu_k
// (the last knot: no A', B', D' term and no e_u) and
//     S = sum_bounded rows (hi max(dmu, 0) + lo min(dmu, 0)) - x0' dlam_0 - sum_k d_k' dlam_(k+1),
// e = 0 and S < 0: every (x, u) that satisfies the dynamics and the rows has e'(x, u) <= S. A row whose dmu points to an
// infinite bound contributes nothing to S and must be negligible. lin_certify tests, with D = ||dmu||_inf,
//     D > 0,   ||e||_inf <= eps D,   max |dmu_i| over the rows pointing to an infinite bound <= eps D,   S < -eps D
// and every one of these numbers finite. Everything is in the caller's block sizes and horizon (u): A, B, C, D, d, x0 and
// the bounds as LinState retains them; only lin_lambda_out reads the device layout (d).
//
// Compiled with floating-point contraction off (the error-free transformations of kernels_dd.hpp); the explicit fma()
// calls stay fused. One code path for fast and strict mode.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_dd.hpp"
#include "kernels_lin.hpp"

namespace ndlqr {

// doubles of LDS of lin_lambda_out: the knot's L^ and lambda~
__host__ __device__ inline size_t lin_lambda_lds(int n) { return (size_t)n * cost_ld(n) + (size_t)n; }

// lambda = L^ lambda~ of every knot of the re-solve z~ (device layout d) under the shifted records rec, into lam
// [batch][N][n] (the caller's horizon): the lambda rows of lin_deliver_knot and nothing else, with its staging and its
// arithmetic (cost_stage_record, the fma chain of cost_knot_S<true>) -- bit for bit what lin_finish would deliver.
//   grid (u.N, batch), block 64, dynamic LDS lin_lambda_lds(n) doubles.
static __global__ __launch_bounds__(64) void lin_lambda_out(Dims u, Dims d, const double* __restrict__ rec,
                                                            const double* __restrict__ z, double* __restrict__ lam) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int n = u.n, ldn = cost_ld(n);
  double* sL = lin_lds;
  double* sl = sL + (size_t)n * ldn;
  const size_t kb = (size_t)b * u.N + k, ok = ((size_t)b * d.N + k) * d.rows;
  cost_stage_record(rec + kb * cost_record_doubles(n, u.m), n, u.m, false, sL, nullptr, nullptr, lane);
  for (int i = lane; i < n; i += 64) sl[i] = z[ok + i];
  wave_lds_sync();
  for (int i = lane; i < n; i += 64) {
    double s = 0.0;
    for (int c = 0; c <= i; ++c) s = fma(sL[i + ldn * c], sl[c], s);
    lam[kb * n + i] = s;
  }
}

// knots a workgroup of lin_certify takes per pass: as many as its 256 threads have columns of [A | B] for
__host__ __device__ inline int lin_certify_group(const int w) { return w >= 256 ? 1 : 256 / w; }
// dynamic LDS: dlam of the knots of a pass and of the one behind them, and dmu of the knots of a pass
static inline size_t lin_certify_lds_bytes(const Dims& u, int p) {
  const size_t G = (size_t)lin_certify_group(u.w);
  return sizeof(double) * ((G + 1) * u.n + G * p);
}

// The test above for every running problem (status[b] == 0) behind lin_update of iteration `it`: lam, lam_prev are the
// multipliers of this re-solve and of the one before in the caller's variables (lin_lambda_out), y, rhov the scaled dual
// and the penalties after this update, mu_prev = rho y after the one before (lin_multipliers). A certified problem is
// frozen: status 4, iters[b] = it, one less in running[0], rhs_cur takes a copy of rhs_next on the x and u rows so that
// every later re-solve solves the same system, and dlam, dmu go to cert_lam [batch][N][n], cert_mu [batch][N][p] (zero
// before the solve). Task t = g w + j of a pass is column j of [A | B] of its g-th knot: one thread forms e of that
// entry -- a unit-stride dot product with dlam of the next knot, another with the knot's dmu staged in LDS --; the
// thread that stages a dlam or dmu entry takes its term of S and its maxima. The sums of S stay in a two-term accumulator
// per thread and are added up in a fixed tree, the maxima likewise with max_nan: the decision is the same from run to
// run. The four numbers it is taken from go to measures [batch][4] = ||e||_inf | D | the maximum toward an infinite
// bound | S, and `it` to measured_at [batch], before it is taken: for every problem the launch examined.
//   grid (batch), block 256, dynamic LDS lin_certify_lds_bytes(u, p).
static __global__ __launch_bounds__(256) void lin_certify(Dims u, Dims d, int p, int it, double eps,
                                                          const double* __restrict__ A, const double* __restrict__ B,
                                                          const double* __restrict__ C, const double* __restrict__ D,
                                                          const double* __restrict__ dv, const double* __restrict__ x0,
                                                          const double* __restrict__ lo, const double* __restrict__ hi,
                                                          size_t bstride, const double* __restrict__ lam,
                                                          const double* __restrict__ lam_prev, const double* __restrict__ y,
                                                          const double* __restrict__ mu_prev, const double* __restrict__ rhov,
                                                          double* __restrict__ rhs_cur, const double* __restrict__ rhs_next,
                                                          int* __restrict__ status, int* __restrict__ iters,
                                                          int* __restrict__ running, double* __restrict__ cert_lam,
                                                          double* __restrict__ cert_mu, double* __restrict__ measures,
                                                          int* __restrict__ measured_at) {
#pragma clang fp contract(off)
  extern __shared__ double certify_lds[];  // dlam of knots k0 .. k0 + G, [G + 1][n], then dmu of knots k0 .. k0 + G - 1, [G][p]
  __shared__ double red[5][256];           // |e|, |dmu|, |dmu| toward an infinite bound, S hi, S lo
  __shared__ int found_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const int n = u.n, m = u.m, w = u.w, N = u.N;
  const int G = lin_certify_group(w);
  double* sdl = certify_lds;
  double* sdm = sdl + (size_t)(G + 1) * n;
  const double rho = rhov[b];
  const size_t ol = (size_t)b * N * n, ov = (size_t)b * N * p;
  const double* lb = lo + (size_t)b * bstride;
  const double* hb = hi + (size_t)b * bstride;
  double emax = 0.0, dmax = 0.0, dinf = 0.0, scale = 0.0;
  DD S = {0.0, 0.0};
  for (int k0 = 0; k0 < N; k0 += G) {
    const int nk = k0 + G < N ? G : N - k0;    // knots of this pass
    const int nl = k0 + nk < N ? nk + 1 : nk;  // ... and those whose dlam it needs
    __syncthreads();
    for (int t = tid; t < nl * n; t += blockDim.x) {
      const int g = t / n, i = t - g * n, k = k0 + g;
      const size_t at = ol + (size_t)k * n + i;
      const double dl = lam[at] - lam_prev[at];
      sdl[t] = dl;
      // -x0' dlam_0, -d_(k-1)' dlam_k: once per knot (the knot behind a pass belongs to the next one)
      if (g < nk) dd_fma(S, scale, k == 0 ? -x0[(size_t)b * n + i] : -dv[ol + (size_t)(k - 1) * n + i], dl);
    }
    for (int t = tid; t < nk * p; t += blockDim.x) {
      const size_t eb = (size_t)k0 * p + t;
      const double l = lb[eb], h = hb[eb];
      double dm = 0.0;
      if (box_bounded(l, h)) {
        const double m1 = rho * y[ov + eb];
        dm = m1 - mu_prev[ov + eb];
        const double bound = dm > 0.0 ? h : l;  // the side dmu points to
        if (dm != dm || (dm != 0.0 && !(fabs(bound) < HUGE_VAL))) dinf = max_nan(dinf, fabs(dm));
        else if (dm != 0.0) dd_fma(S, scale, bound, dm);
        dmax = max_nan(dmax, fabs(dm));
      }
      sdm[t] = dm;
    }
    __syncthreads();
    for (int t = tid; t < nk * w; t += blockDim.x) {
      const int g = t / w, j = t - g * w, k = k0 + g;
      const bool last = k == N - 1;
      if (last && j >= n) continue;  // (no e_u at the last knot; its B, D are never loaded)
      const size_t kb = (size_t)b * N + k;
      const double* cc = j < n ? C + (kb * n + j) * p : D + (kb * m + (j - n)) * p;  // column j of C_k | D_k
      const double* dm = sdm + (size_t)g * p;
      double e = 0.0;
      for (int r = 0; r < p; ++r) e = fma(cc[r], dm[r], e);
      if (!last) {  // column j of [A_k | B_k] against dlam_(k+1)
        const double* col = j < n ? A + (kb * n + j) * n : B + (kb * m + (j - n)) * n;
        const double* dl = sdl + (size_t)(g + 1) * n;
        for (int i = 0; i < n; ++i) e = fma(col[i], dl[i], e);
      }
      if (j < n) e = e - sdl[g * n + j];
      emax = max_nan(emax, fabs(e));
    }
  }
  red[0][tid] = emax; red[1][tid] = dmax; red[2][tid] = dinf; red[3][tid] = S.hi; red[4][tid] = S.lo;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      for (int q = 0; q < 3; ++q) red[q][tid] = max_nan(red[q][tid], red[q][tid + s]);
      DD acc = {red[3][tid], red[4][tid]};
      dd_add(acc, red[3][tid + s], red[4][tid + s]);
      red[3][tid] = acc.hi; red[4][tid] = acc.lo;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double E = red[0][0], Dm = red[1][0], I = red[2][0], sum = red[3][0] + red[4][0];
    measures[4 * (size_t)b] = E; measures[4 * (size_t)b + 1] = Dm; measures[4 * (size_t)b + 2] = I; measures[4 * (size_t)b + 3] = sum;
    measured_at[b] = it;
    // a NaN or an infinity anywhere: no certificate (the comparisons alone would already refuse a NaN)
    const bool finite = isfinite(E) && isfinite(Dm) && isfinite(I) && isfinite(sum);
    const double tol = eps * Dm;
    const int found = finite && Dm > 0.0 && E <= tol && I <= tol && sum < -tol;
    if (found) {
      status[b] = 4;
      iters[b] = it;
      atomicSub(running, 1);
    }
    found_s = found;
  }
  __syncthreads();
  if (!found_s) return;
  for (unsigned e = tid; e < (unsigned)(N * p); e += blockDim.x)
    cert_mu[ov + e] = box_bounded(lb[e], hb[e]) ? rho * y[ov + e] - mu_prev[ov + e] : 0.0;
  for (unsigned e = tid; e < (unsigned)(N * n); e += blockDim.x) cert_lam[ol + e] = lam[ol + e] - lam_prev[ol + e];
  // both ping-pong right-hand sides hold the system of rhs_next from here on
  lin_tail_frozen(u, d, (size_t)b * d.N * d.rows, rhs_next, rhs_cur, tid);
}

}  // namespace ndlqr
