// kernels_box_infeas.hpp -- internal: primal infeasibility detection of the box-constrained batch solve
// (ndlqr_hip_set_box_infeasibility, ndlqr_hip_download_infeasibility_certificate).
//
// With lambda^i the multipliers of re-solve i and mu^i = rho^i y^i after the update of iteration i, the differences over
// one ADMM iteration
//     dlam = lambda^it - lambda^(it-1),   dmu = rho^it y^it - rho^(it-1) y^(it-1)   (0 on the unbounded entries)
// are a Farkas certificate of "dynamics + box has no point" when, with
//     e_x,k = -dlam_k + A_k' dlam_(k+1) + dmu_x,k     e_u,k = B_k' dlam_(k+1) + dmu_u,k     (no A', B' term at k = N - 1)
//     S = sum_bounded (hi max(dmu, 0) + lo min(dmu, 0)) - x0' dlam_0 - sum_k d_k' dlam_(k+1),
// e = 0 and S < 0: every (x, u) that satisfies the dynamics and the bounds has e'(x, u) <= S. An entry whose dmu points to
// an infinite bound contributes nothing to S and must be negligible. box_certify tests, with D = ||dmu||_inf,
//     D > 0,   ||e||_inf <= eps D,   max |dmu_i| over the entries pointing to an infinite bound <= eps D,   S < -eps D
// and every one of these numbers finite.
//
// Compiled with floating-point contraction off (the error-free transformations of kernels_refine.hpp); the explicit fma()
// calls stay fused. One code path for fast and strict mode.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box.hpp"
#include "kernels_common.hpp"
#include "kernels_dd.hpp"

namespace ndlqr {

// knots a workgroup of box_certify takes per pass: as many as its 256 threads have columns of [A | B] for
__host__ __device__ inline int certify_group(const int w) { return w >= 256 ? 1 : 256 / w; }
// dynamic LDS: dlam of the knots of a pass and of the one behind them
static inline size_t certify_lds_bytes(const Dims& d) { return sizeof(double) * (size_t)(certify_group(d.w) + 1) * d.n; }

// The test above for every running problem (status[b] == 0) behind box_update of iteration `it`: z, y, rhov are the
// re-solve, the scaled dual and the penalties of this iteration, zp, yp, rhop their copies of the one before; res is the
// resident right-hand side (its lambda rows are -x0 | -d_(k-1)). A certified problem is frozen: status 4, one less in
// running[0], rhs_cur takes a copy of rhs_next on its bounded entries so that every later re-solve solves the same
// system, and dlam, dmu go to cert_lam [batch][N][n], cert_mu [batch][N][n+m] (device block sizes; zero before the solve).
// Task t = g w + j of a pass is column j of [A | B] of its g-th knot: one thread forms e of that entry, its terms of S
// and its maxima; the sums of S stay in a two-term accumulator per thread and are added up in a fixed tree, the maxima
// likewise with max_nan: the decision is the same from run to run. The four numbers the decision is taken from go to
// measures [batch][4] = ||e||_inf | D | the maximum toward an infinite bound | S, and `it` to measured_at [batch], before
// it is taken: for every problem the launch examined, whatever becomes of it (a NaN among them is stored as it is).
//   grid (batch), block 256, dynamic LDS certify_lds_bytes(d).
static __global__ __launch_bounds__(256) void box_certify(Dims d, int it, double eps, const double* __restrict__ AB,
                                                          const double* __restrict__ z, const double* __restrict__ zp,
                                                          const double* __restrict__ y, const double* __restrict__ yp,
                                                          const double* __restrict__ rhov, const double* __restrict__ rhop,
                                                          const double* __restrict__ lo, const double* __restrict__ hi,
                                                          size_t bstride, const double* __restrict__ res,
                                                          double* __restrict__ rhs_cur, const double* __restrict__ rhs_next,
                                                          int* __restrict__ status, int* __restrict__ iters,
                                                          int* __restrict__ running, double* __restrict__ cert_lam,
                                                          double* __restrict__ cert_mu, double* __restrict__ measures,
                                                          int* __restrict__ measured_at) {
#pragma clang fp contract(off)
  extern __shared__ double certify_lds[];  // dlam of knots k0 .. k0 + G, [G + 1][n]
  __shared__ double red[5][256];           // |e|, |dmu|, |dmu| toward an infinite bound, S hi, S lo
  __shared__ int found_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const int n = d.n, w = d.w, rows = d.rows, N = d.N;
  const int G = certify_group(w);
  const double rho = rhov[b], rho_prev = rhop[b];
  const size_t oz = (size_t)b * N * rows, ov = (size_t)b * N * w;
  const double* lb = lo + (size_t)b * bstride;
  const double* hb = hi + (size_t)b * bstride;
  const double* ab = AB + (size_t)b * N * n * w;
  double emax = 0.0, dmax = 0.0, dinf = 0.0, scale = 0.0;
  DD S = {0.0, 0.0};
  for (int k0 = 0; k0 < N; k0 += G) {
    const int nk = k0 + G < N ? G : N - k0;           // knots of this pass
    const int nl = k0 + nk < N ? nk + 1 : nk;         // ... and those whose dlam it needs
    __syncthreads();
    for (int t = tid; t < nl * n; t += blockDim.x) {
      const int g = t / n, i = t - g * n;
      const size_t at = oz + (size_t)(k0 + g) * rows + i;
      certify_lds[t] = z[at] - zp[at];
    }
    __syncthreads();
    for (int t = tid; t < nk * w; t += blockDim.x) {
      const int g = t / w, j = t - g * w, k = k0 + g;
      const size_t eb = (size_t)k * w + j;
      const double l = lb[eb], h = hb[eb];
      double dm = 0.0;
      if (box_bounded(l, h)) {
        const double m1 = rho * y[ov + eb], m0 = rho_prev * yp[ov + eb];
        dm = m1 - m0;
        const double bound = dm > 0.0 ? h : l;  // the side dmu points to
        if (dm != dm || (dm != 0.0 && !(fabs(bound) < HUGE_VAL))) dinf = max_nan(dinf, fabs(dm));
        else if (dm != 0.0) dd_fma(S, scale, bound, dm);
        dmax = max_nan(dmax, fabs(dm));
      }
      double e = dm;
      if (k < N - 1) {  // column j of [A_k | B_k] against dlam_(k+1)
        const double* col = ab + (size_t)k * n * w + j;
        const double* dl = certify_lds + (g + 1) * n;
        for (int i = 0; i < n; ++i) e = fma(col[(size_t)i * w], dl[i], e);
      }
      if (j < n) {
        const double dlk = certify_lds[g * n + j];
        e = e - dlk;
        dd_fma(S, scale, res[oz + (size_t)k * rows + j], dlk);  // -x0' dlam_0, -d_(k-1)' dlam_k
      }
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
    const double E = red[0][0], D = red[1][0], I = red[2][0], sum = red[3][0] + red[4][0];
    measures[4 * (size_t)b] = E; measures[4 * (size_t)b + 1] = D; measures[4 * (size_t)b + 2] = I; measures[4 * (size_t)b + 3] = sum;
    measured_at[b] = it;
    // a NaN or an infinity anywhere: no certificate (the comparisons alone would already refuse a NaN)
    const bool finite = isfinite(E) && isfinite(D) && isfinite(I) && isfinite(sum);
    const double tol = eps * D;
    const int found = finite && D > 0.0 && E <= tol && I <= tol && sum < -tol;
    if (found) {
      status[b] = 4;
      iters[b] = it;
      atomicSub(running, 1);
    }
    found_s = found;
  }
  __syncthreads();
  if (!found_s) return;
  for (unsigned e = tid; e < (unsigned)(N * w); e += blockDim.x) {
    const bool bounded = box_bounded(lb[e], hb[e]);
    cert_mu[ov + e] = bounded ? rho * y[ov + e] - rho_prev * yp[ov + e] : 0.0;
    if (bounded) {
      const size_t at = oz + box_entry_offset(d, e);
      rhs_cur[at] = rhs_next[at];
    }
  }
  for (unsigned e = tid; e < (unsigned)(N * n); e += blockDim.x) {
    const unsigned k = e / (unsigned)n, i = e - k * (unsigned)n;
    const size_t at = oz + (size_t)k * rows + i;
    cert_lam[(size_t)b * N * n + e] = z[at] - zp[at];
  }
}

// The certificate into the caller's flat layout: dlam [batch][N][n], dmu_x [batch][N][n], dmu_u [batch][N][m] (each may
// be nullptr).
//   grid (N, batch), block 64.
static __global__ void box_certificate_out(Dims du, Dims d, const double* __restrict__ cert_lam,
                                           const double* __restrict__ cert_mu, double* __restrict__ dlam,
                                           double* __restrict__ dmu_x, double* __restrict__ dmu_u) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t kb = (size_t)b * d.N + k, ku = (size_t)b * du.N + k;
  for (int j = threadIdx.x; j < du.n + du.m; j += blockDim.x) {
    if (j < du.n) {
      if (dlam) dlam[ku * du.n + j] = cert_lam[kb * d.n + j];
      if (dmu_x) dmu_x[ku * du.n + j] = cert_mu[kb * d.w + j];
    } else if (dmu_u) {
      const int i = j - du.n;
      dmu_u[ku * du.m + i] = cert_mu[kb * d.w + d.n + i];
    }
  }
}

}  // namespace ndlqr
