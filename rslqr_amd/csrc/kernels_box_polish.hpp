// kernels_box_polish.hpp -- internal: the active-set polish of a box-constrained batch solve
// (ndlqr_hip_polish_box).
//
// Once ADMM has identified the active set A, the constrained solution solves K z + E_A' mu = b, E_A z = c_A. The polish
// runs the method of multipliers on it: with Q, R shifted by sigma on the entries of A (K~, factored once per round), a
// step is
//     r = (b - E_A' mu) - K z            kkt_residual_dd on the UNSHIFTED Q, R (kernels_refine.hpp), right-hand side bt
//     K~ delta = r                       re-solve against the kept factorisation
//     z+ = z + delta,   mu+_A = mu_A + sigma delta_A,   z+_A = c exactly,   bt+ = b - E_A' mu+
// z_A = c holds for every iterate, so r equals b~(mu) - K~ z with b~ = b + E_A'(sigma c - mu) -- without the roundings of
// sigma c and Q + sigma, which would put a floor of eps sigma |c| under the residual -- and z+_A - c is delta_A. A step is
// a candidate (zc, muc, btc) until its residual norm is known: polish_update commits the previous candidate when
// refine_accepted says so and stops the problem otherwise.
//
// Layouts as in kernels_box.hpp: entries [batch][N][n+m] (codes, mu, v, y; bounds with bstride), vectors [batch][N][2n+m].
// Entry codes: 0 unbounded (the pad entries of a padded shape among them), 1 free, 2 active at the lower bound, 3 active at
// the upper one. Problem states: 0 running, 4 stopped until the round's validation, 1 polished, 2 not polished, 3 not
// finite (1 .. 3 are final and are what the caller gets).
// STRICT: separate mul and add, t = sigma delta, mu+ = mu + t; numpy reproduces every value bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box.hpp"
#include "kernels_common.hpp"
#include "kernels_dd.hpp"

namespace ndlqr {

enum { POLISH_RUNNING = 0, POLISH_DONE = 1, POLISH_KEPT = 2, POLISH_NAN = 3, POLISH_STOPPED = 4 };

// sig[b] = sigma * (largest entry of diag Q, R of problem b over the caller's block sizes; R of the last knot, which is
// not part of the problem, left out). A NaN entry gives a NaN.
//   grid (batch), block 256.
static __global__ __launch_bounds__(256) void polish_sigma(Dims du, Dims d, double sigma, const double* __restrict__ QR,
                                                           double* __restrict__ sig) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned nw = (unsigned)(d.N * d.w);
  const double* qr = QR + (size_t)b * nw;
  double big = 0.0;
  for (unsigned e = tid; e < nw; e += blockDim.x) {
    const unsigned k = e / (unsigned)d.w, j = e - k * (unsigned)d.w;
    const bool used = j < (unsigned)d.n ? j < (unsigned)du.n : (j - d.n < (unsigned)du.m && k + 1 < (unsigned)d.N);
    if (used) big = max_nan(big, qr[e]);
  }
  red[tid] = big;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = max_nan(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) sig[b] = sigma * red[0];
}

// Start of a polish: the resident solution zs saved into z0 and taken as z; codes from the exact comparisons of the ADMM
// iterate with its bounds -- 3: v == hi && y > 0, or lo == hi; 2: v == lo && y < 0; 1: bounded otherwise --; mu = rho y on
// the active entries, 0 elsewhere; bt = b - E_A' mu from the resident right-hand side res; state 3 for a problem whose
// constrained solve ended non-finite, 2 (kept as it is) for one that was certified infeasible (status 4), 0 otherwise
// (counted in *running); no steps yet.
//   grid (N, batch), block 64.
static __global__ void polish_start(Dims d, const double* __restrict__ rhov, const double* __restrict__ lo,
                                    const double* __restrict__ hi, size_t bstride, const double* __restrict__ v,
                                    const double* __restrict__ y, const int* __restrict__ box_status,
                                    const double* __restrict__ res, const double* __restrict__ zs, double* __restrict__ z0,
                                    double* __restrict__ z, unsigned char* __restrict__ code, double* __restrict__ mu,
                                    double* __restrict__ bt, int* __restrict__ state, int* __restrict__ steps,
                                    int* __restrict__ here, int* __restrict__ running) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double rho = rhov[b];
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w,
               ob = (size_t)b * bstride + (size_t)k * d.w;
  if (k == 0 && threadIdx.x == 0) {
    const int bst = box_status[b];
    const bool run = bst != 3 && bst != 4;
    state[b] = run ? POLISH_RUNNING : bst == 3 ? POLISH_NAN : POLISH_KEPT;
    if (run) atomicAdd(running, 1);
    steps[b] = 0;
    here[b] = 0;
  }
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    const double zr = zs[oz + r];
    double rhs = res[oz + r];
    z0[oz + r] = zr;
    z[oz + r] = zr;
    if (r >= d.n) {
      const int j = r - d.n;
      const double l = lo[ob + j], h = hi[ob + j], vj = v[ov + j], yj = y[ov + j];
      unsigned char cd = 0;
      double m = 0.0;
      if (box_bounded(l, h)) {
        cd = ((vj == h && yj > 0.0) || l == h) ? 3 : (vj == l && yj < 0.0) ? 2 : 1;
        if (cd >= 2) {
          m = rho * yj;
          rhs = rhs - m;
        }
      }
      code[ov + j] = cd;
      mu[ov + j] = m;
    }
    bt[oz + r] = rhs;
  }
}

// QR <- QR + sig[b] on the active entries, in place (the caller has saved QR).
//   grid (N, batch), block 64.
static __global__ void polish_shift_qr(Dims d, const double* __restrict__ sig, const unsigned char* __restrict__ code,
                                       double* __restrict__ QR) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double s = sig[b];
  const size_t o = ((size_t)b * d.N + k) * d.w;
  for (int j = threadIdx.x; j < d.w; j += blockDim.x)
    if (code[o + j] >= 2) QR[o + j] = QR[o + j] + s;
}

// Step `step` (1-based) of every running problem, after the re-solve of the residual of slot step - 1 into delta.
// step >= 2: the candidate of step - 1 is committed -- z, mu, bt <- zc, muc, btc, here[b] = step - 1 -- when
// refine_accepted(norms, step - 1) holds; otherwise the problem stops (state 4) with what it has, and the running count
// drops by one. form != 0: the next candidate,
//     zc = z + delta;   on the active entries  muc = mu + sig delta,  zc = c,  btc = res - muc;   elsewhere muc = 0, btc = res
// and a problem whose candidate is not finite ends as state 3 (the reductions keep a NaN). form == 0 (behind the last
// step): the commit alone. One thread owns the same entries in both parts. lo == nullptr (the adjoint): c = 0.
//   grid (batch), block 256.
template <bool STRICT>
__global__ __launch_bounds__(256) void polish_update(Dims d, int step, int form, const unsigned long long* __restrict__ norms,
                                                     const double* __restrict__ sig, const double* __restrict__ lo,
                                                     const double* __restrict__ hi, size_t bstride,
                                                     const unsigned char* __restrict__ code, const double* __restrict__ res,
                                                     const double* __restrict__ delta, double* __restrict__ z,
                                                     double* __restrict__ mu, double* __restrict__ bt, double* __restrict__ zc,
                                                     double* __restrict__ muc, double* __restrict__ btc, int* __restrict__ state,
                                                     int* __restrict__ here, int* __restrict__ running) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (state[b] != POLISH_RUNNING) return;  // (uniform over the workgroup)
  const int rows = d.rows, n = d.n, w = d.w;
  const unsigned nz = (unsigned)(d.N * rows);
  const size_t oz = (size_t)b * nz, ov = (size_t)b * d.N * w;
  if (step >= 2) {
    if (!refine_accepted(norms, d.batch, b, step - 1)) {
      if (tid == 0) {
        state[b] = POLISH_STOPPED;
        atomicSub(running, 1);
      }
      return;
    }
    for (unsigned e = tid; e < nz; e += blockDim.x) {
      const unsigned k = e / (unsigned)rows, r = e - k * (unsigned)rows;
      z[oz + e] = zc[oz + e];
      bt[oz + e] = btc[oz + e];
      if (r >= (unsigned)n) mu[ov + (size_t)k * w + (r - n)] = muc[ov + (size_t)k * w + (r - n)];
    }
    if (tid == 0) here[b] = step - 1;
  }
  if (!form) return;
  const double s = sig[b];
  const double* lb = lo ? lo + (size_t)b * bstride : nullptr;
  const double* hb = lo ? hi + (size_t)b * bstride : nullptr;
  double big = 0.0;
  for (unsigned e = tid; e < nz; e += blockDim.x) {
    const unsigned k = e / (unsigned)rows, r = e - k * (unsigned)rows;
    const double dl = delta[oz + e];
    double zn = z[oz + e] + dl;
    double rhs = res[oz + e];
    if (r >= (unsigned)n) {
      const size_t ev = (size_t)k * w + (r - n);
      const unsigned char cd = code[ov + ev];
      double m = 0.0;
      if (cd >= 2) {
        if constexpr (STRICT) {
          const double t = s * dl;
          m = mu[ov + ev] + t;
        } else {
          m = fma(s, dl, mu[ov + ev]);
        }
        zn = !lo ? 0.0 : cd == 3 ? hb[ev] : lb[ev];
        rhs = rhs - m;
        big = max_nan(big, fabs(m));
      }
      muc[ov + ev] = m;
    }
    zc[oz + e] = zn;
    btc[oz + e] = rhs;
    big = max_nan(big, fabs(zn));
  }
  red[tid] = big;
  __syncthreads();
  for (int t = 128; t > 0; t >>= 1) {
    if (tid < t) red[tid] = max_nan(red[tid], red[tid + t]);
    __syncthreads();
  }
  if (tid == 0 && !isfinite(red[0])) {
    state[b] = POLISH_NAN;
    atomicSub(running, 1);
  }
}

// End of a round, for every problem that is running or stopped: its steps counted, and its last accepted iterate
// validated with exact comparisons -- mu >= 0 where the code is 3 and lo < hi, mu <= 0 where it is 2, lo <= z <= hi on
// every code-1 entry. Valid: state 1 when the round accepted a step, 2 when it did not. Not valid and final != 0: state 2.
// Not valid otherwise: the set is corrected -- a wrong-signed entry is released (code 1, mu = 0), a code-1 entry outside
// its box is fixed at the violated bound (z = that bound, mu = 0), bt = res on both -- and the problem runs again
// (state 0): words[0] counts the running problems, words[1] those whose set changed.
//   grid (batch), block 256.
static __global__ __launch_bounds__(256) void polish_validate(Dims d, int final, const double* __restrict__ lo,
                                                              const double* __restrict__ hi, size_t bstride,
                                                              const double* __restrict__ res, unsigned char* __restrict__ code,
                                                              double* __restrict__ z, double* __restrict__ mu,
                                                              double* __restrict__ bt, int* __restrict__ state,
                                                              int* __restrict__ steps, int* __restrict__ here,
                                                              int* __restrict__ words) {
  __shared__ int bad_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int st = state[b];
  if (st != POLISH_RUNNING && st != POLISH_STOPPED) return;  // (uniform over the workgroup)
  const int rows = d.rows, w = d.w;
  const unsigned nw = (unsigned)(d.N * w);
  const size_t oz = (size_t)b * d.N * rows, ov = (size_t)b * nw;
  const double* lb = lo + (size_t)b * bstride;
  const double* hb = hi + (size_t)b * bstride;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  int bad = 0;
  for (unsigned e = tid; e < nw; e += blockDim.x) {
    const unsigned char cd = code[ov + e];
    if (cd == 0) continue;
    const double l = lb[e], h = hb[e], m = mu[ov + e], zi = z[oz + box_entry_offset(d, e)];
    if (cd == 3) bad |= (l < h && m < 0.0);
    else if (cd == 2) bad |= (m > 0.0);
    else bad |= (zi > h || zi < l);
  }
  if (bad) atomicOr(&bad_s, 1);
  __syncthreads();
  const int invalid = bad_s;
  if (!invalid || final) {
    if (tid == 0) {
      const int took = here[b];
      steps[b] += took;
      here[b] = 0;
      state[b] = (!invalid && took >= 1) ? POLISH_DONE : POLISH_KEPT;
    }
    return;
  }
  for (unsigned e = tid; e < nw; e += blockDim.x) {
    const unsigned char cd = code[ov + e];
    if (cd == 0) continue;
    const size_t at = oz + box_entry_offset(d, e);
    const double l = lb[e], h = hb[e], m = mu[ov + e], zi = z[at];
    unsigned char nc = cd;
    if ((cd == 3 && l < h && m < 0.0) || (cd == 2 && m > 0.0)) nc = 1;
    else if (cd == 1 && zi > h) { nc = 3; z[at] = h; }
    else if (cd == 1 && zi < l) { nc = 2; z[at] = l; }
    if (nc != cd) {
      code[ov + e] = nc;
      mu[ov + e] = 0.0;
      bt[at] = res[at];
    }
  }
  if (tid == 0) {
    steps[b] += here[b];
    here[b] = 0;
    state[b] = POLISH_RUNNING;
    atomicAdd(words, 1);
    atomicAdd(words + 1, 1);
  }
}

// End of a polish: the resident solution zs gets the polished z of the problems in state 1 and the saved z0 of every other
// (the factorisations overwrote it); for state 1 also v <- (x, u) and, on the bounded entries, y <- mu / rho, so that a
// warm-started ADMM begins at the polished point.
//   grid (N, batch), block 64.
static __global__ void polish_finish(Dims d, const double* __restrict__ rhov, const int* __restrict__ state,
                                     const unsigned char* __restrict__ code, const double* __restrict__ z,
                                     const double* __restrict__ mu, const double* __restrict__ z0, double* __restrict__ zs,
                                     double* __restrict__ v, double* __restrict__ y) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w;
  if (state[b] != POLISH_DONE) {
    for (int r = threadIdx.x; r < d.rows; r += blockDim.x) zs[oz + r] = z0[oz + r];
    return;
  }
  const double rho = rhov[b];
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    const double val = z[oz + r];
    zs[oz + r] = val;
    if (r >= d.n) {
      const int j = r - d.n;
      v[ov + j] = val;
      if (code[ov + j] != 0) y[ov + j] = mu[ov + j] / rho;
    }
  }
}

// Start of the adjoint on the polish's system (c = 0, right-hand side the packed g in `rhs`): w = 0, nu = 0, bt = rhs; a
// problem whose polish ended as 1 runs (counted in *running), every other keeps that status and its zeros.
//   grid (N, batch), block 64.
static __global__ void polish_adjoint_start(Dims d, const int* __restrict__ pol_state, const double* __restrict__ rhs,
                                            double* __restrict__ w, double* __restrict__ nu, double* __restrict__ bt,
                                            int* __restrict__ state, int* __restrict__ steps, int* __restrict__ here,
                                            int* __restrict__ running) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w;
  if (k == 0 && threadIdx.x == 0) {
    const bool run = pol_state[b] == POLISH_DONE;
    state[b] = run ? POLISH_RUNNING : pol_state[b];
    if (run) atomicAdd(running, 1);
    steps[b] = 0;
    here[b] = 0;
  }
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    w[oz + r] = 0.0;
    bt[oz + r] = rhs[oz + r];
    if (r >= d.n) nu[ov + r - d.n] = 0.0;
  }
}

// End of the adjoint: a problem that ran reports its accepted steps and status 1 when it accepted one or its right-hand
// side was zero (slot 0 of the norms: w = 0 is then exact), 2 otherwise.
//   grid ceil(batch / 256), block 256.
static __global__ void polish_adjoint_finish(int batch, const unsigned long long* __restrict__ norms, int* __restrict__ state,
                                             int* __restrict__ steps, const int* __restrict__ here) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const int st = state[b];
  if (st != POLISH_RUNNING && st != POLISH_STOPPED) return;
  steps[b] = here[b];
  state[b] = (here[b] >= 1 || refine_norm(norms, batch, 0, b) == 0.0) ? POLISH_DONE : POLISH_KEPT;
}

// Multipliers into the caller's flat layout, as box_multipliers: the polished mu of the problems in state 1, rho y of the
// others.
//   grid (N, batch), block 64.
static __global__ void polish_multipliers(Dims du, Dims d, const double* __restrict__ rhov, const double* __restrict__ y,
                                          const int* __restrict__ state, const double* __restrict__ mu,
                                          double* __restrict__ mu_x, double* __restrict__ mu_u) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double rho = rhov[b];
  const bool done = state[b] == POLISH_DONE;
  const size_t ov = ((size_t)b * d.N + k) * d.w;
  for (int j = threadIdx.x; j < du.n + du.m; j += blockDim.x) {
    const int i = j < du.n ? j : d.n + (j - du.n);
    const double val = done ? mu[ov + i] : rho * y[ov + i];
    if (j < du.n) {
      if (mu_x) mu_x[((size_t)b * du.N + k) * du.n + j] = val;
    } else if (mu_u) {
      mu_u[((size_t)b * du.N + k) * du.m + (j - du.n)] = val;
    }
  }
}

}  // namespace ndlqr
