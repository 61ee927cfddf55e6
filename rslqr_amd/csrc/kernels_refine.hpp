// kernels_refine.hpp -- internal: iterative refinement of a batch solve with a double-double residual
// (ndlqr_hip_refine, ndlqr_hip_kkt_residual_vector).
//
// The KKT system is K z = b with b the device right-hand side (rhs = -(x_init | d_{k-1}) | -q_k | -r_k) and
//     row lambda_0:      -x_0                                    row x_k:  Q_k x_k - lambda_k + A_k' lambda_{k+1}
//     row lambda_{k+1}:  A_k x_k + B_k u_k - x_{k+1}              row u_k:  R_k u_k + B_k' lambda_{k+1}     (k < N - 1)
// (K is symmetric: kernels_grad.hpp). kkt_residual_dd evaluates r = b - K (z (+) delta) with every row accumulated in
// double-double and rounded once; r has the layout of a right-hand side, so K delta' = r is one more re-solve against the
// kept factorisation, and refine_commit stores z (+) delta for the problems whose residual norm went down.
//
// Everything here is compiled with floating-point contraction off, whatever the mode: the error-free transformations
// need the rounded product and the rounded sum. The explicit fma() calls stay fused. The kernels are therefore the same
// code, bit for bit, under NDLQR_FLAG_STRICT_FP and without it.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"
#include "kernels_dd.hpp"

namespace ndlqr {

// pitch of the [A | B] tile in LDS: odd, so that the rows (lambda rows: thread i reads row i) and the columns (x and u
// rows: thread i reads column i) both spread over the banks
__host__ __device__ inline int refine_tile_pitch(const int w) { return w | 1; }
static inline size_t refine_lds_bytes(const Dims& d, const bool staged) {
  return sizeof(double) * ((staged ? (size_t)d.n * refine_tile_pitch(d.w) : 0) + 2 * (size_t)d.rows);
}

// r = b - K (z (+) delta) in the layout of rhs, per problem ||r||_inf and the scale into slot `slot` of `norms`.
//   delta == nullptr: the residual of z. norms == nullptr: the vector alone.
//   du: the caller's block sizes (rows and columns beyond them -- a padded shape -- are not part of the system: r = 0 there).
//   staged: [A_k | B_k] goes through LDS (one coalesced read serves both products); 0: the tile is beyond the LDS of a
//   workgroup and is read in place.
// Term order of a row: the right-hand-side entry, then the identity and diagonal terms, then j
// ascending (for a lambda row: the columns of A, then those of B).
//   grid (N, batch); block k: the x and u rows of knot k, the lambda rows of knot k + 1, block 0 also those of knot 0.
static __global__ void kkt_residual_dd(Dims du, Dims d, const double* __restrict__ AB, const double* __restrict__ QR,
                                       const double* __restrict__ rhs, const double* __restrict__ z,
                                       const double* __restrict__ delta, double* __restrict__ r,
                                       unsigned long long* __restrict__ norms, const int nslots, const int slot,
                                       const int staged) {
#pragma clang fp contract(off)
  const int k = blockIdx.x, b = blockIdx.y;
  const int n = d.n, N = d.N, rows = d.rows, w = d.w, nu = du.n, mu = du.m;
  // a chain that has already broken: nothing of this problem is looked at again
  if (norms && slot >= 2 && !refine_accepted(norms, d.batch, b, slot - 1)) return;
  extern __shared__ double refine_lds[];
  __shared__ unsigned long long smax[2];
  const bool last = k == N - 1;
  const int wp = staged ? refine_tile_pitch(w) : w;
  double* zk = refine_lds;        // z (+) delta of knot k
  double* zn = zk + rows;         // ... of knot k + 1
  double* tile_lds = zn + rows;
  const size_t kb = (size_t)b * N + k;
  const double* ab = AB + kb * n * w;
  if (threadIdx.x < 2) smax[threadIdx.x] = 0ull;
  for (int e = threadIdx.x; e < (last ? rows : 2 * rows); e += blockDim.x) {
    const size_t at = kb * rows + e;
    zk[e] = delta ? z[at] + delta[at] : z[at];  // (zn follows zk)
  }
  if (staged && !last)
    for (int e = threadIdx.x; e < n * w; e += blockDim.x) {
      const int i = e / w;
      tile_lds[i * wp + (e - i * w)] = ab[e];
    }
  __syncthreads();
  const double* tile = staged ? tile_lds : ab;
  const double* qr = QR + kb * w;
  const double* bk = rhs + kb * rows;
  double* rk = r + kb * rows;
  // tasks: [0, n + m): rows n .. rows - 1 of knot k; [n + m, rows): lambda rows of knot k + 1; block 0: n more, those of knot 0
  const int ntask = rows + (k == 0 ? n : 0);
  // non-negative doubles (or NaN with the sign bit clear): the order of the bit patterns is the order of the values
  unsigned long long pr = 0ull, ps = 0ull;
  for (int t = threadIdx.x; t < ntask; t += blockDim.x) {
    DD acc = {0.0, 0.0};
    double scale = 0.0;
    bool live = true;
    double* out;
    if (t < n) {  // x row i of knot k
      const int i = t;
      out = rk + n + i;
      live = i < nu;
      if (live) {
        acc.hi = bk[n + i];
        scale = fabs(acc.hi);
        dd_term(acc, scale, zk[i]);
        dd_fma(acc, scale, -qr[i], zk[n + i]);
        if (!last)
          for (int j = 0; j < nu; ++j) dd_fma(acc, scale, -tile[j * wp + i], zn[j]);
      }
    } else if (t < n + d.m) {  // u row i of knot k
      const int i = t - n;
      out = rk + 2 * n + i;
      live = i < mu && !last;
      if (live) {
        acc.hi = bk[2 * n + i];
        scale = fabs(acc.hi);
        dd_fma(acc, scale, -qr[n + i], zk[2 * n + i]);
        for (int j = 0; j < nu; ++j) dd_fma(acc, scale, -tile[j * wp + n + i], zn[j]);
      }
    } else if (t < rows) {  // lambda row i of knot k + 1
      const int i = t - n - d.m;
      if (last) continue;
      out = rk + rows + i;
      live = i < nu;
      if (live) {
        acc.hi = bk[rows + i];
        scale = fabs(acc.hi);
        dd_term(acc, scale, zn[n + i]);
        for (int j = 0; j < nu; ++j) dd_fma(acc, scale, -tile[i * wp + j], zk[n + j]);
        for (int j = 0; j < mu; ++j) dd_fma(acc, scale, -tile[i * wp + n + j], zk[2 * n + j]);
      }
    } else {  // lambda row i of knot 0
      const int i = t - rows;
      out = rk + i;
      live = i < nu;
      if (live) {
        acc.hi = bk[i];
        scale = fabs(acc.hi);
        dd_term(acc, scale, zk[n + i]);
      }
    }
    const double v = live ? acc.hi + acc.lo : 0.0;
    *out = v;
    const unsigned long long bv = (unsigned long long)__double_as_longlong(fabs(v));
    const unsigned long long bs = (unsigned long long)__double_as_longlong(fabs(scale));
    pr = bv > pr ? bv : pr;
    ps = bs > ps ? bs : ps;
  }
  if (!norms) return;
  if (pr) atomicMax(&smax[0], pr);
  if (ps) atomicMax(&smax[1], ps);
  __syncthreads();
  if (threadIdx.x < 2 && smax[threadIdx.x])
    atomicMax(norms + ((size_t)threadIdx.x * nslots + slot) * d.batch + b, smax[threadIdx.x]);
}

// z <- z (+) delta for the problems whose step `step` is accepted; everything else keeps its bits.
//   grid (ceil(N rows / 256), batch), block 256.
static __global__ void refine_commit(Dims d, const unsigned long long* __restrict__ norms, const int step,
                                     const double* __restrict__ delta, double* __restrict__ z) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, per = d.N * d.rows;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per || !refine_accepted(norms, d.batch, b, step)) return;
  const size_t at = (size_t)b * per + e;
  z[at] = z[at] + delta[at];
}

// What the caller gets of a refinement of max_steps steps: the steps taken by every problem and eta = rho / scale of its
// residual before and after them (0 where the residual is 0). block 256, one thread per problem.
static __global__ void refine_report(const int batch, const int max_steps, const unsigned long long* __restrict__ norms,
                                     int* __restrict__ steps, double* __restrict__ eta) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  int s = 0;
  while (s < max_steps && refine_accepted(norms, batch, b, s + 1)) ++s;
  const unsigned long long* scale = norms + (size_t)(max_steps + 1) * batch;
  const double r0 = refine_norm(norms, batch, 0, b), r1 = refine_norm(norms, batch, s, b);
  steps[b] = s;
  eta[b] = r0 == 0.0 ? 0.0 : r0 / refine_norm(scale, batch, 0, b);
  eta[batch + b] = r1 == 0.0 ? 0.0 : r1 / refine_norm(scale, batch, s, b);
}

}  // namespace ndlqr
