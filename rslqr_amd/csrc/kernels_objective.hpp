// kernels_objective.hpp -- the objective value of every problem at its resident solution and its stage costs
// (ndlqr_hip_objective):
//     J_b = sum_{k<N} l_k,   l_k = 1/2 x_k'Q_k x_k + x_k'H_k u_k + 1/2 u_k'R_k u_k + q_k'x_k + r_k'u_k
// with the last knot contributing 1/2 x'Qx + q'x alone (its H, R, r are not part of the problem and are never read) and no
// constant term. Two forms of the stage cost, one finish:
//   objective_diag   diagonal weights in the device layout: QR, the negated right-hand side and z with the pitches of the
//                    device block sizes `d`, the sums over the caller's `u` -- the dummy states and inputs of a zero-padded
//                    block size and the tail knots of a padded horizon never enter. In dense-cost mode with z in the reduced
//                    variables the same kernel on the reduced problem (weights 1) IS the caller's objective:
//                    with xi = L'x, nu = L_R'(u + G x), q~ = L^-1 (q - G'r), r~ = L_R^-1 r the stage cost equals
//                    1/2 |xi|^2 + 1/2 |nu|^2 + q~'xi + r~'nu exactly.
//   objective_dense  dense Q, H, R, q, r in the caller's flat layout (column-major per knot) and z in the caller's
//                    variables: the lower triangles of Q and R alone are read.
//   objective_finish one wavefront per problem adds the knots' partials in an order that N alone fixes and rounds J and
//                    every l_k once.
// Every product's rounding error is captured (fma) and every sum runs in double-double (kernels_dd.hpp); a knot's terms
// are added in the order of its entries by one thread, whatever the launch shape: the bits depend on z and the inputs
// alone. No atomics.
#pragma once
#include "kernels_common.hpp"
#include "kernels_dd.hpp"

namespace ndlqr {

constexpr int kObjKnots = 16;     // knots of a workgroup's chunk
constexpr int kObjThreads = 256;  // workgroup size of the stage kernels

// dynamic LDS (doubles) of the two stage kernels at the caller's w = n + m
__host__ __device__ constexpr size_t objective_diag_lds(int w) { return 2 * (size_t)kObjKnots * w; }
__host__ __device__ constexpr size_t objective_dense_lds(int w) { return 3 * (size_t)kObjKnots * w; }

// s * v for a double-double s: the product of the high part exactly, that of the low part rounded
__device__ __forceinline__ DD obj_scale(const DD s, const double v) {
  const double p = s.hi * v;
  return DD{p, fma(s.lo, v, fma(s.hi, v, -p))};
}

// The terms of a chunk are in LDS, thi | tlo [w][kObjKnots]: thread kk adds those of knot k0 + kk in the order of the
// entries and writes the knot's partial, part [batch][N][2] = hi | lo.
__device__ __forceinline__ void obj_knot_sums(const double* thi, const double* tlo, const int w, const int nk, const size_t knot0,
                                              double* __restrict__ part) {
  const int kk = threadIdx.x;
  if (kk >= nk) return;
  DD acc = {0.0, 0.0};
  for (int i = 0; i < w; ++i) dd_add(acc, thi[i * kObjKnots + kk], tlo[i * kObjKnots + kk]);
  part[2 * (knot0 + kk)] = acc.hi;
  part[2 * (knot0 + kk) + 1] = acc.lo;
}

//   grid (ceil(u.N / kObjKnots), batch), block kObjThreads, dynamic LDS objective_diag_lds(u.w) doubles
static __global__ void __launch_bounds__(kObjThreads)
objective_diag(const Dims u, const Dims d, const double* __restrict__ QR, const double* __restrict__ rhs,
               const double* __restrict__ z, double* __restrict__ part) {
  extern __shared__ double obj_lds[];
  const int w = u.w, b = blockIdx.y, k0 = blockIdx.x * kObjKnots;
  const int nk = u.N - k0 < kObjKnots ? u.N - k0 : kObjKnots;
  double* thi = obj_lds;
  double* tlo = obj_lds + (size_t)kObjKnots * w;
  for (int e = threadIdx.x; e < nk * w; e += kObjThreads) {
    const int kk = e / w, i = e - kk * w, k = k0 + kk;
    DD t = {0.0, 0.0};
    if (i < u.n || k < u.N - 1) {  // (the last knot has no input)
      const int col = i < u.n ? i : d.n + (i - u.n);  // place in Q | R and, behind the n leading entries, in a block of rhs and z
      const size_t knot = (size_t)b * d.N + k;
      const double v = z[knot * d.rows + d.n + col];
      const double half = 0.5 * QR[knot * d.w + col];
      const double lin = -rhs[knot * d.rows + d.n + col];
      double scale = 0.0;
      const double p = v * v, e2 = fma(v, v, -p);
      dd_fma(t, scale, half, p);
      t.lo = fma(half, e2, t.lo);
      dd_fma(t, scale, lin, v);
    }
    thi[i * kObjKnots + kk] = t.hi;
    tlo[i * kObjKnots + kk] = t.lo;
  }
  __syncthreads();
  obj_knot_sums(thi, tlo, w, nk, (size_t)b * u.N + k0, part);
}

// Q [batch][N][n*n], H [batch][N][n*m] (null: zero), R [batch][N][m*m], q [batch][N][n], r [batch][N][m]: the caller's flat
// layout, column-major per knot; z in the caller's variables with the pitches of `d`. Entry i of knot k takes row i of the
// lower triangle:  x_i (1/2 Q_ii x_i + sum_{j<i} Q_ij x_j + sum_j H_ij u_j + q_i),  u_i (1/2 R_ii u_i + sum_{j<i} R_ij u_j + r_i).
//   grid (ceil(u.N / kObjKnots), batch), block kObjThreads, dynamic LDS objective_dense_lds(u.w) doubles
static __global__ void __launch_bounds__(kObjThreads)
objective_dense(const Dims u, const Dims d, const double* __restrict__ Q, const double* __restrict__ H,
                const double* __restrict__ R, const double* __restrict__ q, const double* __restrict__ r,
                const double* __restrict__ z, double* __restrict__ part) {
  extern __shared__ double obj_lds[];
  const int n = u.n, m = u.m, w = u.w, b = blockIdx.y, k0 = blockIdx.x * kObjKnots;
  const int nk = u.N - k0 < kObjKnots ? u.N - k0 : kObjKnots;
  double* thi = obj_lds;
  double* tlo = obj_lds + (size_t)kObjKnots * w;
  double* xu = obj_lds + 2 * (size_t)kObjKnots * w;  // [kObjKnots][w]: x | u of every knot of the chunk
  for (int e = threadIdx.x; e < nk * w; e += kObjThreads) {
    const int kk = e / w, i = e - kk * w, k = k0 + kk;
    const int col = i < n ? i : d.n + (i - n);
    xu[e] = (i < n || k < u.N - 1) ? z[((size_t)b * d.N + k) * d.rows + d.n + col] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nk * w; e += kObjThreads) {
    const int kk = e / w, i = e - kk * w, k = k0 + kk;
    const size_t knot = (size_t)b * u.N + k;
    const double* xk = xu + (size_t)kk * w;
    const double* uk = xk + n;
    const bool last = k == u.N - 1;
    DD t = {0.0, 0.0};
    double scale = 0.0;
    if (i < n) {
      const double* Qk = Q + knot * n * n;
      DD s = {0.0, 0.0};
      for (int j = 0; j < i; ++j) dd_fma(s, scale, Qk[i + (size_t)n * j], xk[j]);
      dd_fma(s, scale, 0.5 * Qk[i + (size_t)n * i], xk[i]);
      if (H && !last) {
        const double* Hk = H + knot * n * m;
        for (int j = 0; j < m; ++j) dd_fma(s, scale, Hk[i + (size_t)n * j], uk[j]);
      }
      dd_add(s, q[knot * n + i], 0.0);
      t = obj_scale(s, xk[i]);
    } else if (!last) {
      const int iu = i - n;
      const double* Rk = R + knot * m * m;
      DD s = {0.0, 0.0};
      for (int j = 0; j < iu; ++j) dd_fma(s, scale, Rk[iu + (size_t)m * j], uk[j]);
      dd_fma(s, scale, 0.5 * Rk[iu + (size_t)m * iu], uk[iu]);
      dd_add(s, r[knot * m + iu], 0.0);
      t = obj_scale(s, uk[iu]);
    }
    thi[i * kObjKnots + kk] = t.hi;
    tlo[i * kObjKnots + kk] = t.lo;
  }
  __syncthreads();
  obj_knot_sums(thi, tlo, w, nk, (size_t)b * u.N + k0, part);
}

// part [batch][N][2] -> J [batch] and, where asked for, stage [batch][N], every l_k and J rounded once. Lane l adds the
// partials of the knots l, l + 64, l + 128, ... in increasing order (whole lines in), lane 0 then adds the sixty-four lane
// sums in lane order: up to 64 knots that is the knot order, beyond it an order that N alone fixes. (One lane adding all of
// them in knot order measured 0.24 ms at N = 8192, 2.6 solves of that shape: DESIGN.md section 3.24.)
//   grid (batch), block 64
static __global__ void __launch_bounds__(64)
objective_finish(const int N, const double* __restrict__ part, double* __restrict__ J, double* __restrict__ stage) {
  __shared__ double shi[64], slo[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* pb = part + 2 * (size_t)b * N;
  DD acc = {0.0, 0.0};
  for (int k = lane; k < N; k += 64) {
    const double hi = pb[2 * (size_t)k], lo = pb[2 * (size_t)k + 1];
    if (stage) stage[(size_t)b * N + k] = hi + lo;
    dd_add(acc, hi, lo);
  }
  shi[lane] = acc.hi;
  slo[lane] = acc.lo;
  __syncthreads();
  if (lane == 0) {
    DD total = {0.0, 0.0};
    for (int j = 0; j < 64; ++j) dd_add(total, shi[j], slo[j]);
    J[b] = total.hi + total.lo;
  }
}

}  // namespace ndlqr
