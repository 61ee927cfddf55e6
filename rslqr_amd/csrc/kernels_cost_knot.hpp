// kernels_cost_knot.hpp -- the per-knot pieces of the dense-cost reduction that more than one
// kernel header uses: the record layout, the triangular solves of one wavefront in LDS, and the bodies of S and S' on
// one knot's staged record. kernels_cost.hpp (cost_apply, cost_apply_t), kernels_lin.hpp (lin_update, lin_finish) and
// kernels_lin_grad.hpp (lin_adjoint_start) call them; no __global__ kernel lives here.
#pragma once
#include "kernels_common.hpp"

namespace ndlqr {

// doubles of one knot's record: L [n][n] | L_R [m][m] | G [m][n], each column-major, the triangles with zeros above
__host__ __device__ inline size_t cost_record_doubles(int n, int m) { return (size_t)n * n + (size_t)m * m + (size_t)m * n; }
// leading dimension of a triangular factor staged in LDS: odd, so that walking a row is as conflict-free as walking a column
__host__ __device__ inline int cost_ld(int k) { return k | 1; }
// v <- L^-1 v (k entries in LDS, L lower with leading dimension ld) by one wavefront: the dependent chain, a column per step
__device__ inline void cost_trsv_lower(const double* L, const int ld, const int k, double* v, const int lane) {
  for (int j = 0; j < k; ++j) {
    const double xj = v[j] / L[j + ld * j];
    if (lane == 0) v[j] = xj;
    for (int i = j + 1 + lane; i < k; i += 64) v[i] = fma(-L[i + ld * j], xj, v[i]);
    wave_lds_sync();
  }
}
// v <- L^-T v
__device__ inline void cost_trsv_lower_t(const double* L, const int ld, const int k, double* v, const int lane) {
  for (int j = k - 1; j >= 0; --j) {
    const double xj = v[j] / L[j + ld * j];
    if (lane == 0) v[j] = xj;
    for (int i = lane; i < j; i += 64) v[i] = fma(-L[j + ld * i], xj, v[i]);
    wave_lds_sync();
  }
}

// a knot's record into LDS: L (leading dimension cost_ld(n)), and with `rest` L_R (cost_ld(m)) and G [m][n]
__device__ inline void cost_stage_record(const double* __restrict__ rk, const int n, const int m, const bool rest, double* sL,
                                         double* sLR, double* sG, const int lane) {
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  for (int idx = lane; idx < n * n; idx += 64) {
    const int j = idx / n;
    sL[idx - j * n + ldn * j] = rk[idx];
  }
  if (!rest) return;
  rk += (size_t)n * n;
  for (int idx = lane; idx < m * m; idx += 64) {
    const int j = idx / m;
    sLR[idx - j * m + ldm * j] = rk[idx];
  }
  rk += (size_t)m * m;
  for (int idx = lane; idx < m * n; idx += 64) sG[idx] = rk[idx];
}

// S' on one knot whose record is staged (sL, and with !last sLR, sG) and whose right-hand-side rows are staged in sl
// (lambda rows; LAMBDA only), sx (x rows) and su (u rows; !last): ol = L' sl, sx <- L^-1 (sx - G' su), su <- L_R^-1 su in
// LDS; STORE: ox, ou receive them. One wavefront; the caller has synchronised the staging.
template <bool LAMBDA, bool STORE>
__device__ __forceinline__ void cost_knot_St(const int n, const int m, const bool last, const double* sL, const double* sLR,
                                             const double* sG, const double* sl, double* sx, double* su, double* ol, double* ox,
                                             double* ou, const int lane) {
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  for (int i = lane; i < n; i += 64) {
    if constexpr (LAMBDA) {
      double s = 0.0;
      for (int c = i; c < n; ++c) s = fma(sL[c + ldn * i], sl[c], s);
      ol[i] = s;
    }
    if (!last) {
      double t = sx[i];
      for (int c = 0; c < m; ++c) t = fma(-sG[c + m * i], su[c], t);
      sx[i] = t;
    }
  }
  wave_lds_sync();
  cost_trsv_lower(sL, ldn, n, sx, lane);
  if constexpr (STORE)
    for (int i = lane; i < n; i += 64) ox[i] = sx[i];
  if (!last) {
    cost_trsv_lower(sLR, ldm, m, su, lane);
    if constexpr (STORE)
      for (int i = lane; i < m; i += 64) ou[i] = su[i];
  }
}

// S on one knot whose record and reduced solution rows are staged as above: ol = L sl (LAMBDA only), sx <- L^-T sx in LDS
// and into ox, and with !last su <- L_R^-T su in LDS, ou = su - G sx. ox, ou may be LDS or global memory.
template <bool LAMBDA>
__device__ __forceinline__ void cost_knot_S(const int n, const int m, const bool last, const double* sL, const double* sLR,
                                            const double* sG, const double* sl, double* sx, double* su, double* ol, double* ox,
                                            double* ou, const int lane) {
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  if constexpr (LAMBDA)
    for (int i = lane; i < n; i += 64) {
      double s = 0.0;
      for (int c = 0; c <= i; ++c) s = fma(sL[i + ldn * c], sl[c], s);
      ol[i] = s;
    }
  cost_trsv_lower_t(sL, ldn, n, sx, lane);
  for (int i = lane; i < n; i += 64) ox[i] = sx[i];
  if (last) return;
  cost_trsv_lower_t(sLR, ldm, m, su, lane);
  for (int j = lane; j < m; j += 64) {
    double s = su[j];
    for (int i = 0; i < n; ++i) s = fma(-sG[j + m * i], sx[i], s);
    ou[j] = s;
  }
}

}  // namespace ndlqr
