// kernels_lin_shift.hpp -- internal: the body lin_shift_cost (kernels_lin.hpp, the ADMM's penalties) and
// lin_polish_shift_cost (kernels_lin_polish.hpp, the polish's sigma on the active rows) share. Device functions only: no
// __global__ kernel lives here.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace ndlqr {

__host__ __device__ inline size_t lin_shift_lds(int n, int m, int p) { return (size_t)p * n + (size_t)p * m + p; }

// Q^ = Q + C'WC, H^ = H + C'WD, R^ = R + D'WD of knot k of problem b, W = diag(weight(r)) over the knot's p rows (the last
// knot: Q^ alone; H^ = 0, R^ = 1 are written and nothing of the caller's H, R, D is loaded there). One wavefront; C, D and
// the row weights go through LDS (lin_shift_lds(n, m, p) doubles), the costs come in and leave as they lie. Q, R are read
// in their lower triangles (as cost_factor does) and leave symmetric. H may be null (zero).
template <class Weight>
__device__ __forceinline__ void lin_shift_cost_knot(double* lds, const int n, const int m, const int N, const int p, const int k,
                                                    const int b, const Weight& weight, const double* __restrict__ Q,
                                                    const double* __restrict__ H, const double* __restrict__ R,
                                                    const double* __restrict__ C, const double* __restrict__ D,
                                                    double* __restrict__ Qs, double* __restrict__ Hs, double* __restrict__ Rs,
                                                    const int lane) {
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  double* sC = lds;
  double* sD = sC + (size_t)p * n;
  double* sw = sD + (size_t)p * m;
  {
    const double* Ck = C + kb * p * n;
    for (int idx = lane; idx < p * n; idx += 64) sC[idx] = Ck[idx];
    if (!last) {
      const double* Dk = D + kb * p * m;
      for (int idx = lane; idx < p * m; idx += 64) sD[idx] = Dk[idx];
    }
    for (int r = lane; r < p; r += 64) sw[r] = weight(r);
  }
  wave_lds_sync();
  {
    const double* Qk = Q + kb * n * n;
    double* Qo = Qs + kb * n * n;
    for (int idx = lane; idx < n * n; idx += 64) {
      const int j = idx / n, i = idx - j * n;
      double s = 0.0;
      for (int r = 0; r < p; ++r) s = fma(sC[r + p * i] * sw[r], sC[r + p * j], s);
      Qo[idx] = (i >= j ? Qk[idx] : Qk[j + n * i]) + s;
    }
  }
  double* Ho = Hs + kb * n * m;
  double* Ro = Rs + kb * m * m;
  if (last) {
    for (int idx = lane; idx < n * m; idx += 64) Ho[idx] = 0.0;
    for (int idx = lane; idx < m * m; idx += 64) Ro[idx] = (idx / m == idx % m) ? 1.0 : 0.0;
    return;
  }
  const double* Hk = H ? H + kb * n * m : nullptr;
  for (int idx = lane; idx < n * m; idx += 64) {
    const int j = idx / n, i = idx - j * n;
    double s = 0.0;
    for (int r = 0; r < p; ++r) s = fma(sC[r + p * i] * sw[r], sD[r + p * j], s);
    Ho[idx] = (Hk ? Hk[idx] : 0.0) + s;
  }
  const double* Rk = R + kb * m * m;
  for (int idx = lane; idx < m * m; idx += 64) {
    const int j = idx / m, i = idx - j * m;
    double s = 0.0;
    for (int r = 0; r < p; ++r) s = fma(sD[r + p * i] * sw[r], sD[r + p * j], s);
    Ro[idx] = (i >= j ? Rk[idx] : Rk[j + m * i]) + s;
  }
}

}  // namespace ndlqr
