// kernels_dd.hpp -- internal: double-double accumulation and the norm slots of a refinement, shared by the residual
// kernels (kernels_refine.hpp) and the box kernels that judge a step by them (kernels_box_infeas.hpp,
// kernels_box_polish.hpp). Device functions only: no __global__ kernel lives here.
//
// Compiled with floating-point contraction off, whatever the mode: the error-free transformations need the rounded
// product and the rounded sum. The explicit fma() calls stay fused.
#pragma once
#include <hip/hip_runtime.h>

namespace ndlqr {

// hi + lo: an unevaluated sum, |lo| small against |hi|
struct DD {
  double hi, lo;
};

// acc + p (+ e): TwoSum of hi and p (Knuth), its error and the product's error e go to lo
__device__ __forceinline__ void dd_add(DD& acc, const double p, const double e) {
#pragma clang fp contract(off)
  const double s = acc.hi + p;
  const double bb = s - acc.hi;
  const double es = (acc.hi - (s - bb)) + (p - bb);
  acc.hi = s;
  acc.lo = acc.lo + (e + es);
}
// acc + a * z with the product's rounding error (TwoProd by fma); the plain fp64 size of the term goes to `scale`
__device__ __forceinline__ void dd_fma(DD& acc, double& scale, const double a, const double z) {
#pragma clang fp contract(off)
  const double p = a * z;
  const double e = fma(a, z, -p);
  dd_add(acc, p, e);
  scale = scale + fabs(p);
}
// acc + v (an identity entry of K: the product is exact)
__device__ __forceinline__ void dd_term(DD& acc, double& scale, const double v) {
#pragma clang fp contract(off)
  dd_add(acc, v, 0.0);
  scale = scale + fabs(v);
}

// The norm slots of a refinement: rho = ||r||_inf and the scale max_i (|b_i| + sum_j |K_ij| |z_j|) of every residual
// evaluated so far, as the bit patterns of non-negative doubles (an unsigned maximum of those is the maximum of the
// doubles, and a NaN -- above every finite pattern and infinity -- wins): [2][max_steps + 1][batch], rho first.
// Slot 0 belongs to z as found, slot s to z (+) delta_s.
__device__ __forceinline__ double refine_norm(const unsigned long long* norms, const int batch, const int slot, const int b) {
  return __longlong_as_double((long long)norms[(size_t)slot * batch + b]);
}
// Step s (1-based) is accepted iff rho_t < rho_(t-1) for every t <= s: strict, false for NaN, and a rejection is
// permanent. A pure function of the slots 0 .. s, which earlier launches completed.
__device__ __forceinline__ bool refine_accepted(const unsigned long long* norms, const int batch, const int b, const int s) {
  double prev = refine_norm(norms, batch, 0, b);
  for (int t = 1; t <= s; ++t) {
    const double cur = refine_norm(norms, batch, t, b);
    if (!(cur < prev)) return false;
    prev = cur;
  }
  return true;
}

}  // namespace ndlqr
