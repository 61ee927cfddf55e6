// kernels_box_grad.hpp -- internal: gradients through the box-constrained batch solve (ndlqr_hip_solve_box_adjoint,
// ndlqr_hip_bound_gradients).
//
// At the constrained solution z* with the active set A (the bounded entries whose projected iterate v lies exactly on a
// bound), the adjoint of a loss L(z*) with g = dL/dz* is the equality-constrained system
//     K w + E_A' nu = g,   E_A w = 0,
// solved as one more box-constrained problem by the ADMM of kernels_box.hpp on the forward's kept shifted factorisation
// (same rho per problem, same M): right-hand side g, lo = hi = 0 on A. The entries of M \ A carry the rho shift of that factorisation,
// so they stay in the splitting as free entries: bounded, but their clip is the identity (y stays 0). Every entry gets a
// byte code from the forward's v once:
//     BOX_UNBOUNDED 0   not in M: untouched by the iteration (right-hand side as packed, w = z)
//     BOX_SPLIT     1   in M, strictly inside its bounds: v+ = zh + y with y = 0, so y stays 0 and is never stored
//     BOX_AT_LO     2   in M, v == lo: fixed at 0 -- v stays 0 and is never stored
//     BOX_AT_HI     3   in M, v == hi (lo == hi reports here): as BOX_AT_LO
// which is box_update with those bounds, operation for operation (STRICT: numpy reproduces every value bit for bit), with
// 41 B per bounded entry instead of 72 B: z, code, the resident right-hand side and one of v / y read, that one and the next
// right-hand side written -- lo and hi are not read. nu = rho y; dL/dc_A = nu goes to dL/dhi of BOX_AT_HI entries and to
// dL/dlo of BOX_AT_LO ones, 0 everywhere else.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box.hpp"
#include "kernels_common.hpp"

namespace ndlqr {

enum : unsigned char { BOX_UNBOUNDED = 0, BOX_SPLIT = 1, BOX_AT_LO = 2, BOX_AT_HI = 3 };

// Start of a box adjoint: the codes from the forward's v (vf) and bounds, v = y = 0, both ADMM right-hand sides from the
// packed g (res, the adjoint's resident right-hand side); status and iteration count of every problem -- 3 or 4 (not
// iterated) where the forward ended so, else 0 and one more in the running count.
//   grid (N, batch), block 64.
template <bool STRICT>
__global__ void box_adjoint_start(Dims d, const double* __restrict__ rhov, const double* __restrict__ lo,
                                  const double* __restrict__ hi, size_t bstride, const double* __restrict__ vf, const int* __restrict__ fstatus,
                                  const double* __restrict__ res, unsigned char* __restrict__ code, double* __restrict__ v,
                                  double* __restrict__ y, double* __restrict__ rhs0, double* __restrict__ rhs1,
                                  int* __restrict__ status, int* __restrict__ iters, int* __restrict__ running) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double rho = rhov[b];
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w,
               ob = (size_t)b * bstride + (size_t)k * d.w;
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    double val = res[oz + r];
    if (r >= d.n) {
      const int j = r - d.n;
      const double l = lo[ob + j], h = hi[ob + j], vv = vf[ov + j];
      const unsigned char c = !box_bounded(l, h) ? BOX_UNBOUNDED : vv == h ? BOX_AT_HI : vv == l ? BOX_AT_LO : BOX_SPLIT;
      code[ov + j] = c;
      v[ov + j] = 0.0;
      y[ov + j] = 0.0;
      if (c != BOX_UNBOUNDED) val = box_rhs_entry<STRICT>(val, 0.0, 0.0, rho);
    }
    rhs0[oz + r] = val;
    rhs1[oz + r] = val;
  }
  if (k == 0 && threadIdx.x == 0) {
    const int fs = fstatus[b];
    const int st = (fs == 3 || fs == 4) ? fs : 0;
    status[b] = st;
    iters[b] = 0;
    if (st == 0) atomicAdd(running, 1);
  }
}

// One ADMM update of the box adjoint for every running problem after re-solve `it`: box_update (kernels_box.hpp) with
// lo = hi = 0 on the fixed entries and the identity for the clip of the split ones -- same convergence test, freezing,
// NaN handling and running count. v holds the split entries' projected iterate, y the fixed entries' scaled dual.
//   grid (batch), block 256.
template <bool STRICT>
__global__ __launch_bounds__(256) void box_adjoint_update(Dims d, int it, BoxParams P, const double* __restrict__ z,
                                                          const unsigned char* __restrict__ code, double* __restrict__ v,
                                                          double* __restrict__ y, const double* __restrict__ res,
                                                          const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                          const double* __restrict__ rhov, int* __restrict__ status,
                                                          int* __restrict__ iters, double* __restrict__ resid,
                                                          int* __restrict__ running) {
  __shared__ double red[5][256];
  __shared__ int conv_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const double rho = rhov[b];  // (the forward's final penalty of this problem: the adjoint does not adapt)
  const int w = d.w, n = d.n, rows = d.rows;
  const unsigned nw = (unsigned)(d.N * w);
  const unsigned char* cb = code + (size_t)b * nw;
  double* vb = v + (size_t)b * nw;
  double* yb = y + (size_t)b * nw;
  const double* zb = z + (size_t)b * d.N * rows;
  const double* rs = res + (size_t)b * d.N * rows;
  const double* rc = rhs_cur + (size_t)b * d.N * rows;
  double* rn = rhs_next + (size_t)b * d.N * rows;
  double rp = 0.0, rd = 0.0, zm = 0.0, vm = 0.0, ym = 0.0;
  for (unsigned e = tid; e < nw; e += blockDim.x) {
    const unsigned char c = cb[e];
    if (c == BOX_UNBOUNDED) continue;
    const bool fixed = c != BOX_SPLIT;
    const unsigned k = e / (unsigned)w, j = e - k * (unsigned)w;
    const size_t oz = (size_t)k * rows + n + j;
    const double zi = zb[oz];
    const double v0 = fixed ? 0.0 : vb[e], y0 = fixed ? yb[e] : 0.0;
    double zh;
    if constexpr (STRICT) {
      const double a = P.alpha * zi;
      const double cc = P.oma * v0;
      zh = a + cc;
    } else {
      zh = fma(P.alpha, zi, P.oma * v0);
    }
    const double t = zh + y0;
    const double vn = fixed ? fmin(fmax(t, 0.0), 0.0) : t;
    const double yn = (y0 + zh) - vn;
    if (fixed) yb[e] = yn;
    else vb[e] = vn;  // (yn is +0 exactly: y of a split entry is never stored)
    rn[oz] = box_rhs_entry<STRICT>(rs[oz], vn, yn, rho);
    rp = max_nan(rp, fabs(zi - vn));
    rd = max_nan(rd, fabs(vn - v0));
    zm = max_nan(zm, fabs(zi));
    vm = max_nan(vm, fabs(vn));
    ym = max_nan(ym, fabs(yn));
  }
  red[0][tid] = rp; red[1][tid] = rd; red[2][tid] = zm; red[3][tid] = vm; red[4][tid] = ym;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int q = 0; q < 5; ++q) red[q][tid] = max_nan(red[q][tid], red[q][tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    const double r_prim = red[0][0], r_dual = rho * red[1][0];
    const double sp = max_nan(red[2][0], red[3][0]), sd = rho * red[4][0];
    const double tol_p = P.eps_abs + P.eps_rel * sp;
    const double tol_d = P.eps_abs + P.eps_rel * sd;
    const bool finite = isfinite(r_prim) && isfinite(r_dual) && isfinite(red[2][0]) && isfinite(red[3][0]) &&
                        isfinite(red[4][0]);
    const int conv = finite && r_prim <= tol_p && r_dual <= tol_d;
    iters[b] = it;
    resid[4 * (size_t)b] = r_prim;  // the read-out (ndlqr_CopyBatchBoxAdjointResiduals)
    resid[4 * (size_t)b + 1] = r_dual;
    resid[4 * (size_t)b + 2] = sp;
    resid[4 * (size_t)b + 3] = sd;
    if (conv || !finite) {
      status[b] = conv ? 1 : 3;
      atomicSub(running, 1);
    }
    conv_s = conv || !finite;
  }
  __syncthreads();
  if (!conv_s) return;
  for (unsigned e = tid; e < nw; e += blockDim.x) {  // frozen: the next right-hand side is the current one
    if (cb[e] == BOX_UNBOUNDED) continue;
    const unsigned k = e / (unsigned)w, j = e - k * (unsigned)w;
    const size_t oz = (size_t)k * rows + n + j;
    rn[oz] = rc[oz];
  }
}

// End of a box adjoint, in place on the adjoint solution z (the last re-solve): x, u of the bounded entries become v
// (0 on the fixed ones); lambda and the unbounded entries stay as the re-solve left them. A problem whose forward was
// certified infeasible (status 4) has no solution to differentiate: w = 0 (its nu = rho y is 0 from the start).
//   grid (N, batch), block 64.
static __global__ void box_adjoint_finish(Dims d, const unsigned char* __restrict__ code, const double* __restrict__ v,
                                          const int* __restrict__ status, double* __restrict__ z) {
  const int k = blockIdx.x, b = blockIdx.y;
  if (status[b] == 4) {
    for (int r = threadIdx.x; r < d.rows; r += blockDim.x) z[((size_t)b * d.N + k) * d.rows + r] = 0.0;
    return;
  }
  const size_t oz = ((size_t)b * d.N + k) * d.rows + d.n, ov = ((size_t)b * d.N + k) * d.w;
  for (int j = threadIdx.x; j < d.w; j += blockDim.x)
    if (code[ov + j] != BOX_UNBOUNDED) z[oz + j] = v[ov + j];
}

// Destinations of the bound gradients: dL/d(xlo, xhi, ulo, uhi), nullptr = not computed.
struct BoundOut {
  double* p[4];
};

// nu of entry j (caller's block sizes: x then u) of knot k of problem b split onto its lower and upper bound
__device__ __forceinline__ void bound_grad_entry(const Dims& du, const Dims& d, const double* rhov, const unsigned char* code,
                                                 const double* y, int b, int k, int j, double* glo, double* ghi) {
  const double rho = rhov[b];
  const int jd = j < du.n ? j : d.n + (j - du.n);
  const size_t ov = ((size_t)b * d.N + k) * d.w + jd;
  const unsigned char c = code[ov];
  const double nu = c >= BOX_AT_LO ? rho * y[ov] : 0.0;
  *glo = c == BOX_AT_LO ? nu : 0.0;
  *ghi = c == BOX_AT_HI ? nu : 0.0;
}

__device__ __forceinline__ void bound_grad_put(const Dims& du, const BoundOut& out, size_t p, int k, int j, double glo,
                                               double ghi) {
  if (j < du.n) {
    const size_t o = (p * du.N + k) * du.n + j;
    if (out.p[0]) out.p[0][o] = glo;
    if (out.p[1]) out.p[1][o] = ghi;
  } else {
    const size_t o = (p * du.N + k) * du.m + (j - du.n);
    if (out.p[2]) out.p[2][o] = glo;
    if (out.p[3]) out.p[3][o] = ghi;
  }
}

// Per-problem bound gradients in the caller's flat layout ([batch][N][n], [batch][N][m]).
//   grid (N, batch), block 64.
static __global__ void box_bound_grads(Dims du, Dims d, const double* __restrict__ rho, const unsigned char* __restrict__ code,
                                       const double* __restrict__ y, BoundOut out) {
  const int k = blockIdx.x, b = blockIdx.y;
  for (int j = threadIdx.x; j < du.n + du.m; j += blockDim.x) {
    double glo, ghi;
    bound_grad_entry(du, d, rho, code, y, b, k, j, &glo, &ghi);
    bound_grad_put(du, out, (size_t)b, k, j, glo, ghi);
  }
}

// Batch sums of the bound gradients: entry e = k (n+m) + j of [N][n+m], one thread each, over problems [p0, p1) of split
// blockIdx.y in order. nsplit == 1 (part == nullptr): straight into the outputs ([N][n], [N][m]); else into
// part[split][2][N (n+m)] (lower | upper), which box_bound_sum_splits adds up in order. Deterministic, no atomics.
//   grid (ceil(N (n+m) / 256), nsplit), block 256.
static __global__ __launch_bounds__(256) void box_bound_grads_sum(Dims du, Dims d, const double* __restrict__ rho, int ppb,
                                                                  const unsigned char* __restrict__ code,
                                                                  const double* __restrict__ y, BoundOut out,
                                                                  double* __restrict__ part) {
  const int W = du.n + du.m;
  const size_t E = (size_t)du.N * W;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int k = (int)(e / W), j = (int)(e - (size_t)k * W);
  const int p0 = blockIdx.y * ppb, p1 = (p0 + ppb < du.batch) ? p0 + ppb : du.batch;
  double slo = 0.0, shi = 0.0;
  for (int p = p0; p < p1; ++p) {
    double glo, ghi;
    bound_grad_entry(du, d, rho, code, y, p, k, j, &glo, &ghi);
    slo += glo;
    shi += ghi;
  }
  if (part) {
    part[(size_t)blockIdx.y * 2 * E + e] = slo;
    part[(size_t)blockIdx.y * 2 * E + E + e] = shi;
  } else {
    bound_grad_put(du, out, 0, k, j, slo, shi);
  }
}

// Second stage of a split batch sum: the splits of entry e added in order.
//   grid ceil(N (n+m) / 256), block 256.
static __global__ __launch_bounds__(256) void box_bound_sum_splits(Dims du, int nsplit, const double* __restrict__ part,
                                                                   BoundOut out) {
  const int W = du.n + du.m;
  const size_t E = (size_t)du.N * W;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double slo = 0.0, shi = 0.0;
  for (int s = 0; s < nsplit; ++s) {
    slo += part[(size_t)s * 2 * E + e];
    shi += part[(size_t)s * 2 * E + E + e];
  }
  const int k = (int)(e / W), j = (int)(e - (size_t)k * W);
  bound_grad_put(du, out, 0, k, j, slo, shi);
}

}  // namespace ndlqr
