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

// One ADMM update of the box adjoint for every running problem after re-solve `it`: the shared core of kernels_box.hpp
// (box_step, box_judge, box_tail_frozen) over the entries whose code is not BOX_UNBOUNDED, with its own clip: to [0, 0]
// on the fixed entries, the identity -- not a clip to +-inf, which would drop a NaN -- on the split ones. v holds the
// split entries' projected iterate, y the fixed entries' scaled dual; rho is the forward's final penalty (no adapting).
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
  const double rho = rhov[b];
  const BoxViews V(d, b, z, v, y, res, rhs_cur, rhs_next);
  const unsigned char* cb = code + (size_t)b * V.nw;
  BoxMaxima M;
  for (unsigned e = tid; e < V.nw; e += blockDim.x) {
    const unsigned char c = cb[e];
    if (c == BOX_UNBOUNDED) continue;
    const bool fixed = c != BOX_SPLIT;
    const size_t oz = box_entry_offset(d, e);
    const double zi = V.zb[oz], v0 = fixed ? 0.0 : V.vb[e], y0 = fixed ? V.yb[e] : 0.0;
    const BoxStep s = box_step<STRICT>(P, zi, v0, y0, fixed, 0.0, 0.0);
    if (fixed) V.yb[e] = s.yn;
    else V.vb[e] = s.vn;  // (yn is +0 exactly: y of a split entry is never stored)
    V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], s.vn, s.yn, rho);
    M.note(zi, v0, s.vn, s.yn);
  }
  M.reduce(red, tid);
  if (tid == 0) conv_s = box_judge(P, rho, red, b, it, status, iters, resid, running).frozen;
  __syncthreads();
  if (conv_s) box_tail_frozen(d, V, tid, [=](unsigned e) { return cb[e] != BOX_UNBOUNDED; });
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
