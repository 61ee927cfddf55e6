// kernels_lin_grad.hpp -- internal: gradients through the solve with linear inequality constraints
// (ndlqr_hip_solve_constrained_adjoint, ndlqr_hip_constraint_gradients).
//
// At the constrained solution z* with the active set A (the bounded rows whose projected iterate v lies exactly on a
// bound) and G = [C D], the adjoint of a loss L(z*) with g = dL/dz* is the equality-constrained system
//     K w + G_A' nu = g,   G_A w = 0,
// solved as section 3.10 solves the box case: by the ADMM of kernels_lin.hpp on the forward's remembered SHIFTED
// reduction and factorisation (same rho[batch] -- the vector the forward ended with, which nothing here moves --, same M), right-hand side S^' g, lo = hi = 0 on A. The rows of M \ A carry the
// rho shift of that factorisation, so they stay in the splitting as free rows: bounded, but their clip is the identity
// (y stays 0). Every row gets a byte code from the forward's v once -- the codes of box_adjoint_start:
//     LIN_UNBOUNDED 0   not in M: no part of the iteration
//     LIN_FREE      1   in M, strictly inside its bounds
//     LIN_AT_LO     2   in M, v == lo: fixed at 0
//     LIN_AT_HI     3   in M, v == hi (lo == hi reports here): fixed at 0
// The update is lin_update with codes in place of bounds (lin_update_knot, kernels_lin.hpp): lo and hi are not read.
// nu = rho y; dL/dc_A = nu goes to dL/dhi of LIN_AT_HI rows and to dL/dlo of LIN_AT_LO ones; row r of knot k gives
// dL/dC[r, :] = -(mu_r w_x' + nu_r x'), dL/dD[r, :] = -(mu_r w_u' + nu_r u'), zero outside A.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_lin.hpp"

namespace ndlqr {

enum : unsigned char { LIN_UNBOUNDED = 0, LIN_FREE = 1, LIN_AT_LO = 2, LIN_AT_HI = 3 };

// Start of a constrained adjoint. Per knot: the codes from the forward's v (vf) and the bounds, v = y = 0, and S^' (the
// SHIFTED records rec) on the knot's rows of the adjoint's resident right-hand side `res` -- the packed g on entry, S^' g
// on exit, in place -- which both ADMM right-hand sides receive; the pad entries and the knots k >= u.N are copied. Status
// and iteration count of every problem: 3 (not iterated) where the forward ended so or as 4 (certified infeasible), else
// 0 and one more in the running count.
//   grid (d.N, batch), block 64, dynamic LDS lin_wave_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_adjoint_start(Dims u, Dims d, int p, const double* __restrict__ rec,
                                                               const double* __restrict__ lo, const double* __restrict__ hi,
                                                               size_t bstride, const double* __restrict__ vf,
                                                               const int* __restrict__ fstatus, double* __restrict__ res,
                                                               unsigned char* __restrict__ code, double* __restrict__ v,
                                                               double* __restrict__ y, double* __restrict__ rhs0,
                                                               double* __restrict__ rhs1, int* __restrict__ status,
                                                               int* __restrict__ iters, int* __restrict__ running) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int n = u.n, m = u.m;
  if (k == 0 && lane == 0) {
    const int st = (fstatus[b] == 3 || fstatus[b] == 4) ? 3 : 0;  // (certified infeasible: nothing to differentiate)
    status[b] = st;
    iters[b] = 0;
    if (st == 0) atomicAdd(running, 1);
  }
  const size_t ok = ((size_t)b * d.N + k) * d.rows;
  const bool real = k < u.N, last = k == u.N - 1;
  if (real) {
    const size_t ob = (size_t)b * bstride + (size_t)k * p, ov = ((size_t)b * u.N + k) * p;
    for (int r = lane; r < p; r += 64) {
      const double l = lo[ob + r], h = hi[ob + r], vv = vf[ov + r];
      code[ov + r] = !box_bounded(l, h) ? LIN_UNBOUNDED : vv == h ? LIN_AT_HI : vv == l ? LIN_AT_LO : LIN_FREE;
      v[ov + r] = 0.0;
      y[ov + r] = 0.0;
    }
    const LinKnotLds S(lin_lds, n, m, p);
    cost_stage_record(rec + ((size_t)b * u.N + k) * cost_record_doubles(n, m), n, m, !last, S.sL, S.sLR, S.sG, lane);
    for (int i = lane; i < n; i += 64) { S.sl[i] = res[ok + i]; S.sx[i] = res[ok + d.n + i]; }
    if (!last)
      for (int j = lane; j < m; j += 64) S.su[j] = res[ok + 2 * d.n + j];
    wave_lds_sync();
    // lambda rows: L' straight into res (each lane reads back below only what it wrote itself); x and u rows stay in LDS
    cost_knot_St<true, false>(n, m, last, S.sL, S.sLR, S.sG, S.sl, S.sx, S.su, res + ok, nullptr, nullptr, lane);
    wave_lds_sync();
  }
  for (int r = lane; r < d.rows; r += 64) {
    const int blk = r < d.n ? 0 : (r < 2 * d.n ? 1 : 2), i = r - blk * d.n;
    const bool mapped = real && (blk < 2 ? i < n : (i < m && !last));
    double val;
    if (!mapped || blk == 0) {
      val = res[ok + r];  // (lambda row i: stored above by lane i mod 64 = r mod 64, this lane, since blk == 0 means r == i)
    } else {
      const LinKnotLds S(lin_lds, n, m, p);
      val = blk == 1 ? S.sx[i] : S.su[i];
      res[ok + r] = val;
    }
    rhs0[ok + r] = val;
    rhs1[ok + r] = val;
  }
}

// The rows of an adjoint update: the codes. A fixed row is clipped to [0, 0]; a free row's clip is the identity -- not a
// clip to +-inf, which would drop a NaN.
struct LinCodeRows {
  const unsigned char* cb;
  __device__ __forceinline__ LinCodeRows(const unsigned char* code, int b, int N, int p) : cb(code + (size_t)b * N * p) {}
  __device__ __forceinline__ bool operator()(int k, int p, int r, bool& clip, double& l, double& h) const {
    const unsigned char c = cb[(size_t)k * p + r];
    l = 0.0;
    h = 0.0;
    clip = c >= LIN_AT_LO;
    return c != LIN_UNBOUNDED;
  }
};

// One ADMM update of the constrained adjoint for every running problem after re-solve `it`: lin_update with the codes in
// place of the bounds (lin_update_knot over LinCodeRows; box_judge; lin_tail_frozen). v, y, res, the right-hand sides,
// status, iters, resid and the running count are the adjoint's own; rho [batch] is the forward's.
//   grid (batch), block 256, dynamic LDS 4 lin_wave_lds(n, m, p) doubles.
template <bool STRICT>
__global__ __launch_bounds__(256) void lin_adjoint_update(Dims u, Dims d, int p, int it, BoxParams P,
                                                          const double* __restrict__ z, const double* __restrict__ rec,
                                                          const double* __restrict__ C, const double* __restrict__ D,
                                                          const unsigned char* __restrict__ code, double* __restrict__ v,
                                                          double* __restrict__ y, const double* __restrict__ res,
                                                          const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                          const double* __restrict__ rhov, int* __restrict__ status,
                                                          int* __restrict__ iters, double* __restrict__ resid,
                                                          int* __restrict__ running) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  __shared__ double red[5][256];
  __shared__ int conv_s;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const double rho = rhov[b];
  const size_t oz = (size_t)b * d.N * d.rows;
  double* vb = v + (size_t)b * u.N * p;
  double* yb = y + (size_t)b * u.N * p;
  const LinKnotLds S(lin_lds + (size_t)wave * lin_wave_lds(u.n, u.m, p), u.n, u.m, p);
  const LinCodeRows rows(code, b, u.N, p);
  BoxMaxima M;
  for (int k = wave; k < u.N; k += 4)
    lin_update_knot<STRICT>(S, u, d, p, k, b, P, rho, z, rec, C, D, rows, vb, yb, res, rhs_next, oz, M, lane);
  M.reduce(red, tid);
  if (tid == 0) conv_s = box_judge(P, rho, red, b, it, status, iters, resid, running).frozen ? 1 : 0;
  __syncthreads();
  if (conv_s == 1) lin_tail_frozen(u, d, oz, rhs_cur, rhs_next, tid);
}

// End of a constrained adjoint: the adjoint solution blocks zs get w = S^ w~ of the last re-solve, in the caller's
// variables (lin_deliver_knot); a problem whose status is 3 (its forward ended non-finite and it was not iterated, or its own iterates did) gets w = 0.
//   grid (d.N, batch), block 64, dynamic LDS lin_wave_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_adjoint_finish(Dims u, Dims d, int p, const double* __restrict__ rec,
                                                                const double* __restrict__ z, const int* __restrict__ status,
                                                                double* __restrict__ zs) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (status[b] == 3) {
    for (int r = lane; r < d.rows; r += 64) zs[((size_t)b * d.N + k) * d.rows + r] = 0.0;
    return;
  }
  lin_deliver_knot(lin_lds, u, d, p, k, b, rec, z, zs, lane);
}

// Destinations of the constraint gradients: dL/d(C, D, lo, hi), nullptr = not computed. Per problem (or once, summed):
// gC [N][p n], gD [N][p m] column-major per knot like C, D; glo, ghi [N][p].
struct LinGradOut {
  double* p[4];
};
// entries of one knot: p n of gC | p m of gD | p of glo | p of ghi
__host__ __device__ inline int lin_grad_width(int n, int m, int p) { return p * (n + m + 2); }

// -(mu w + nu z) of one entry of a row; STRICT: t = mu w, s = nu z, -(t + s), each operation rounded on its own
template <bool STRICT>
__device__ __forceinline__ double lin_row_grad(double mu, double wj, double nu, double zj) {
  if constexpr (STRICT) {
    const double t = mu * wj;
    const double s = nu * zj;
    return -(t + s);
  } else {
    return -fma(mu, wj, nu * zj);
  }
}

// Entry e (< lin_grad_width) of knot k of problem b: *which = 0 .. 3 (gC, gD, glo, ghi), *at = its offset within the
// knot's part of that output. z: the resident solution, w: the adjoint's, both [batch][N][2n+m] in the device layout and
// the caller's variables; yf, ya: the forward's and the adjoint's scaled duals. Exactly 0 on the rows outside the active
// set, for D of the last knot and for a problem the adjoint did not solve (status 3).
template <bool STRICT>
__device__ __forceinline__ double lin_grad_entry(const Dims& u, const Dims& d, const int p, const double* __restrict__ rhov,
                                                 const unsigned char* __restrict__ code, const double* __restrict__ yf,
                                                 const double* __restrict__ ya, const int* __restrict__ status,
                                                 const double* __restrict__ z, const double* __restrict__ w, const int b,
                                                 const int k, const int e, int* which, int* at) {
  const int n = u.n, m = u.m, pn = p * n, pm = p * (n + m);
  int r, j = 0;
  if (e < pn) {
    *which = 0; *at = e;
    j = e / p; r = e - j * p;
  } else if (e < pm) {
    *which = 1; *at = e - pn;
    j = (e - pn) / p; r = (e - pn) - j * p;
  } else {
    r = e - pm;
    *which = r < p ? 2 : 3;
    if (r >= p) r -= p;
    *at = r;
  }
  if (status[b] == 3 || (*which == 1 && k == u.N - 1)) return 0.0;
  const size_t ev = ((size_t)b * u.N + k) * p + r;
  const unsigned char c = code[ev];
  if (c < LIN_AT_LO) return 0.0;
  const double rho = rhov[b];
  const double nu = rho * ya[ev];
  if (*which >= 2) return (*which == 3 ? c == LIN_AT_HI : c == LIN_AT_LO) ? nu : 0.0;
  const double mu = rho * yf[ev];
  const size_t o = ((size_t)b * d.N + k) * d.rows + (*which == 1 ? 2 * d.n : d.n) + j;
  return lin_row_grad<STRICT>(mu, w[o], nu, z[o]);
}

__device__ __forceinline__ void lin_grad_put(const Dims& u, const int p, const LinGradOut& out, const size_t prob, const int k,
                                             const int which, const int at, const double val) {
  if (!out.p[which]) return;
  const int per = which == 0 ? p * u.n : which == 1 ? p * u.m : p;
  out.p[which][(prob * u.N + k) * per + at] = val;
}

// Per-problem constraint gradients.
//   grid (N, batch), block 64.
template <bool STRICT>
__global__ void lin_constraint_grads(Dims u, Dims d, int p, const double* __restrict__ rhov,
                                     const unsigned char* __restrict__ code,
                                     const double* __restrict__ yf, const double* __restrict__ ya,
                                     const int* __restrict__ status, const double* __restrict__ z,
                                     const double* __restrict__ w, LinGradOut out) {
  const int k = blockIdx.x, b = blockIdx.y, W = lin_grad_width(u.n, u.m, p);
  for (int e = threadIdx.x; e < W; e += blockDim.x) {
    int which, at;
    const double val = lin_grad_entry<STRICT>(u, d, p, rhov, code, yf, ya, status, z, w, b, k, e, &which, &at);
    lin_grad_put(u, p, out, (size_t)b, k, which, at, val);
  }
}

// Batch sums of the constraint gradients: entry k W + e of [N][W], one thread each, over the problems [p0, p1) of split
// blockIdx.y in order. part == nullptr (one split): straight into the outputs; else into part[split][N W], which
// lin_grad_sum_splits adds up in order (the scheme of box_bound_grads_sum: deterministic, no atomics).
//   grid (ceil(N W / 256), nsplit), block 256.
template <bool STRICT>
__global__ __launch_bounds__(256) void lin_constraint_grads_sum(Dims u, Dims d, int p, const double* __restrict__ rhov,
                                                                int ppb,
                                                                const unsigned char* __restrict__ code,
                                                                const double* __restrict__ yf, const double* __restrict__ ya,
                                                                const int* __restrict__ status, const double* __restrict__ z,
                                                                const double* __restrict__ w, LinGradOut out,
                                                                double* __restrict__ part) {
  const int W = lin_grad_width(u.n, u.m, p);
  const size_t E = (size_t)u.N * W;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= E) return;
  const int k = (int)(g / W), e = (int)(g - (size_t)k * W);
  const int p0 = blockIdx.y * ppb, p1 = (p0 + ppb < u.batch) ? p0 + ppb : u.batch;
  double sum = 0.0;
  int which = 0, at = 0;
  for (int b = p0; b < p1; ++b) sum += lin_grad_entry<STRICT>(u, d, p, rhov, code, yf, ya, status, z, w, b, k, e, &which, &at);
  if (part) part[(size_t)blockIdx.y * E + g] = sum;
  else lin_grad_put(u, p, out, 0, k, which, at, sum);
}

// Second stage of a split batch sum: the splits of an entry added in order.
//   grid ceil(N W / 256), block 256.
static __global__ __launch_bounds__(256) void lin_grad_sum_splits(Dims u, int p, int nsplit, const double* __restrict__ part,
                                                                  LinGradOut out) {
  const int n = u.n, m = u.m, W = lin_grad_width(n, m, p);
  const size_t E = (size_t)u.N * W;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= E) return;
  double sum = 0.0;
  for (int s = 0; s < nsplit; ++s) sum += part[(size_t)s * E + g];
  const int k = (int)(g / W), e = (int)(g - (size_t)k * W), pn = p * n, pm = p * (n + m);
  const int which = e < pn ? 0 : e < pm ? 1 : e - pm < p ? 2 : 3;
  const int at = which == 0 ? e : which == 1 ? e - pn : which == 2 ? e - pm : e - pm - p;
  lin_grad_put(u, p, out, 0, k, which, at, sum);
}

// nu = rho[b] y of the adjoint on the fixed rows, 0 elsewhere, elementwise over [batch][N][p].
//   grid ceil(N p / 256), batch; block 256.
static __global__ void lin_adjoint_multipliers(int per_problem, const double* __restrict__ rhov,
                                               const unsigned char* __restrict__ code, const double* __restrict__ y,
                                               double* __restrict__ nu) {
  const double rho = rhov[blockIdx.y];
  const size_t o = (size_t)blockIdx.y * per_problem + blockIdx.x * blockDim.x + threadIdx.x;
  if ((int)(blockIdx.x * blockDim.x + threadIdx.x) < per_problem) nu[o] = code[o] >= LIN_AT_LO ? rho * y[o] : 0.0;
}

}  // namespace ndlqr
