// kernels_lin.hpp -- internal: general linear inequality constraints lo_k <= C_k x_k + D_k u_k <= hi_k by scaled ADMM on
// the dense-cost reduction (ndlqr_hip_init_constrained, ndlqr_hip_solve_constrained).
//
// Section 3.9 carried to the rows w = C x + D u: v (projected copy of w) and y (scaled dual) are [batch][N][p] in the
// CALLER's horizon, like the bounds lo, hi ([N][p] once when shared). A row is bounded (M = 1) when one of its bounds is
// finite. ADMM on such rows shifts the cost by rho C'MC, rho C'MD, rho D'MD -- dense: lin_shift_cost forms the shifted
// costs, the kernels of kernels_cost.hpp reduce them to a unit-cost problem (the SHIFTED records L | L_R | G and A~, B~),
// which is factored once. One iteration is a re-solve in the reduced variables followed by lin_update, which per knot
//     applies S^ to the knot's z~ (x, u in the caller's variables),      forms w = C x + D u,
//     steps the bounded rows (box_step of the shared update core),        stores v+, y+,
//     forms rho [C'; D'] M (y+ - v+),   applies S^',   writes the next reduced right-hand side res~ - S^'[...],
// and then judges the problem (box_judge) from
//     r_prim = max |w - v+|,  r_dual = rho max |G'(v+ - v)|,  sp = max(max |w|, max |v+|),  sd = rho max |G' y+|   (G = [C D]).
// The caller's block sizes are `u` (n, m, N of the flat arrays, the records and C, D), the device layout of z~ and of the
// right-hand sides is `d` (a zero-padded block size and / or a padded horizon): row i of lambda | x | u of knot k sits at
// k d.rows + (i | d.n + i | 2 d.n + i). Pad entries and the knots k >= u.N are never written: they keep the resident
// right-hand side lin_start copied. D of the caller's last knot is never loaded (its rows are w = C x).
// The penalty is per problem, rho[batch] (a fixed-penalty solve fills it with one value; lin_update may move it by powers
// of two at an adapt iteration, after which the host shifts, reduces and factors again and lin_start, in its restart
// mode, rewrites the right-hand sides of the problems that moved: DESIGN.md section 3.19).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box_core.hpp"
#include "kernels_cost_knot.hpp"
#include "kernels_lin_shift.hpp"

namespace ndlqr {

// doubles of LDS one wavefront of lin_update / lin_start / lin_finish stages for its knot: the record, C [p][n], D [p][m]
// (column-major, as the caller gives them) and the vectors lambda | x | u~ | u | three row vectors
__host__ __device__ inline size_t lin_wave_lds(int n, int m, int p) {
  return (size_t)n * cost_ld(n) + (size_t)m * cost_ld(m) + (size_t)m * n + (size_t)p * n + (size_t)p * m + 2 * (size_t)n +
         2 * (size_t)m + 3 * (size_t)p;
}

// Bounds in the caller's layout lo, hi [P][N][p] (P = batch or 1). commit == 0: only check, *bad = 1 when lo > hi (or
// NaN). commit == 1: copy them to dlo, dhi and the bounded pattern into mask, *changed = 1 where it differs.
//   grid (N, P), block 64.
static __global__ void lin_bounds(int N, int p, const double* __restrict__ lo, const double* __restrict__ hi, int commit,
                                  double* __restrict__ dlo, double* __restrict__ dhi, unsigned char* __restrict__ mask,
                                  int* __restrict__ bad, int* __restrict__ changed) {
  const size_t o = ((size_t)blockIdx.y * N + blockIdx.x) * p;
  for (int r = threadIdx.x; r < p; r += blockDim.x) {
    const double l = lo[o + r], h = hi[o + r];
    if (!commit) {
      if (!(l <= h)) *bad = 1;
      continue;
    }
    dlo[o + r] = l;
    dhi[o + r] = h;
    const unsigned char b = box_bounded(l, h) ? 1 : 0;
    if (mask[o + r] != b) {
      mask[o + r] = b;
      *changed = 1;
    }
  }
}

// rho[b] = value for every problem.
//   grid ceil(batch / 256), block 256.
static __global__ void lin_fill_rho(int batch, double value, double* __restrict__ rho) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) rho[b] = value;
}

// the row weights of the ADMM: the penalty on the bounded rows
struct LinPenaltyWeight {
  const double *lo, *hi;  // the knot's bounds
  double rho;
  __device__ __forceinline__ double operator()(int r) const { return box_bounded(lo[r], hi[r]) ? rho : 0.0; }
};

// Q^ = Q + rho[b] C'MC, H^ = H + rho[b] C'MD, R^ = R + rho[b] D'MD of every knot (the last: Q^ alone; H^ = 0, R^ = 1 are written
// and nothing of the caller's H, R, D is loaded there). One wavefront per (knot, problem); C, D and the row weights
// rho M go through LDS, the costs come in and leave as they lie. Q, R are read in their lower triangles (as cost_factor
// does) and leave symmetric. H may be null (zero).
//   grid (N, batch), block 64, dynamic LDS lin_shift_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_shift_cost(const int n, const int m, const int N, const int p,
                                                            const double* __restrict__ rhov,
                                                            const double* __restrict__ Q,
                                                            const double* __restrict__ H, const double* __restrict__ R,
                                                            const double* __restrict__ C, const double* __restrict__ D,
                                                            const double* __restrict__ lo, const double* __restrict__ hi,
                                                            const size_t bstride, double* __restrict__ Qs,
                                                            double* __restrict__ Hs, double* __restrict__ Rs) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  const int k = blockIdx.x, b = blockIdx.y;
  const LinPenaltyWeight weight = {lo + (size_t)b * bstride + (size_t)k * p, hi + (size_t)b * bstride + (size_t)k * p, rhov[b]};
  lin_shift_cost_knot(lin_lds, n, m, N, p, k, b, weight, Q, H, R, C, D, Qs, Hs, Rs, threadIdx.x);
}

// One wavefront's LDS for its knot (lin_wave_lds doubles at `base`).
struct LinKnotLds {
  double *sL, *sLR, *sG, *sC, *sD, *sl, *sx, *su, *ux, *t0, *t1, *t2;
  __device__ __forceinline__ LinKnotLds(double* base, int n, int m, int p) {
    sL = base;
    sLR = sL + (size_t)n * cost_ld(n);
    sG = sLR + (size_t)m * cost_ld(m);
    sC = sG + (size_t)m * n;
    sD = sC + (size_t)p * n;
    sl = sD + (size_t)p * m;  // lambda~ (lin_finish) | the x rows of the perturbation (n entries, as sx)
    sx = sl + n;
    su = sx + n;
    ux = su + m;  // u in the caller's variables
    t0 = ux + m;  // rho M (y - v) | M (v+ - v) | M y+ of the knot's rows
    t1 = t0 + p;
    t2 = t1 + p;
  }
};

// the knot's shifted record and C, D into LDS (D and the rest of the record: !last)
__device__ __forceinline__ void lin_stage_knot(const LinKnotLds& S, const Dims& u, const int p, const bool last,
                                               const double* __restrict__ rk, const double* __restrict__ Ck,
                                               const double* __restrict__ Dk, const int lane) {
  cost_stage_record(rk, u.n, u.m, !last, S.sL, S.sLR, S.sG, lane);
  for (int idx = lane; idx < p * u.n; idx += 64) S.sC[idx] = Ck[idx];
  if (!last)
    for (int idx = lane; idx < p * u.m; idx += 64) S.sD[idx] = Dk[idx];
}

// With rho M (y - v) of the knot's rows in S.t0 (and the record, C, D staged): the x and u rows of the next reduced
// right-hand side, rn = rs - S^'[C' t0; D' t0]. E != nullptr (lin_update): S.t1, S.t2 hold M (v+ - v) and M y+, and the
// maxima of |G' t1|, |G' t2| over the knot's entries are taken into E->rd, E->ym on the way. rn2: a second destination
// (lin_start writes both ping-pong buffers) or null. Begins and ends with the wavefront's LDS in order.
__device__ __forceinline__ void lin_next_rhs(const LinKnotLds& S, const Dims& u, const Dims& d, const int p, const bool last,
                                             const double* __restrict__ rs, double* __restrict__ rn, double* __restrict__ rn2,
                                             BoxMaxima* E, const int lane) {
  const int n = u.n, m = u.m;
  wave_lds_sync();
  for (int j = lane; j < n + (last ? 0 : m); j += 64) {
    const double* col = j < n ? S.sC + (size_t)p * j : S.sD + (size_t)p * (j - n);
    double a = 0.0, bb = 0.0, cc = 0.0;
    for (int r = 0; r < p; ++r) {
      a = fma(col[r], S.t0[r], a);
      if (E) {
        bb = fma(col[r], S.t1[r], bb);
        cc = fma(col[r], S.t2[r], cc);
      }
    }
    if (E) {
      E->rd = max_nan(E->rd, fabs(bb));
      E->ym = max_nan(E->ym, fabs(cc));
    }
    if (j < n) S.sx[j] = a;
    else S.su[j - n] = a;
  }
  wave_lds_sync();
  cost_knot_St<false, false>(n, m, last, S.sL, S.sLR, S.sG, nullptr, S.sx, S.su, nullptr, nullptr, nullptr, lane);
  wave_lds_sync();
  for (int i = lane; i < n; i += 64) {
    const double val = rs[d.n + i] - S.sx[i];
    rn[d.n + i] = val;
    if (rn2) rn2[d.n + i] = val;
  }
  if (!last)
    for (int j = lane; j < m; j += 64) {
      const double val = rs[2 * d.n + j] - S.su[j];
      rn[2 * d.n + j] = val;
      if (rn2) rn2[2 * d.n + j] = val;
    }
  wave_lds_sync();
}

// rho (y - v) of one bounded row (a rounded difference, then a rounded product: the same in both modes)
__device__ __forceinline__ double lin_row_weight(double rho, double v, double y) {
  const double t = y - v;
  return rho * t;
}

enum : int { LIN_START_WARM = 0, LIN_START_COLD = 1, LIN_START_MOVED = 2 };

// Start of a solve: both ADMM right-hand sides from the resident (shifted, reduced) one `res`. LIN_START_COLD: v = y = 0
// and the right-hand sides are copies of res. LIN_START_WARM: y of the rows the current bounds leave unbounded is zeroed
// and the right-hand sides are res~ - S^'[rho G'M(y - v)]. v and the SCALED dual y are taken as the previous solve left
// them whatever its penalty was -- as box_start does: a warm start with another rho starts from mu = rho y, not from the
// previous mu; the iteration converges from any start. A problem the previous solve left as 4 (prev_status: certified
// infeasible, its y has diverged) starts cold, as in box_start.
// LIN_START_MOVED, within a solve, after the shifted problem was reduced and factored again for new penalties: what
// LIN_START_WARM does -- pad entries and the knots k >= u.N included --, from the new res and the new records, for the
// problems marked in `moved` alone, whose marks it clears; y is zeroed nowhere. A problem that is not marked keeps both
// buffers: a frozen one's hold the right-hand side of its last re-solve, which its final (v, y) would not give again.
//   grid (batch), block 256, dynamic LDS 4 lin_wave_lds(n, m, p) doubles.
static __global__ __launch_bounds__(256) void lin_start(Dims u, Dims d, int p, int mode, const double* __restrict__ rhov,
                                                 const double* __restrict__ rec, const double* __restrict__ C,
                                                 const double* __restrict__ D, const double* __restrict__ lo,
                                                 const double* __restrict__ hi, size_t bstride, const double* __restrict__ res,
                                                 const int* __restrict__ prev_status, double* __restrict__ v,
                                                 double* __restrict__ y, double* __restrict__ rhs0, double* __restrict__ rhs1,
                                                 int* __restrict__ moved) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (mode == LIN_START_MOVED && moved[b] == 0) return;  // (uniform over the workgroup)
  const double rho = rhov[b];
  const size_t oz = (size_t)b * d.N * d.rows;
  for (unsigned e = tid; e < (unsigned)(d.N * d.rows); e += blockDim.x) {
    const double val = res[oz + e];
    rhs0[oz + e] = val;
    rhs1[oz + e] = val;
  }
  double* vb = v + (size_t)b * u.N * p;
  double* yb = y + (size_t)b * u.N * p;
  if (mode == LIN_START_COLD || (mode == LIN_START_WARM && prev_status[b] == 4)) {  // (uniform over the workgroup)
    for (unsigned e = tid; e < (unsigned)(u.N * p); e += blockDim.x) { vb[e] = 0.0; yb[e] = 0.0; }
    return;
  }
  __syncthreads();  // (the copies above precede this workgroup's overwrites of the x and u rows; every thread has read the mark)
  if (mode == LIN_START_MOVED && tid == 0) moved[b] = 0;
  const LinKnotLds S(lin_lds + (size_t)wave * lin_wave_lds(u.n, u.m, p), u.n, u.m, p);
  const size_t recd = cost_record_doubles(u.n, u.m);
  for (int k = wave; k < u.N; k += 4) {
    const bool last = k == u.N - 1;
    const size_t kb = (size_t)b * u.N + k;
    lin_stage_knot(S, u, p, last, rec + kb * recd, C + kb * p * u.n, D + kb * p * u.m, lane);
    const size_t ob = (size_t)b * bstride + (size_t)k * p;
    for (int r = lane; r < p; r += 64) {
      const bool bounded = box_bounded(lo[ob + r], hi[ob + r]);
      if (!bounded && mode == LIN_START_WARM) yb[(size_t)k * p + r] = 0.0;
      S.t0[r] = bounded ? lin_row_weight(rho, vb[(size_t)k * p + r], yb[(size_t)k * p + r]) : 0.0;
    }
    const size_t ok = oz + (size_t)k * d.rows;
    lin_next_rhs(S, u, d, p, last, res + ok, rhs0 + ok, rhs1 + ok, nullptr, lane);
  }
}

// What an update knows of the rows of problem b: row r of knot k -> is it in the splitting (bounded), and the
// clip of its step. The forward's rows: the bounds as they lie; the clip is always on.
struct LinBoundRows {
  const double *lo, *hi;
  size_t ob;  // the problem's offset in the bounds
  __device__ __forceinline__ LinBoundRows(const double* lo_, const double* hi_, size_t bstride, int b)
      : lo(lo_), hi(hi_), ob((size_t)b * bstride) {}
  __device__ __forceinline__ bool operator()(int k, int p, int r, bool& clip, double& l, double& h) const {
    const size_t o = ob + (size_t)k * p;
    l = lo[o + r];
    h = hi[o + r];
    clip = true;
    return box_bounded(l, h);
  }
};

// One knot of an ADMM update, by one wavefront: the body lin_update and lin_adjoint_update (kernels_lin_grad.hpp) share.
// Stages the knot's shifted record and C, D, applies S^ to the knot's z~, forms w = C x + D u a row per lane, steps the
// rows `rows` puts in the splitting (box_step), stores v+, y+, and writes the knot's next right-hand side with the maxima
// on the same pass (lin_next_rhs). oz: the problem's offset in z, res and rhs_next; vb, yb: the problem's v and y.
template <bool STRICT, class Rows>
__device__ __forceinline__ void lin_update_knot(const LinKnotLds& S, const Dims& u, const Dims& d, const int p, const int k,
                                                const int b, const BoxParams& P, const double rho,
                                                const double* __restrict__ z, const double* __restrict__ rec,
                                                const double* __restrict__ C, const double* __restrict__ D, const Rows& rows,
                                                double* __restrict__ vb, double* __restrict__ yb,
                                                const double* __restrict__ res, double* __restrict__ rhs_next, const size_t oz,
                                                BoxMaxima& M, const int lane) {
  const int n = u.n, m = u.m;
  const size_t recd = cost_record_doubles(n, m);
  const bool last = k == u.N - 1;
  const size_t kb = (size_t)b * u.N + k, ok = oz + (size_t)k * d.rows;
  lin_stage_knot(S, u, p, last, rec + kb * recd, C + kb * p * n, D + kb * p * m, lane);
  for (int i = lane; i < n; i += 64) S.sx[i] = z[ok + d.n + i];
  if (!last)
    for (int j = lane; j < m; j += 64) S.su[j] = z[ok + 2 * d.n + j];
  wave_lds_sync();
  // x -> S.sx, u -> S.ux
  cost_knot_S<false>(n, m, last, S.sL, S.sLR, S.sG, nullptr, S.sx, S.su, nullptr, S.sx, S.ux, lane);
  wave_lds_sync();
  for (int r = lane; r < p; r += 64) {
    double w = 0.0;
    for (int j = 0; j < n; ++j) w = fma(S.sC[r + p * j], S.sx[j], w);
    if (!last)
      for (int j = 0; j < m; ++j) w = fma(S.sD[r + p * j], S.ux[j], w);
    bool clip;
    double l, h;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (rows(k, p, r, clip, l, h)) {
      const size_t e = (size_t)k * p + r;
      const double v0 = vb[e], y0 = yb[e];
      const BoxStep s = box_step<STRICT>(P, w, v0, y0, clip, l, h);
      vb[e] = s.vn;
      yb[e] = s.yn;
      M.rp = max_nan(M.rp, fabs(w - s.vn));
      M.zm = max_nan(M.zm, fabs(w));
      M.vm = max_nan(M.vm, fabs(s.vn));
      t0 = lin_row_weight(rho, s.vn, s.yn);
      t1 = s.vn - v0;
      t2 = s.yn;
    }
    S.t0[r] = t0;
    S.t1[r] = t1;
    S.t2[r] = t2;
  }
  lin_next_rhs(S, u, d, p, last, res + ok, rhs_next + ok, nullptr, &M, lane);
}

// a frozen problem's next right-hand side is its current one (the x and u rows of the knots k < u.N)
__device__ __forceinline__ void lin_tail_frozen(const Dims& u, const Dims& d, const size_t oz,
                                                const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                const int tid) {
  const int n = u.n, m = u.m;
  for (unsigned e = tid; e < (unsigned)(u.N * (n + m)); e += blockDim.x) {
    const unsigned k = e / (unsigned)(n + m), j = e - k * (unsigned)(n + m);
    if ((int)k == u.N - 1 && (int)j >= n) continue;
    const size_t o = oz + (size_t)k * d.rows + ((int)j < n ? d.n + j : 2 * d.n + (j - n));
    rhs_next[o] = rhs_cur[o];
  }
}

// Tail of a problem whose penalty moved: y <- y (rho / rho+) on its bounded rows. Row r of knot k belongs to the lane
// that stored its y+ in lin_update_knot, so every lane re-reads only what it wrote itself.
__device__ __forceinline__ void lin_tail_new_penalty(const Dims& u, const int p, const LinBoundRows& rows,
                                                     double* __restrict__ yb, const double s, const int wave, const int lane) {
  for (int k = wave; k < u.N; k += 4)
    for (int r = lane; r < p; r += 64) {
      bool clip;
      double l, h;
      if (rows(k, p, r, clip, l, h)) yb[(size_t)k * p + r] *= s;
    }
}

// One ADMM update of every running problem (status[b] == 0) after re-solve `it`; see the head of this file. z: the
// re-solve's solution z~ [batch][N][2n+m] (device layout) with the right-hand side rhs_cur; rec, C, D, v, y in the
// caller's block sizes. The four wavefronts take the knots k < u.N round-robin (lin_update_knot); then the maxima are
// reduced and thread 0 judges (box_judge). A frozen problem's next right-hand side is its current one. adapt != 0: a
// problem that goes on may move its penalty (box_adapt_penalty): then rho[b] = rho+, y of its bounded rows is multiplied
// by rho / rho+ (mu = rho y is kept), moved[b] = 1 and running[1] counts it. Its next right-hand side is NOT the one of
// rho+ -- res~ and S^' belong to the shifted records of rho+, which the host has yet to make: lin_start(LIN_START_MOVED)
// writes it after them. A frozen problem never moves.
//   grid (batch), block 256, dynamic LDS 4 lin_wave_lds(n, m, p) doubles.
template <bool STRICT>
__global__ __launch_bounds__(256) void lin_update(Dims u, Dims d, int p, int it, int adapt, BoxParams P,
                                                  const double* __restrict__ z,
                                                  const double* __restrict__ rec, const double* __restrict__ C,
                                                  const double* __restrict__ D, const double* __restrict__ lo,
                                                  const double* __restrict__ hi, size_t bstride, double* __restrict__ v,
                                                  double* __restrict__ y, const double* __restrict__ res,
                                                  const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                  double* __restrict__ rhov, int* __restrict__ status,
                                                  int* __restrict__ iters, double* __restrict__ resid,
                                                  int* __restrict__ running, int* __restrict__ moved) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  __shared__ double red[5][256];
  __shared__ double rho_s;  // the new penalty when conv_s == 2
  __shared__ int conv_s;    // 0: goes on, 1: frozen, 2: goes on with a new penalty
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const double rho = rhov[b];
  const size_t oz = (size_t)b * d.N * d.rows;
  double* vb = v + (size_t)b * u.N * p;
  double* yb = y + (size_t)b * u.N * p;
  const LinKnotLds S(lin_lds + (size_t)wave * lin_wave_lds(u.n, u.m, p), u.n, u.m, p);
  const LinBoundRows rows(lo, hi, bstride, b);
  BoxMaxima M;
  for (int k = wave; k < u.N; k += 4)
    lin_update_knot<STRICT>(S, u, d, p, k, b, P, rho, z, rec, C, D, rows, vb, yb, res, rhs_next, oz, M, lane);
  M.reduce(red, tid);
  if (tid == 0) {
    const BoxVerdict J = box_judge(P, rho, red, b, it, status, iters, resid, running);
    conv_s = J.frozen ? 1 : adapt && box_adapt_penalty(P, rho, J, b, rhov, running, &rho_s) ? 2 : 0;
    if (conv_s == 2) moved[b] = 1;
  }
  __syncthreads();
  if (conv_s == 1) lin_tail_frozen(u, d, oz, rhs_cur, rhs_next, tid);
  else if (conv_s == 2) lin_tail_new_penalty(u, p, rows, yb, rho / rho_s, wave, lane);
}

// Knot k of problem b of a delivery, by one wavefront: zs gets S^ z~ -- lambda, x, u in the caller's variables under the
// shifted records -- and the pad entries and the knots k >= u.N as z~ holds them. The body of lin_finish and
// lin_adjoint_finish (kernels_lin_grad.hpp). lds: lin_wave_lds(n, m, p) doubles.
__device__ __forceinline__ void lin_deliver_knot(double* lds, const Dims& u, const Dims& d, const int p, const int k,
                                                 const int b, const double* __restrict__ rec, const double* __restrict__ z,
                                                 double* __restrict__ zs, const int lane) {
  const int n = u.n, m = u.m;
  const size_t ok = ((size_t)b * d.N + k) * d.rows;
  const bool real = k < u.N, last = k == u.N - 1;
  for (int r = lane; r < d.rows; r += 64) {
    const int blk = r < d.n ? 0 : (r < 2 * d.n ? 1 : 2), i = r - blk * d.n;
    const bool mapped = real && (blk < 2 ? i < n : (i < m && !last));
    if (!mapped) zs[ok + r] = z[ok + r];
  }
  if (!real) return;
  const LinKnotLds S(lds, n, m, p);
  cost_stage_record(rec + ((size_t)b * u.N + k) * cost_record_doubles(n, m), n, m, !last, S.sL, S.sLR, S.sG, lane);
  for (int i = lane; i < n; i += 64) { S.sl[i] = z[ok + i]; S.sx[i] = z[ok + d.n + i]; }
  if (!last)
    for (int j = lane; j < m; j += 64) S.su[j] = z[ok + 2 * d.n + j];
  wave_lds_sync();
  cost_knot_S<true>(n, m, last, S.sL, S.sLR, S.sG, S.sl, S.sx, S.su, zs + ok, zs + ok + d.n, zs + ok + 2 * d.n, lane);
}

// End of a solve: the resident solution blocks zs get S^ z~ of the last re-solve (lin_deliver_knot).
//   grid (d.N, batch), block 64, dynamic LDS lin_wave_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_finish(Dims u, Dims d, int p, const double* __restrict__ rec,
                                                        const double* __restrict__ z, double* __restrict__ zs) {
  extern __shared__ __attribute__((aligned(16))) double lin_lds[];
  lin_deliver_knot(lin_lds, u, d, p, blockIdx.x, blockIdx.y, rec, z, zs, threadIdx.x);
}

// mu = rho[b] y, elementwise over [batch][N][p].
//   grid ceil(N p / 256), batch; block 256.
static __global__ void lin_multipliers(int per_problem, const double* __restrict__ rhov, const double* __restrict__ y,
                                       double* __restrict__ mu) {
  const int b = blockIdx.y;
  const double rho = rhov[b];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < per_problem) mu[(size_t)b * per_problem + e] = rho * y[(size_t)b * per_problem + e];
}

}  // namespace ndlqr
