// kernels_cost.hpp -- dense cost matrices and state-input cross terms by exact reduction to a unit-cost problem of the
// same shape (gfx950, fp64, runtime-sized in n and m).
//
// The dense problem has, per knot k < N-1, the cost blocks Q_k [n][n], R_k [m][m] and the cross term H_k [n][m]
// (stationarity rows Q x + H u + q - lambda_k + A' lambda_{k+1} = 0 and H' x + R u + r + B' lambda_{k+1} = 0), and Q alone at
// the last knot. Only the LOWER triangles of Q and R are read. With
//     R = L_R L_R',   G = R^-1 H',   Q' = Q - H G = Q - W W' (W = H L_R^-T),   Q' = L L'
// the change of variables lambda_k = L_k lambda~_k, x_k = L_k^-T xi_k, u_k = L_R^-T nu_k - G_k x_k (z = S z~) turns the KKT
// system into that of a problem with Q~ = 1, R~ = 1 and
//     A~_k = L_{k+1}' (A_k - B_k G_k) L_k^-T,   B~_k = L_{k+1}' B_k L_R^-T:   K~ = S' K S, b~ = S' b, K^-1 g = S K~^-1 S' g.
// Four kernels, one wavefront per (knot, problem), everything staged through LDS, whole lines in and out:
//     cost_factor      Q, H, R             -> the knot's record L | L_R | G (resident, cost_record_doubles(n, m) doubles)
//     cost_transform   A, B, records k, k+1 -> A~, B~ in the caller's flat layout (what the pack kernels read)
//     cost_apply_t     S' on a right-hand side: flat (q, r, d, x0) -> flat (q~, r~, d~, x0~), or a packed [count][nvars]
//                      vector in [lambda x u] order in place (the adjoint's g)
//     cost_apply       S on a packed [count][nvars] solution, in place
// and the two of the asynchronous step (ndlqr_hip_step_dense_async), which work between the caller's arrays and the device
// layout directly:
//     cost_pack_rhs       S' on the flat (q, r, d, x0), or a part of them -> the device right-hand side of a buffer set
//     cost_deliver_slice  S on the z blocks of a knot range -> the packed slice [count][nknots][width]
// The per-knot pieces -- record layout, triangular solves, the bodies of S and S' -- live in kernels_cost_knot.hpp, which
// kernels_lin.hpp shares.
// A, B, H, R, r, d of the caller's last knot are never loaded (every such load sits behind the wave-uniform test of the
// knot): whatever they hold, a NaN included, reaches no output. The last knot's record is L | 1 | 0.
// A Cholesky pivot that is not positive counts in the problem's info word like the solver's own (flag_failure) and is
// taken as 1: finite input gives finite output, nothing is written out of range.
#pragma once
#include "kernels_common.hpp"
#include "kernels_cost_knot.hpp"

namespace ndlqr {

// dynamic LDS (doubles) of the four kernels
__host__ __device__ inline size_t cost_factor_lds(int n, int m) { return (size_t)n * n + (size_t)m * m + (size_t)n * m; }
__host__ __device__ inline size_t cost_transform_lds(int n, int m) {
  return (size_t)n * n + (size_t)n * m + 2 * (size_t)n * cost_ld(n) + (size_t)m * cost_ld(m) + (size_t)m * n;
}
__host__ __device__ inline size_t cost_apply_lds(int n, int m) {
  return (size_t)n * cost_ld(n) + (size_t)m * cost_ld(m) + (size_t)m * n + 3 * (size_t)n + m;
}

// count entries of `a` set to `value` (Q~ | R~ = 1 of the reduced problem)
static __global__ __launch_bounds__(256) void cost_fill(double* __restrict__ a, const size_t count, const double value) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) a[i] = value;
}

// In-place Cholesky of the lower triangle of the k x k matrix `a` (leading dimension ld) in LDS by one wavefront,
// right-looking, a column per step. Returns how many pivots were not positive (each taken as 1).
__device__ inline int cost_chol_lds(double* a, const int ld, const int k, const int lane) {
  int bad = 0;
  for (int j = 0; j < k; ++j) {
    const double p = a[j + ld * j];
    const bool ok = p > 0.0;
    bad += ok ? 0 : 1;
    const double dj = ok ? sqrt(p) : 1.0;
    for (int i = j + lane; i < k; i += 64) a[i + ld * j] = i == j ? dj : a[i + ld * j] / dj;
    wave_lds_sync();
    const int t = k - j - 1;
    for (int idx = lane; idx < t * t; idx += 64) {
      const int cc = idx / t, c = j + 1 + cc, i = j + 1 + (idx - cc * t);
      if (i >= c) a[i + ld * c] = fma(-a[i + ld * j], a[c + ld * j], a[i + ld * c]);
    }
    wave_lds_sync();
  }
  return bad;
}

// grid (N, batch), block 64, dynamic LDS cost_factor_lds(n, m) doubles. Q [batch][N][n*n], R [batch][N][m*m], H
// [batch][N][n*m] (null: zero), column-major; rec [batch][N][cost_record_doubles]; info [batch + 1].
static __global__ __launch_bounds__(64) void cost_factor(const int n, const int m, const int N, const int batch,
                                                         const double* __restrict__ Q, const double* __restrict__ H,
                                                         const double* __restrict__ R, double* __restrict__ rec,
                                                         int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  double* sQ = cost_lds;
  double* sR = sQ + (size_t)n * n;
  double* sH = sR + (size_t)m * m;  // H, then W = H L_R^-T, then G' (sH[i + n j] = G(j, i))
  {
    const double* Qk = Q + kb * n * n;
    for (int idx = lane; idx < n * n; idx += 64) {
      const int j = idx / n, i = idx - j * n;
      sQ[idx] = i >= j ? Qk[idx] : 0.0;
    }
  }
  if (!last) {
    const double* Rk = R + kb * m * m;
    for (int idx = lane; idx < m * m; idx += 64) {
      const int j = idx / m, i = idx - j * m;
      sR[idx] = i >= j ? Rk[idx] : 0.0;
    }
    const double* Hk = H ? H + kb * n * m : nullptr;
    for (int idx = lane; idx < n * m; idx += 64) sH[idx] = Hk ? Hk[idx] : 0.0;
  }
  wave_lds_sync();
  int bad = 0;
  if (!last) {
    bad += cost_chol_lds(sR, m, m, lane);
    // W L_R' = H: a row per lane, forward over the columns
    for (int i = lane; i < n; i += 64)
      for (int j = 0; j < m; ++j) {
        double s = sH[i + n * j];
        for (int c = 0; c < j; ++c) s = fma(-sH[i + n * c], sR[j + m * c], s);
        sH[i + n * j] = s / sR[j + m * j];
      }
    wave_lds_sync();
    // Q' = Q - W W' (lower triangle)
    for (int idx = lane; idx < n * n; idx += 64) {
      const int j = idx / n, i = idx - j * n;
      if (i < j) continue;
      double s = sQ[idx];
      for (int c = 0; c < m; ++c) s = fma(-sH[i + n * c], sH[j + n * c], s);
      sQ[idx] = s;
    }
    wave_lds_sync();
    // G' L_R = W: a row per lane, backward over the columns
    for (int i = lane; i < n; i += 64)
      for (int j = m - 1; j >= 0; --j) {
        double s = sH[i + n * j];
        for (int c = j + 1; c < m; ++c) s = fma(-sR[c + m * j], sH[i + n * c], s);
        sH[i + n * j] = s / sR[j + m * j];
      }
    wave_lds_sync();
  }
  bad += cost_chol_lds(sQ, n, n, lane);
  if (bad > 0 && lane == 0) {
    atomicAdd(info + b, bad);
    atomicAdd(info + batch, bad);
  }
  double* rk = rec + kb * cost_record_doubles(n, m);
  for (int idx = lane; idx < n * n; idx += 64) rk[idx] = sQ[idx];
  rk += (size_t)n * n;
  for (int idx = lane; idx < m * m; idx += 64) {
    const int j = idx / m, i = idx - j * m;
    rk[idx] = last ? (i == j ? 1.0 : 0.0) : sR[idx];
  }
  rk += (size_t)m * m;
  for (int idx = lane; idx < m * n; idx += 64) {
    const int i = idx / m, j = idx - i * m;
    rk[idx] = last ? 0.0 : sH[i + n * j];
  }
}

// grid (N, batch), block 64, dynamic LDS cost_transform_lds(n, m) doubles. A [batch][N][n*n], B [batch][N][n*m] and the
// outputs At, Bt likewise (column-major, the caller's flat layout); knot N-1 gets zeros.
static __global__ __launch_bounds__(64) void cost_transform(const int n, const int m, const int N,
                                                            const double* __restrict__ A, const double* __restrict__ B,
                                                            const double* __restrict__ rec, double* __restrict__ At,
                                                            double* __restrict__ Bt) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const size_t kb = (size_t)b * N + k;
  double* Atk = At + kb * n * n;
  double* Btk = Bt + kb * n * m;
  if (k == N - 1) {
    for (int idx = lane; idx < n * n; idx += 64) Atk[idx] = 0.0;
    for (int idx = lane; idx < n * m; idx += 64) Btk[idx] = 0.0;
    return;
  }
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  double* sM = cost_lds;                 // A, then A - B G, then (A - B G) L_k^-T
  double* sB = sM + (size_t)n * n;       // B, then B L_R^-T
  double* sLk = sB + (size_t)n * m;
  double* sL1 = sLk + (size_t)n * ldn;   // L_{k+1}
  double* sLR = sL1 + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  const size_t recd = cost_record_doubles(n, m);
  {
    const double* Ak = A + kb * n * n;
    const double* Bk = B + kb * n * m;
    for (int idx = lane; idx < n * n; idx += 64) sM[idx] = Ak[idx];
    for (int idx = lane; idx < n * m; idx += 64) sB[idx] = Bk[idx];
  }
  cost_stage_record(rec + kb * recd, n, m, true, sLk, sLR, sG, lane);
  cost_stage_record(rec + (kb + 1) * recd, n, m, false, sL1, nullptr, nullptr, lane);
  wave_lds_sync();
  for (int idx = lane; idx < n * n; idx += 64) {
    const int j = idx / n, i = idx - j * n;
    double s = sM[idx];
    for (int c = 0; c < m; ++c) s = fma(-sB[i + n * c], sG[c + m * j], s);
    sM[idx] = s;
  }
  wave_lds_sync();
  // X L_k' = A - B G and Y L_R' = B: a row per lane, forward over the columns
  for (int i = lane; i < n; i += 64) {
    for (int j = 0; j < n; ++j) {
      double s = sM[i + n * j];
      for (int c = 0; c < j; ++c) s = fma(-sM[i + n * c], sLk[j + ldn * c], s);
      sM[i + n * j] = s / sLk[j + ldn * j];
    }
    for (int j = 0; j < m; ++j) {
      double s = sB[i + n * j];
      for (int c = 0; c < j; ++c) s = fma(-sB[i + n * c], sLR[j + ldm * c], s);
      sB[i + n * j] = s / sLR[j + ldm * j];
    }
  }
  wave_lds_sync();
  for (int idx = lane; idx < n * n; idx += 64) {
    const int j = idx / n, i = idx - j * n;
    double s = 0.0;
    for (int c = i; c < n; ++c) s = fma(sL1[c + ldn * i], sM[c + n * j], s);
    Atk[idx] = s;
  }
  for (int idx = lane; idx < n * m; idx += 64) {
    const int j = idx / n, i = idx - j * n;
    double s = 0.0;
    for (int c = i; c < n; ++c) s = fma(sL1[c + ldn * i], sB[c + n * j], s);
    Btk[idx] = s;
  }
}

// S' on a right-hand side. grid (N, count), block 64, dynamic LDS cost_apply_lds(n, m) doubles; rec: the records of the
// `count` problems. g null: flat q, d [count][N][n], r [count][N][m], x0 [count][n] -> qt, rt, dt, x0t (rt, dt of knot
// N-1: zero). g set: the packed vectors [count][nvars] -> gt (gt == g: in place). Per knot the lambda rows (x0 | d_{k-1})
// go through L_k', the x rows (q_k) become L_k^-1 (q_k - G_k' r_k) and the u rows (r_k) L_R^-1 r_k.
static __global__ __launch_bounds__(64) void cost_apply_t(const int n, const int m, const int N,
                                                          const double* __restrict__ rec, const double* q, const double* r,
                                                          const double* dd, const double* x0, const double* g, double* qt,
                                                          double* rt, double* dt, double* x0t, double* gt) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  const int ldn = cost_ld(n), ldm = cost_ld(m), rows = 2 * n + m;
  double* sL = cost_lds;
  double* sLR = sL + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  double* sl = sG + (size_t)m * n;
  double* sx = sl + n;
  double* su = sx + n;
  const double *il, *ix, *iu;
  double *ol, *ox, *ou;
  if (g) {
    const size_t at = (size_t)b * ((size_t)rows * N - m) + (size_t)k * rows;
    il = g + at; ix = il + n; iu = ix + n;
    ol = gt + at; ox = ol + n; ou = ox + n;
  } else {
    il = k == 0 ? x0 + (size_t)b * n : dd + (kb - 1) * n;
    ol = k == 0 ? x0t + (size_t)b * n : dt + (kb - 1) * n;
    ix = q + kb * n; ox = qt + kb * n;
    iu = r + kb * m; ou = rt + kb * m;
  }
  cost_stage_record(rec + kb * cost_record_doubles(n, m), n, m, !last, sL, sLR, sG, lane);
  for (int i = lane; i < n; i += 64) { sl[i] = il[i]; sx[i] = ix[i]; }
  if (!last)
    for (int i = lane; i < m; i += 64) su[i] = iu[i];
  wave_lds_sync();
  cost_knot_St<true, true>(n, m, last, sL, sLR, sG, sl, sx, su, ol, ox, ou, lane);
  if (last && !g) {
    for (int i = lane; i < m; i += 64) ou[i] = 0.0;
    for (int i = lane; i < n; i += 64) dt[kb * n + i] = 0.0;
  }
}

// S on packed solutions, in place. grid (N, count), block 64, dynamic LDS cost_apply_lds(n, m) doubles; rec: the records
// of the `count` problems, z [count][nvars] in [lambda x u] order: lambda_k = L_k lambda~_k, x_k = L_k^-T xi_k,
// u_k = L_R^-T nu_k - G_k x_k.
static __global__ __launch_bounds__(64) void cost_apply(const int n, const int m, const int N, const double* __restrict__ rec,
                                                        double* z) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  const int ldn = cost_ld(n), ldm = cost_ld(m), rows = 2 * n + m;
  double* sL = cost_lds;
  double* sLR = sL + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  double* sl = sG + (size_t)m * n;
  double* sx = sl + n;
  double* su = sx + n;
  double* zl = z + (size_t)b * ((size_t)rows * N - m) + (size_t)k * rows;
  double* zx = zl + n;
  double* zu = zx + n;
  cost_stage_record(rec + kb * cost_record_doubles(n, m), n, m, !last, sL, sLR, sG, lane);
  for (int i = lane; i < n; i += 64) { sl[i] = zl[i]; sx[i] = zx[i]; }
  if (!last)
    for (int i = lane; i < m; i += 64) su[i] = zu[i];
  wave_lds_sync();
  cost_knot_S<true>(n, m, last, sL, sLR, sG, sl, sx, su, zl, zx, zu, lane);
}

// The part mask of cost_pack_rhs, the bits of copy_rhs_parts_generic: q and r (the x and u rows of every knot; always
// together, q~_k = L_k^-1 (q_k - G_k' r_k) needs both), d (the lambda rows of the knots >= 1), x0 (the lambda rows of knot 0)
constexpr unsigned COST_PART_QR = 3u, COST_PART_D = 4u, COST_PART_X0 = 8u;

// S' on the caller's flat right-hand side, packed in the same pass: the parts of `parts` of q, d [batch][du.N][n], r
// [batch][du.N][m], x0 [batch][n] (this device's memory or a device-side view of pinned memory; a part that is not
// replaced may be null) -> the entries of the device right-hand side rhs [batch][d.N][d.rows] that pack_rhs_one /
// pack_rhs_one_hp write of S' b: negated, lambda | x | u rows at 0 | d.n | 2 d.n, the u rows of the caller's last knot
// zero. Nothing else of rhs -- the pad rows, the tail knots of a padded horizon, the parts not in `parts` -- is touched,
// and nothing goes through arrays that exist once per solver: two steps in flight on two streams share nothing.
// grid (du.N, batch), or (1, batch) where `parts` is x0 alone; block 64, dynamic LDS cost_apply_lds(n, m) doubles. The
// arithmetic is cost_knot_St's, so the bits are those of cost_apply_t followed by the pack kernel.
static __global__ __launch_bounds__(64) void cost_pack_rhs(const Dims du, const Dims d, const unsigned parts,
                                                           const double* __restrict__ rec, const double* q, const double* r,
                                                           const double* dd, const double* x0, double* __restrict__ rhs) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int n = du.n, m = du.m, N = du.N;
  const bool last = k == N - 1;
  const bool qr = (parts & COST_PART_QR) != 0, lam = (parts & (k == 0 ? COST_PART_X0 : COST_PART_D)) != 0;
  if (!qr && !lam) return;  // (wave-uniform)
  const size_t kb = (size_t)b * N + k;
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  double* sL = cost_lds;
  double* sLR = sL + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  double* sl = sG + (size_t)m * n;
  double* sx = sl + n;
  double* su = sx + n;
  double* so = su + m;  // L' sl
  // (a knot whose x and u rows stay runs as a last knot on a zero x block: L and the lambda rows alone)
  const bool tail = last || !qr;
  cost_stage_record(rec + kb * cost_record_doubles(n, m), n, m, !tail, sL, sLR, sG, lane);
  const double* il = k == 0 ? x0 + (size_t)b * n : dd + (kb - 1) * n;
  for (int i = lane; i < n; i += 64) {
    sl[i] = lam ? il[i] : 0.0;
    sx[i] = qr ? q[kb * n + i] : 0.0;
  }
  if (!tail)
    for (int i = lane; i < m; i += 64) su[i] = r[kb * m + i];
  wave_lds_sync();
  cost_knot_St<true, false>(n, m, tail, sL, sLR, sG, sl, sx, su, so, nullptr, nullptr, lane);
  wave_lds_sync();
  double* out = rhs + ((size_t)b * d.N + k) * d.rows;
  if (lam)
    for (int i = lane; i < n; i += 64) out[i] = -so[i];
  if (qr) {
    for (int i = lane; i < n; i += 64) out[d.n + i] = -sx[i];
    for (int i = lane; i < m; i += 64) out[2 * d.n + i] = last ? 0.0 : -su[i];
  }
}

// S on a slice of the solutions, packed in the same pass: the z blocks of the knots [knot0, knot0 + nknots) of z
// [batch][d.N][d.rows] (the reduced variables, lambda | x | u at 0 | d.n | 2 d.n) through that knot's record into dst
// [batch][nknots][width], of each knot the blocks of `blocks` (bit 0: lambda, 1: state, 2: input) in the order of
// pack_selection_generic. u = L_R^-T nu - G L^-T xi is computed from both whether or not the state block is selected; u
// of the caller's last knot comes out as exact zero. grid (nknots, batch), block 64, dynamic LDS cost_apply_lds(n, m)
// doubles. The arithmetic is cost_knot_S's, so the bits are those of cost_apply on the packed vector.
static __global__ __launch_bounds__(64) void cost_deliver_slice(const Dims du, const Dims d, const int knot0, const int nknots,
                                                                const unsigned blocks, const double* __restrict__ rec,
                                                                const double* __restrict__ z, double* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) double cost_lds[];
  const int kk = blockIdx.x, k = knot0 + kk, b = blockIdx.y, lane = threadIdx.x;
  const int n = du.n, m = du.m, N = du.N;
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  double* sL = cost_lds;
  double* sLR = sL + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  double* sl = sG + (size_t)m * n;
  double* sx = sl + n;
  double* su = sx + n;
  double* so = su + m;  // L sl
  const int nl = (blocks & 1u) ? n : 0, nxs = (blocks & 2u) ? n : 0, nu = (blocks & 4u) ? m : 0;
  const bool rest = !last && nu > 0;  // (the state block alone needs L only)
  cost_stage_record(rec + kb * cost_record_doubles(n, m), n, m, rest, sL, sLR, sG, lane);
  const double* zk = z + ((size_t)b * d.N + k) * d.rows;
  for (int i = lane; i < n; i += 64) { sl[i] = zk[i]; sx[i] = zk[d.n + i]; }
  if (rest)
    for (int i = lane; i < m; i += 64) su[i] = zk[2 * d.n + i];
  wave_lds_sync();
  cost_knot_S<true>(n, m, !rest, sL, sLR, sG, sl, sx, su, so, sx, su, lane);
  wave_lds_sync();
  double* out = dst + ((size_t)b * nknots + kk) * (nl + nxs + nu);
  for (int i = lane; i < nl; i += 64) out[i] = so[i];
  for (int i = lane; i < nxs; i += 64) out[nl + i] = sx[i];
  for (int i = lane; i < nu; i += 64) out[nl + nxs + i] = last ? 0.0 : su[i];
}

}  // namespace ndlqr
