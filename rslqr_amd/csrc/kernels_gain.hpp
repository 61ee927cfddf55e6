// kernels_gain.hpp -- feedback gains and cost-to-go matrices of the resident problems (ndlqr_hip_feedback_gains; gfx950,
// fp64, runtime-sized in n and m).
//
// The backward recursion in the convention of the reference's Riccati solver: P_{N-1} = Q_{N-1}, p_{N-1} = q_{N-1}, and for
// k = N-2 .. 0, with d_k the affine term of the dynamics,
//     g = P_{k+1} d_k + p_{k+1}
//     M = [A | B]' P_{k+1} [A | B] + diag(Q_k, R_k)      (Qxx | Qxu ; Qux | Quu)
//     v = [q_k ; r_k] + [A | B]' g                       (Qx ; Qu)
//     Quu = L L',  W = L^-1 Qux,  w = L^-1 Qu
//     K_k = -L^-T W,  k_k = -L^-T w,  P_k = Qxx - W' W,  p_k = Qx - W' w
// so that u_k = K_k x_k + k_k and lambda_k = P_k x_k + p_k on the optimal trajectory.
//
// gain_sweep: one workgroup per problem walks the knots from du.N - 1 down to knot0; P, [A | B] of the knot, T = P [A | B],
// Qux | Qu, Quu and the vectors stay in LDS (gain_layout). It reads the DEVICE arrays AB, QR and rhs (stored negated) with
// the pitches of the device layout `d` and computes in the caller's dimensions `du`: the dummy states and inputs of a
// padded block size never enter, and on a padded horizon the sweep starts at the caller's last knot, of which it takes Q
// and q only -- no [A | B], R, r of that knot and no tail knot is read. PF: [A | B] and the vectors of knot k - 1 travel
// through registers into a second LDS buffer while knot k is computed (the loads are issued at the top of the iteration,
// the LDS stores sit at its end); without it they are loaded into the one buffer once it is dead (behind the two products).
// Six workgroup barriers per knot, plus the 2 m wavefront-local synchronisations of the m x m Cholesky.
// A pivot of Quu that is not > 0 (NaN included) is taken as 1 and counted in fails[problem]: finite input gives finite
// output, nothing is written out of range. No template on the flag mode: the outputs do not depend on the schedule.
//
// gain_map_back (dense-cost mode, section 3.16): the sweep ran on the reduced unit-cost problem; one wavefront per
// (knot, problem) maps K~, k~, P~, p~ back through the knot's record L | L_R | G:
//     K = L_R^-T K~ L' - G,   k = L_R^-T k~,   P = L P~ L' (lower triangle, mirrored),   p = L p~.
#pragma once
#include "kernels_common.hpp"
#include "kernels_cost_knot.hpp"

namespace ndlqr {

// entries of [A | B] a thread carries through registers in the prefetching form
constexpr int kGainPrefetchRegs = 8;

// The LDS map of gain_sweep, in doubles. wp: pitch of the rows of [A | B] and T (odd: a column is read conflict-free);
// ldm: leading dimension of Quu and of W = Qux | Qu, m x (n + 1) (odd, as the triangular factors of kernels_cost.hpp).
// vec: diag Q | diag R | d | q | r of the knot (signs of the caller's).
struct GainLayout {
  int wp, ldm;
  size_t P, AB[2], vec[2], T, W, U, g, p, Qx, total;
};
__host__ __device__ inline GainLayout gain_layout(const int n, const int m, const bool second) {
  GainLayout L;
  const size_t w = (size_t)n + m;
  L.wp = (int)w | 1;
  L.ldm = cost_ld(m);
  size_t at = 0;
  L.P = at; at += (size_t)n * n;
  L.AB[0] = at; at += (size_t)n * L.wp;
  L.AB[1] = second ? at : L.AB[0]; at += second ? (size_t)n * L.wp : 0;
  L.T = at; at += (size_t)n * L.wp;
  L.W = at; at += (size_t)L.ldm * (n + 1);
  L.U = at; at += (size_t)L.ldm * m;
  L.vec[0] = at; at += 3 * (size_t)n + 2 * (size_t)m;
  L.vec[1] = second ? at : L.vec[0]; at += second ? 3 * (size_t)n + 2 * (size_t)m : 0;
  L.g = at; at += n;
  L.p = at; at += n;
  L.Qx = at; at += n;
  L.total = at;
  return L;
}
// does a workgroup of `threads` carry a knot's inputs through its registers?
__host__ __device__ inline bool gain_prefetch_fits(const int n, const int m, const int threads) {
  return (size_t)n * (n + m) <= (size_t)kGainPrefetchRegs * threads && 3 * n + 2 * m <= threads;
}
__host__ __device__ inline size_t gain_map_back_lds(const int n, const int m) {
  return (size_t)n * cost_ld(n) + (size_t)m * cost_ld(m) + (size_t)m * n + 2 * (size_t)cost_ld(m) * (n + 1) + 2 * (size_t)n * n + n;
}

// row a of entry e of a lower triangle packed by rows (e = a (a + 1) / 2 + b, b <= a)
__device__ __forceinline__ int gain_tri_row(const int e) {
  int a = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (a * (a + 1) / 2 > e) --a;
  while ((a + 1) * (a + 2) / 2 <= e) ++a;
  return a;
}

// In-place Cholesky of the lower triangle of the k x k matrix `a` (leading dimension ld) in LDS by ONE wavefront,
// right-looking, a column per step. Returns how many pivots were not > 0 (each taken as 1).
__device__ inline int gain_chol(double* a, const int ld, const int k, const int lane) {
  int bad = 0;
  for (int j = 0; j < k; ++j) {
    const double pv = a[j + ld * j];
    const bool ok = pv > 0.0;
    bad += ok ? 0 : 1;
    const double dj = ok ? sqrt(pv) : 1.0;
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

// The inputs of knot k of one problem (ABb, QRb, rb: the problem's device arrays): entry e < n w of [A | B] (row i = e / w
// as it lies in AB, the pad columns left out), and entry e < 3 n + 2 m of diag Q | diag R | d_k | q_k | r_k.
__device__ __forceinline__ double gain_load_ab(const Dims& d, const int n, const int w, const double* __restrict__ ABb, const int k,
                                               const int e) {
  const int i = e / w, j = e - i * w;
  return ABb[((size_t)k * d.n + i) * d.w + (j < n ? j : d.n + (j - n))];
}
__device__ __forceinline__ double gain_load_vec(const Dims& d, const int n, const int w, const double* __restrict__ QRb,
                                                const double* __restrict__ rb, const int k, const int e) {
  if (e < w) return QRb[(size_t)k * d.w + (e < n ? e : d.n + (e - n))];
  const int f = e - w;
  if (f < n) return -rb[(size_t)(k + 1) * d.rows + f];  // d_k: the lambda rows of knot k + 1
  if (f < 2 * n) return -rb[(size_t)k * d.rows + d.n + (f - n)];
  return -rb[(size_t)k * d.rows + 2 * d.n + (f - 2 * n)];
}

// grid (batch), block 64 .. 256 (a multiple of 64), dynamic LDS gain_layout(n, m, PF).total doubles. PF needs
// gain_prefetch_fits(n, m, blockDim.x). K [batch][nknots][m n], kff [batch][nknots][m], P [batch][nknots][n n],
// p [batch][nknots][n], column-major per knot, any of them null (not written); fails [batch] or null.
template <bool PF>
static __global__ __launch_bounds__(256) void gain_sweep(const Dims du, const Dims d, const double* __restrict__ AB,
                                                         const double* __restrict__ QR, const double* __restrict__ rhs,
                                                         const int knot0, const int nknots, double* __restrict__ K,
                                                         double* __restrict__ kff, double* __restrict__ P,
                                                         double* __restrict__ p, int* __restrict__ fails) {
  extern __shared__ __attribute__((aligned(16))) double gain_lds[];
  const int n = du.n, m = du.m, w = n + m, N = du.N, b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const GainLayout L = gain_layout(n, m, PF);
  const int wp = L.wp, ldm = L.ldm, nvec = 3 * n + 2 * m;
  double* sP = gain_lds + L.P;
  double* sT = gain_lds + L.T;
  double* sW = gain_lds + L.W;  // Qux | Qu, then W | w, then K | k
  double* sU = gain_lds + L.U;  // Quu, then its factor
  double* sg = gain_lds + L.g;
  double* sp = gain_lds + L.p;
  double* sQx = gain_lds + L.Qx;
  const double* ABb = AB + (size_t)b * d.N * d.n * d.w;
  const double* QRb = QR + (size_t)b * d.N * d.w;
  const double* rb = rhs + (size_t)b * d.N * d.rows;
  const int kend = knot0 + nknots;  // knots >= kend are swept, not delivered
  int bad = 0;

  // the last knot: P = diag Q, p = q; its K, k are zero
  for (int e = tid; e < n * n; e += nt) {
    const int j = e / n, i = e - j * n;
    sP[e] = i == j ? QRb[(size_t)(N - 1) * d.w + i] : 0.0;
  }
  for (int i = tid; i < n; i += nt) sp[i] = -rb[(size_t)(N - 1) * d.rows + d.n + i];
  if (N - 2 >= knot0) {
    for (int e = tid; e < n * w; e += nt) gain_lds[L.AB[0] + (e / w) * wp + (e % w)] = gain_load_ab(d, n, w, ABb, N - 2, e);
    for (int e = tid; e < nvec; e += nt) gain_lds[L.vec[0] + e] = gain_load_vec(d, n, w, QRb, rb, N - 2, e);
  }
  __syncthreads();
  if (kend == N) {
    const size_t ob = (size_t)b * nknots + (N - 1 - knot0);
    if (K) for (int e = tid; e < m * n; e += nt) K[ob * m * n + e] = 0.0;
    if (kff) for (int e = tid; e < m; e += nt) kff[ob * m + e] = 0.0;
    if (P) for (int e = tid; e < n * n; e += nt) P[ob * n * n + e] = sP[e];
    if (p) for (int e = tid; e < n; e += nt) p[ob * n + e] = sp[e];
  }

  int cb = 0;
  for (int k = N - 2; k >= knot0; --k) {
    const double* sAB = gain_lds + (cb ? L.AB[1] : L.AB[0]);
    const double* sQR = gain_lds + (cb ? L.vec[1] : L.vec[0]);
    double* oAB = gain_lds + (cb ? L.AB[0] : L.AB[1]);  // the other buffer (PF)
    double* ovec = gain_lds + (cb ? L.vec[0] : L.vec[1]);
    const double* sd = sQR + w;
    const double* sq = sd + n;  // q | r: w entries
    const bool more = k > knot0;
    double pf[kGainPrefetchRegs] = {}, pv = 0.0;
    if constexpr (PF) {  // knot k - 1 on its way: nothing below waits for these loads before the stores at the end
#pragma unroll
      for (int u = 0; u < kGainPrefetchRegs; ++u) {
        const int e = tid + u * nt;
        if (more && e < n * w) pf[u] = gain_load_ab(d, n, w, ABb, k - 1, e);
      }
      if (more && tid < nvec) pv = gain_load_vec(d, n, w, QRb, rb, k - 1, tid);
    }
    // T = P [A | B] and g = P d + p
    for (int e = tid; e < n * w + n; e += nt) {
      if (e < n * w) {
        const int i = e / w, j = e - i * w;
        double s = 0.0;
        for (int c = 0; c < n; ++c) s = fma(sP[c + n * i], sAB[c * wp + j], s);
        sT[i * wp + j] = s;
      } else {
        const int i = e - n * w;
        double s = sp[i];
        for (int c = 0; c < n; ++c) s = fma(sP[c + n * i], sd[c], s);
        sg[i] = s;
      }
    }
    __syncthreads();  // P is dead
    // the lower triangle of M = [A | B]' T + diag(Q, R): Qxx into P's storage, Qux, Quu; v = [q ; r] + [A | B]' g
    const int tri = w * (w + 1) / 2;
    for (int e = tid; e < tri + w; e += nt) {
      if (e < tri) {
        const int a = gain_tri_row(e), c = e - a * (a + 1) / 2;
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(sAB[i * wp + a], sT[i * wp + c], s);
        if (a == c) s += sQR[a];
        if (a < n) sP[a + n * c] = s;
        else if (c < n) sW[(a - n) + ldm * c] = s;
        else sU[(a - n) + ldm * (c - n)] = s;
      } else {
        const int a = e - tri;
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = fma(sAB[i * wp + a], sg[i], s);
        s += sq[a];
        if (a < n) sQx[a] = s;
        else sW[(a - n) + ldm * n] = s;
      }
    }
    __syncthreads();  // [A | B] and the vectors of the knot are dead
    if (tid < 64) bad += gain_chol(sU, ldm, m, tid);
    if (!PF && more) {
      for (int e = tid; e < n * w; e += nt) gain_lds[L.AB[0] + (e / w) * wp + (e % w)] = gain_load_ab(d, n, w, ABb, k - 1, e);
      for (int e = tid; e < nvec; e += nt) gain_lds[L.vec[0] + e] = gain_load_vec(d, n, w, QRb, rb, k - 1, e);
    }
    __syncthreads();
    // W | w = L^-1 (Qux | Qu): a column per thread
    for (int c = tid; c <= n; c += nt) {
      double* x = sW + (size_t)ldm * c;
      for (int j = 0; j < m; ++j) {
        double s = x[j];
        for (int l = 0; l < j; ++l) s = fma(-sU[j + ldm * l], x[l], s);
        x[j] = s / sU[j + ldm * j];
      }
    }
    __syncthreads();
    // P = Qxx - W' W (lower triangle, mirrored), p = Qx - W' w
    const int trin = n * (n + 1) / 2;
    for (int e = tid; e < trin + n; e += nt) {
      if (e < trin) {
        const int i = gain_tri_row(e), j = e - i * (i + 1) / 2;
        double s = sP[i + n * j];
        for (int c = 0; c < m; ++c) s = fma(-sW[c + ldm * i], sW[c + ldm * j], s);
        sP[i + n * j] = s;
        sP[j + n * i] = s;
      } else {
        const int i = e - trin;
        double s = sQx[i];
        for (int c = 0; c < m; ++c) s = fma(-sW[c + ldm * i], sW[c + ldm * n], s);
        sp[i] = s;
      }
    }
    __syncthreads();
    // K | k = -L^-T (W | w), in place
    for (int c = tid; c <= n; c += nt) {
      double* x = sW + (size_t)ldm * c;
      for (int j = m - 1; j >= 0; --j) {
        double s = -x[j];
        for (int l = j + 1; l < m; ++l) s = fma(-sU[l + ldm * j], x[l], s);
        x[j] = s / sU[j + ldm * j];
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int u = 0; u < kGainPrefetchRegs; ++u) {
        const int e = tid + u * nt;
        if (more && e < n * w) oAB[(e / w) * wp + (e % w)] = pf[u];
      }
      if (more && tid < nvec) ovec[tid] = pv;
    }
    __syncthreads();
    if (k < kend) {  // (the next knot writes W and P behind its first barrier)
      const size_t ob = (size_t)b * nknots + (k - knot0);
      if (K) for (int e = tid; e < m * n; e += nt) K[ob * m * n + e] = sW[(e % m) + ldm * (e / m)];
      if (kff) for (int e = tid; e < m; e += nt) kff[ob * m + e] = sW[e + ldm * n];
      if (P) for (int e = tid; e < n * n; e += nt) P[ob * n * n + e] = sP[e];
      if (p) for (int e = tid; e < n; e += nt) p[ob * n + e] = sp[e];
    }
    if (PF) cb ^= 1;
  }
  if (fails && tid == 0) fails[b] = bad;
}

// grid (nknots, batch), block 64, dynamic LDS gain_map_back_lds(n, m) doubles. rec: the records of the batch
// [batch][N][cost_record_doubles]; Kt, kt, Pt, pt: the sweep's outputs on the reduced problem for the knots
// [knot0, knot0 + nknots); K, kff, P, p: the caller's, any of them null.
static __global__ __launch_bounds__(64) void gain_map_back(const int n, const int m, const int N, const int knot0,
                                                           const int nknots, const double* __restrict__ rec,
                                                           const double* __restrict__ Kt, const double* __restrict__ kt,
                                                           const double* __restrict__ Pt, const double* __restrict__ pt,
                                                           double* __restrict__ K, double* __restrict__ kff,
                                                           double* __restrict__ P, double* __restrict__ p) {
  extern __shared__ __attribute__((aligned(16))) double gain_lds[];
  const int kk = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, k = knot0 + kk;
  const bool last = k == N - 1;
  const int ldn = cost_ld(n), ldm = cost_ld(m);
  const size_t ob = (size_t)b * nknots + kk;
  double* sL = gain_lds;
  double* sLR = sL + (size_t)n * ldn;
  double* sG = sLR + (size_t)m * ldm;
  double* sX = sG + (size_t)m * n;            // K~ | k~, m x (n + 1)
  double* sY = sX + (size_t)ldm * (n + 1);    // K~ L' | k~, then L_R^-T of it
  double* sPt = sY + (size_t)ldm * (n + 1);   // P~, then P
  double* sZ = sPt + (size_t)n * n;           // P~ L'
  double* sv = sZ + (size_t)n * n;            // p~
  cost_stage_record(rec + ((size_t)b * N + k) * cost_record_doubles(n, m), n, m, !last, sL, sLR, sG, lane);
  for (int e = lane; e < m * n; e += 64) sX[(e % m) + ldm * (e / m)] = Kt[ob * m * n + e];
  for (int e = lane; e < m; e += 64) sX[e + ldm * n] = kt[ob * m + e];
  for (int e = lane; e < n * n; e += 64) sPt[e] = Pt[ob * n * n + e];
  for (int e = lane; e < n; e += 64) sv[e] = pt[ob * n + e];
  wave_lds_sync();
  if (last) {  // the record is L | 1 | 0 and K~ = 0, k~ = 0
    if (K) for (int e = lane; e < m * n; e += 64) K[ob * m * n + e] = 0.0;
    if (kff) for (int e = lane; e < m; e += 64) kff[ob * m + e] = 0.0;
  } else if (K || kff) {
    for (int e = lane; e < m * (n + 1); e += 64) {
      const int i = e / m, j = e - i * m;
      double s = sX[j + ldm * i];
      if (i < n) {
        s = 0.0;
        for (int c = 0; c <= i; ++c) s = fma(sX[j + ldm * c], sL[i + ldn * c], s);
      }
      sY[j + ldm * i] = s;
    }
    wave_lds_sync();
    for (int c = lane; c <= n; c += 64) {  // L_R^-T: a column per lane
      double* x = sY + (size_t)ldm * c;
      for (int j = m - 1; j >= 0; --j) {
        double s = x[j];
        for (int l = j + 1; l < m; ++l) s = fma(-sLR[l + ldm * j], x[l], s);
        x[j] = s / sLR[j + ldm * j];
      }
    }
    wave_lds_sync();
    if (K) for (int e = lane; e < m * n; e += 64) K[ob * m * n + e] = sY[(e % m) + ldm * (e / m)] - sG[e];
    if (kff) for (int e = lane; e < m; e += 64) kff[ob * m + e] = sY[e + ldm * n];
  }
  if (p)
    for (int i = lane; i < n; i += 64) {
      double s = 0.0;
      for (int c = 0; c <= i; ++c) s = fma(sL[i + ldn * c], sv[c], s);
      p[ob * n + i] = s;
    }
  if (!P) return;
  for (int e = lane; e < n * n; e += 64) {  // Z = P~ L'
    const int i = e / n, a = e - i * n;
    double s = 0.0;
    for (int c = 0; c <= i; ++c) s = fma(sPt[a + n * c], sL[i + ldn * c], s);
    sZ[e] = s;
  }
  wave_lds_sync();
  for (int e = lane; e < n * n; e += 64) {  // P = L Z: the lower triangle, mirrored
    const int j = e / n, i = e - j * n;
    if (i < j) continue;
    double s = 0.0;
    for (int a = 0; a <= i; ++a) s = fma(sL[i + ldn * a], sZ[a + n * j], s);
    sPt[i + n * j] = s;
    sPt[j + n * i] = s;
  }
  wave_lds_sync();
  for (int e = lane; e < n * n; e += 64) P[ob * n * n + e] = sPt[e];
}

}  // namespace ndlqr
