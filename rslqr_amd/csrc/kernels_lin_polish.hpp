// kernels_lin_polish.hpp -- internal: the active-set polish of the solve with linear inequality rows
// (ndlqr_hip_polish_constrained).
//
// Section 3.13 carried from entries to rows. With G_k = [C_k D_k] (C alone at the last knot), A the active rows and c the
// bound each is active at, the constrained solution solves K z + G_A' mu = b, G_A z = c_A, K and b the dense-cost KKT
// system in the CALLER's variables. The polish runs the method of multipliers on it: with the costs shifted by
// sigma_p G_A' G_A (lin_polish_shift_cost; reduced and factored once per round by the host), a step is
//     r_z = b - K z - G_A' mu,   r_c = c_A - G_A z         lin_polish_residual, on the UNSHIFTED problem
//     rhs = r_z + sigma_p G_A' r_c                          (the same launch), S^' rhs: lin_polish_apply_t
//     K^ delta = rhs                                        re-solve against the kept factorisation, delta = S^ delta~
//     z+ = z + delta,   mu+_A = mu_A + sigma_p (G_A delta - r_c)      lin_polish_update
// A step is a candidate (zc, muc) until its norm max(|r_z|_inf, |r_c|_inf) is known: lin_polish_update commits the
// previous candidate when refine_accepted says so and stops the problem otherwise. Unlike the box polish an active row
// cannot be put onto its bound by assignment: it holds to the floor of the residual, not bit for bit.
//
// Layouts as in kernels_lin.hpp: the caller's block sizes `u` for the flat inputs, the records, C, D and everything per
// row ([batch][N][p]: codes, mu, muc, rc, v, y; the bounds with bstride); the device layout `d` for z, zc, z0, the
// right-hand sides and delta~ ([batch][d.N][2 d.n + d.m]: row i of lambda | x | u of knot k at k d.rows + (i | d.n + i |
// 2 d.n + i)). Pad entries and the knots k >= u.N of a padded horizon are rows of zeros in every right-hand side written
// here and are never touched in z.
// Row codes: 0 unbounded, 1 bounded and inactive, 2 active at lo, 3 active at hi. Problem states: those of
// kernels_box_polish.hpp (0 running, 4 stopped until the round's validation, 1 polished, 2 not polished, 3 not finite).
// Every sum runs in one fixed order (the unit is compiled with contraction off); the rows of the residual are accumulated
// in double-double (kernels_dd.hpp) and rounded once, as kkt_residual_dd's -- a float64 chain leaves every row at its
// evaluation error, several times the floor a direct solve reaches --: the residual does not depend on the mode. STRICT (lin_polish_update alone): t = sigma_p (G delta - r_c) rounded, then mu + t.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box_core.hpp"
#include "kernels_cost_knot.hpp"
#include "kernels_dd.hpp"
#include "kernels_lin_shift.hpp"

namespace ndlqr {

enum { LIN_POLISH_RUNNING = 0, LIN_POLISH_DONE = 1, LIN_POLISH_KEPT = 2, LIN_POLISH_NAN = 3, LIN_POLISH_STOPPED = 4 };

// odd pitch of a matrix staged in LDS that is walked along its rows and along its columns
__host__ __device__ inline int lin_polish_pitch(int k) { return k | 1; }
// doubles of LDS of lin_polish_residual: Q | H | R | A | B | C | D, then lambda_k, x_k, u_k, lambda_{k+1}, x_{k+1}, mu_A, r_c
__host__ __device__ inline size_t lin_polish_residual_lds(int n, int m, int p) {
  return (size_t)n * n + (size_t)m * lin_polish_pitch(n) + (size_t)m * m + (size_t)n * lin_polish_pitch(n) +
         (size_t)m * lin_polish_pitch(n) + (size_t)n * lin_polish_pitch(p) + (size_t)m * lin_polish_pitch(p) + 4 * (size_t)n + m +
         2 * (size_t)p;
}
// doubles of LDS one wavefront of lin_polish_update / lin_polish_apply_t stages for its knot: the record, C, D and the
// vectors lambda~ | x | u~ | u | delta lambda
__host__ __device__ inline size_t lin_polish_wave_lds(int n, int m, int p) {
  return (size_t)n * cost_ld(n) + (size_t)m * cost_ld(m) + (size_t)m * n + (size_t)p * n + (size_t)p * m + 3 * (size_t)n +
         2 * (size_t)m;
}

// w = C x + D u of one row: j ascending, C before D, from zero (the order of lin_update_knot). cs, ds: the stride between
// the columns of the row in C and D; D == nullptr (the last knot): C x alone.
__device__ __forceinline__ double lin_polish_row(const double* C, const int cs, const double* D, const int ds, const double* x,
                                                 const double* uu, const int n, const int m) {
  double w = 0.0;
  for (int j = 0; j < n; ++j) w = fma(C[(size_t)cs * j], x[j], w);
  if (D)
    for (int j = 0; j < m; ++j) w = fma(D[(size_t)ds * j], uu[j], w);
  return w;
}

// sig[b] = (sigma * the largest entry of diag Q, diag R of problem b) / g2, g2 the largest squared row norm of the
// problem's bounded rows of [C D] (R, D of the last knot left out; a problem without a bounded row: g2 = 1). Every
// product and sum rounded on its own, j ascending, C before D: numpy gives the same bits. A NaN entry gives a NaN.
//   grid (batch), block 256.
static __global__ __launch_bounds__(256) void lin_polish_sigma(Dims u, int p, double sigma, const double* __restrict__ Q,
                                                               const double* __restrict__ R, const double* __restrict__ C,
                                                               const double* __restrict__ D, const double* __restrict__ lo,
                                                               const double* __restrict__ hi, size_t bstride,
                                                               double* __restrict__ sig) {
  __shared__ double red[2][256];
  const int b = blockIdx.x, tid = threadIdx.x, n = u.n, m = u.m, N = u.N;
  double big = 0.0, g2 = 0.0;
  for (unsigned e = tid; e < (unsigned)(N * (n + m)); e += blockDim.x) {
    const unsigned k = e / (unsigned)(n + m), j = e - k * (unsigned)(n + m);
    const size_t kb = (size_t)b * N + k;
    if (j < (unsigned)n) big = max_nan(big, Q[kb * n * n + j + (size_t)n * j]);
    else if ((int)k < N - 1) big = max_nan(big, R[kb * m * m + (j - n) + (size_t)m * (j - n)]);
  }
  for (unsigned e = tid; e < (unsigned)(N * p); e += blockDim.x) {
    const unsigned k = e / (unsigned)p, r = e - k * (unsigned)p;
    if (!box_bounded(lo[(size_t)b * bstride + e], hi[(size_t)b * bstride + e])) continue;
    const size_t kb = (size_t)b * N + k;
    const double* Cr = C + kb * p * n + r;
    const double* Dr = D + kb * p * m + r;
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
      const double t = Cr[(size_t)p * j] * Cr[(size_t)p * j];
      s = s + t;
    }
    if ((int)k < N - 1)
      for (int j = 0; j < m; ++j) {
        const double t = Dr[(size_t)p * j] * Dr[(size_t)p * j];
        s = s + t;
      }
    g2 = max_nan(g2, s);
  }
  red[0][tid] = big;
  red[1][tid] = g2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] = max_nan(red[0][tid], red[0][tid + s]);
      red[1][tid] = max_nan(red[1][tid], red[1][tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double num = sigma * red[0][0];
    sig[b] = num / (red[1][0] > 0.0 || red[1][0] != red[1][0] ? red[1][0] : 1.0);
  }
}

// Start of a polish: the resident solution zs saved into z0 and taken as z (pad entries and pad knots included); codes
// from the exact comparisons of the ADMM iterate with its bounds -- 3: v == hi && y > 0, or lo == hi; 2: v == lo && y < 0;
// 1: bounded otherwise; 0: unbounded --; mu = rho y on the active rows, 0 elsewhere; state 3 for a problem whose
// constrained solve ended non-finite, 2 (kept as it is) for one that was certified infeasible (status 4), 0 otherwise
// (counted in *running); no steps yet.
//   grid (d.N, batch), block 64.
static __global__ void lin_polish_start(Dims u, Dims d, int p, const double* __restrict__ rhov, const double* __restrict__ lo,
                                        const double* __restrict__ hi, size_t bstride, const double* __restrict__ v,
                                        const double* __restrict__ y, const int* __restrict__ lin_status,
                                        const double* __restrict__ zs, double* __restrict__ z0, double* __restrict__ z,
                                        unsigned char* __restrict__ code, double* __restrict__ mu, int* __restrict__ state,
                                        int* __restrict__ steps, int* __restrict__ here, int* __restrict__ running) {
  const int k = blockIdx.x, b = blockIdx.y;
  if (k == 0 && threadIdx.x == 0) {
    const int st = lin_status[b];
    const bool run = st != 3 && st != 4;
    state[b] = run ? LIN_POLISH_RUNNING : st == 3 ? LIN_POLISH_NAN : LIN_POLISH_KEPT;
    if (run) atomicAdd(running, 1);
    steps[b] = 0;
    here[b] = 0;
  }
  const size_t oz = ((size_t)b * d.N + k) * d.rows;
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    const double zr = zs[oz + r];
    z0[oz + r] = zr;
    z[oz + r] = zr;
  }
  if (k >= u.N) return;
  const double rho = rhov[b];
  const size_t ov = ((size_t)b * u.N + k) * p, ob = (size_t)b * bstride + (size_t)k * p;
  for (int r = threadIdx.x; r < p; r += blockDim.x) {
    const double l = lo[ob + r], h = hi[ob + r], vr = v[ov + r], yr = y[ov + r];
    unsigned char cd = 0;
    double m = 0.0;
    if (box_bounded(l, h)) {
      cd = ((vr == h && yr > 0.0) || l == h) ? 3 : (vr == l && yr < 0.0) ? 2 : 1;
      if (cd >= 2) m = rho * yr;
    }
    code[ov + r] = cd;
    mu[ov + r] = m;
  }
}

// the row weights of the polish: sigma_p on the active rows
struct LinPolishWeight {
  const unsigned char* code;  // the knot's codes
  double s;
  __device__ __forceinline__ double operator()(int r) const { return code[r] >= 2 ? s : 0.0; }
};

// lin_shift_cost with the row weights sig[b] [code >= 2] instead of rho[b] [bounded] (the shared body of
// kernels_lin_shift.hpp).
//   grid (N, batch), block 64, dynamic LDS lin_shift_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_polish_shift_cost(const int n, const int m, const int N, const int p,
                                                                   const double* __restrict__ sig,
                                                                   const unsigned char* __restrict__ code,
                                                                   const double* __restrict__ Q, const double* __restrict__ H,
                                                                   const double* __restrict__ R, const double* __restrict__ C,
                                                                   const double* __restrict__ D, double* __restrict__ Qs,
                                                                   double* __restrict__ Hs, double* __restrict__ Rs) {
  extern __shared__ __attribute__((aligned(16))) double lin_polish_lds[];
  const int k = blockIdx.x, b = blockIdx.y;
  const LinPolishWeight weight = {code + ((size_t)b * N + k) * p, sig[b]};
  lin_shift_cost_knot(lin_polish_lds, n, m, N, p, k, b, weight, Q, H, R, C, D, Qs, Hs, Rs, threadIdx.x);
}

// The residual of the active-set system of (z, mu) on the unshifted problem, and the right-hand side of the correction.
// Workgroup (k, b), k < u.N: the x and u rows of knot k, the lambda rows of knot k + 1 (k < u.N - 1), workgroup 0 also
// those of knot 0 -- so only [A_k | B_k] is needed --, and the knot's p constraint rows:
//     row lambda_0:      -x0 + x_0                                 row r:  r_c = c - (C x + D u) on the active rows, else 0
//     row lambda_{k+1}:  -d_k + x_{k+1} - A_k x_k - B_k u_k
//     row x_k:  -q_k + lambda_k - Q_k x_k - H_k u_k - A_k' lambda_{k+1} - C_k' mu_A   (r_z)   + sig (C_k' r_c)   (rhs)
//     row u_k:  -r_k - H_k' x_k - R_k u_k - B_k' lambda_{k+1} - D_k' mu_A             (r_z)   + sig (D_k' r_c)   (rhs)
// r_z, r_c and the lambda rows each accumulated in double-double (dd_fma, dd_term) in exactly this term order, j (or r)
// ascending inside a term, and rounded once; G_A' r_c is a chain of fma and enters by one more fma. The last knot has
// neither u row nor the H, A terms, and A, B, R, H, D, r, d of it are never loaded. rhs gets the right-hand side in the caller's variables
// (device layout; pad entries zero), rc [batch][N][p] the constraint residual r_c, and slot `slot` of the norms (bit
// patterns, as kkt_residual_dd's) the per-problem maxima: set 0 max(|r_z|_inf, |r_c|_inf), set 1 |r_c|_inf.
// Workgroups k >= u.N (a padded horizon) write rows of zeros. state != nullptr: a problem that is not running is
// skipped, and so is one whose chain has broken (slot >= 2, refine_accepted false for slot - 1).
//   grid (d.N, batch), block 64, dynamic LDS lin_polish_residual_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_polish_residual(
    Dims u, Dims d, int p, const double* __restrict__ sig, const double* __restrict__ A, const double* __restrict__ B,
    const double* __restrict__ Q, const double* __restrict__ H, const double* __restrict__ R, const double* __restrict__ q,
    const double* __restrict__ rr, const double* __restrict__ dd, const double* __restrict__ x0, const double* __restrict__ C,
    const double* __restrict__ D, const double* __restrict__ lo, const double* __restrict__ hi, size_t bstride,
    const unsigned char* __restrict__ code, const double* __restrict__ z, const double* __restrict__ mu,
    const int* __restrict__ state, double* __restrict__ rhs, double* __restrict__ rc, unsigned long long* __restrict__ norms,
    const int nslots, const int slot) {
  extern __shared__ __attribute__((aligned(16))) double lin_polish_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int n = u.n, m = u.m, N = u.N;
  if (state && state[b] != LIN_POLISH_RUNNING) return;  // (uniform over the workgroup)
  if (state && slot >= 2 && !refine_accepted(norms, d.batch, b, slot - 1)) return;
  const size_t ok = ((size_t)b * d.N + k) * d.rows;
  if (k >= N) {
    for (int r = lane; r < d.rows; r += 64) rhs[ok + r] = 0.0;
    return;
  }
  const bool last = k == N - 1;
  const size_t kb = (size_t)b * N + k;
  const int pn = lin_polish_pitch(n), pp = lin_polish_pitch(p);
  double* sQ = lin_polish_lds;              // [n][n] symmetric
  double* sH = sQ + (size_t)n * n;          // H(i, j) at i + pn j
  double* sR = sH + (size_t)m * pn;         // [m][m] symmetric
  double* sA = sR + (size_t)m * m;          // A(i, j) at i + pn j
  double* sB = sA + (size_t)n * pn;         // B(i, j) at i + pn j
  double* sC = sB + (size_t)m * pn;         // C(r, j) at r + pp j
  double* sD = sC + (size_t)n * pp;         // D(r, j) at r + pp j
  double* sl = sD + (size_t)m * pp;         // lambda_k
  double* sx = sl + n;
  double* su = sx + n;
  double* sl1 = su + m;                     // lambda_{k+1}
  double* sx1 = sl1 + n;                    // x_{k+1}
  double* smu = sx1 + n;                    // mu on the active rows, 0 elsewhere
  double* src = smu + p;                    // r_c
  {
    const double* Qk = Q + kb * n * n;
    for (int idx = lane; idx < n * n; idx += 64) {
      const int j = idx / n, i = idx - j * n;
      sQ[idx] = i >= j ? Qk[idx] : Qk[j + n * i];
    }
    const double* Ck = C + kb * p * n;
    for (int idx = lane; idx < p * n; idx += 64) {
      const int j = idx / p;
      sC[idx - j * p + pp * j] = Ck[idx];
    }
    for (int i = lane; i < n; i += 64) {
      sl[i] = z[ok + i];
      sx[i] = z[ok + d.n + i];
    }
    for (int r = lane; r < p; r += 64) smu[r] = code[kb * p + r] >= 2 ? mu[kb * p + r] : 0.0;
    if (!last) {
      const double* Hk = H ? H + kb * n * m : nullptr;
      const double* Bk = B + kb * n * m;
      for (int idx = lane; idx < n * m; idx += 64) {
        const int j = idx / n;
        sH[idx - j * n + pn * j] = Hk ? Hk[idx] : 0.0;
        sB[idx - j * n + pn * j] = Bk[idx];
      }
      const double* Rk = R + kb * m * m;
      for (int idx = lane; idx < m * m; idx += 64) {
        const int j = idx / m, i = idx - j * m;
        sR[idx] = i >= j ? Rk[idx] : Rk[j + m * i];
      }
      const double* Ak = A + kb * n * n;
      for (int idx = lane; idx < n * n; idx += 64) {
        const int j = idx / n;
        sA[idx - j * n + pn * j] = Ak[idx];
      }
      const double* Dk = D + kb * p * m;
      for (int idx = lane; idx < p * m; idx += 64) {
        const int j = idx / p;
        sD[idx - j * p + pp * j] = Dk[idx];
      }
      for (int j = lane; j < m; j += 64) su[j] = z[ok + 2 * d.n + j];
      for (int i = lane; i < n; i += 64) {
        sl1[i] = z[ok + d.rows + i];
        sx1[i] = z[ok + d.rows + d.n + i];
      }
    }
  }
  wave_lds_sync();
  // non-negative doubles (or NaN with the sign bit clear): the order of the bit patterns is the order of the values
  unsigned long long pz = 0ull, pc = 0ull;
  const auto note = [](unsigned long long& at, double val) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(val));
    at = bits > at ? bits : at;
  };
  // the constraint rows
  double unused = 0.0;  // (the scale dd_fma keeps for the refinement's eta: not needed here)
  for (int r = lane; r < p; r += 64) {
    const unsigned char cd = code[kb * p + r];
    double res = 0.0;
    if (cd >= 2) {
      const size_t ob = (size_t)b * bstride + (size_t)k * p + r;
      DD acc = {cd == 3 ? hi[ob] : lo[ob], 0.0};
      for (int j = 0; j < n; ++j) dd_fma(acc, unused, -sC[r + pp * j], sx[j]);
      if (!last)
        for (int j = 0; j < m; ++j) dd_fma(acc, unused, -sD[r + pp * j], su[j]);
      res = acc.hi + acc.lo;
    }
    src[r] = res;
    rc[kb * p + r] = res;
    note(pc, res);
  }
  wave_lds_sync();
  // the x and u rows of knot k
  for (int t = lane; t < n + (last ? 0 : m); t += 64) {
    DD acc;
    double g = 0.0;
    if (t < n) {
      const int i = t;
      acc = {-q[kb * n + i], 0.0};
      dd_term(acc, unused, sl[i]);
      for (int j = 0; j < n; ++j) dd_fma(acc, unused, -sQ[i + n * j], sx[j]);
      if (!last) {
        for (int j = 0; j < m; ++j) dd_fma(acc, unused, -sH[i + pn * j], su[j]);
        for (int j = 0; j < n; ++j) dd_fma(acc, unused, -sA[j + pn * i], sl1[j]);
      }
      for (int r = 0; r < p; ++r) dd_fma(acc, unused, -sC[r + pp * i], smu[r]);
      for (int r = 0; r < p; ++r) g = fma(sC[r + pp * i], src[r], g);
    } else {
      const int j = t - n;
      acc = {-rr[kb * m + j], 0.0};
      for (int i = 0; i < n; ++i) dd_fma(acc, unused, -sH[i + pn * j], sx[i]);
      for (int i = 0; i < m; ++i) dd_fma(acc, unused, -sR[j + m * i], su[i]);
      for (int i = 0; i < n; ++i) dd_fma(acc, unused, -sB[i + pn * j], sl1[i]);
      for (int r = 0; r < p; ++r) dd_fma(acc, unused, -sD[r + pp * j], smu[r]);
      for (int r = 0; r < p; ++r) g = fma(sD[r + pp * j], src[r], g);
    }
    const double rz = acc.hi + acc.lo;
    note(pz, rz);
    rhs[ok + (t < n ? d.n + t : 2 * d.n + (t - n))] = fma(sig[b], g, rz);
  }
  // the lambda rows of knot k + 1, and of knot 0
  if (!last)
    for (int i = lane; i < n; i += 64) {
      DD acc = {-dd[kb * n + i], 0.0};
      dd_term(acc, unused, sx1[i]);
      for (int j = 0; j < n; ++j) dd_fma(acc, unused, -sA[i + pn * j], sx[j]);
      for (int j = 0; j < m; ++j) dd_fma(acc, unused, -sB[i + pn * j], su[j]);
      const double rl = acc.hi + acc.lo;
      note(pz, rl);
      rhs[ok + d.rows + i] = rl;
    }
  if (k == 0)
    for (int i = lane; i < n; i += 64) {
      DD acc = {-x0[(size_t)b * n + i], 0.0};
      dd_term(acc, unused, sx[i]);
      const double rl = acc.hi + acc.lo;
      note(pz, rl);
      rhs[ok + i] = rl;
    }
  // the pad entries of this knot's block (a padded block size), and of the u rows of the last knot
  for (int r = lane; r < d.rows; r += 64) {
    const int blk = r < d.n ? 0 : (r < 2 * d.n ? 1 : 2), i = r - blk * d.n;
    if (blk < 2 ? i >= n : (i >= m || last)) rhs[ok + r] = 0.0;
  }
  if (!norms) return;
  pz = pc > pz ? pc : pz;
  // over the wavefront: the maxima of the bit patterns
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long oz2 = __shfl_xor(pz, off), oc2 = __shfl_xor(pc, off);
    pz = oz2 > pz ? oz2 : pz;
    pc = oc2 > pc ? oc2 : pc;
  }
  if (lane == 0) {
    if (pz) atomicMax(norms + (size_t)slot * d.batch + b, pz);
    if (pc) atomicMax(norms + ((size_t)nslots + slot) * d.batch + b, pc);
  }
}

// One wavefront's LDS of lin_polish_update / lin_polish_apply_t (lin_polish_wave_lds doubles at `base`).
struct LinPolishKnotLds {
  double *sL, *sLR, *sG, *sC, *sD, *sl, *sx, *su, *ux, *dl;
  __device__ __forceinline__ LinPolishKnotLds(double* base, int n, int m, int p) {
    sL = base;
    sLR = sL + (size_t)n * cost_ld(n);
    sG = sLR + (size_t)m * cost_ld(m);
    sC = sG + (size_t)m * n;
    sD = sC + (size_t)p * n;
    sl = sD + (size_t)p * m;  // lambda~ of the knot
    sx = sl + n;              // x~, then x
    su = sx + n;              // u~
    ux = su + m;              // u in the caller's variables
    dl = ux + m;              // lambda in the caller's variables
  }
};

// S^' (the polish records `rec`) on the right-hand side `r` of lin_polish_residual, knot by knot (cost_knot_St): rt gets
// the reduced right-hand side of the re-solve; pad entries and the knots k >= u.N: zero. Problems that are not running
// are skipped (state may be null).
//   grid (d.N, batch), block 64, dynamic LDS lin_polish_wave_lds(n, m, p) doubles.
static __global__ __launch_bounds__(64) void lin_polish_apply_t(Dims u, Dims d, int p, const double* __restrict__ rec,
                                                                const double* __restrict__ r, const int* __restrict__ state,
                                                                double* __restrict__ rt) {
  extern __shared__ __attribute__((aligned(16))) double lin_polish_lds[];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (state && state[b] != LIN_POLISH_RUNNING) return;  // (uniform over the workgroup)
  const int n = u.n, m = u.m;
  const size_t ok = ((size_t)b * d.N + k) * d.rows;
  const bool real = k < u.N, last = k == u.N - 1;
  for (int e = lane; e < d.rows; e += 64) {
    const int blk = e < d.n ? 0 : (e < 2 * d.n ? 1 : 2), i = e - blk * d.n;
    if (!(real && (blk < 2 ? i < n : (i < m && !last)))) rt[ok + e] = 0.0;
  }
  if (!real) return;
  const LinPolishKnotLds S(lin_polish_lds, n, m, p);
  cost_stage_record(rec + ((size_t)b * u.N + k) * cost_record_doubles(n, m), n, m, !last, S.sL, S.sLR, S.sG, lane);
  for (int i = lane; i < n; i += 64) {
    S.sl[i] = r[ok + i];
    S.sx[i] = r[ok + d.n + i];
  }
  if (!last)
    for (int j = lane; j < m; j += 64) S.su[j] = r[ok + 2 * d.n + j];
  wave_lds_sync();
  cost_knot_St<true, true>(n, m, last, S.sL, S.sLR, S.sG, S.sl, S.sx, S.su, rt + ok, rt + ok + d.n, rt + ok + 2 * d.n, lane);
}

// Step `step` (1-based) of every running problem, after the re-solve of the right-hand side of slot step - 1 into the
// reduced correction `delta`. step >= 2: the candidate of step - 1 is committed -- z, mu <- zc, muc on the entries of the
// caller's problem, here[b] = step - 1 -- when refine_accepted(norms, step - 1) holds; otherwise the problem stops (state
// 4) with what it has, and the running count drops by one. form != 0: the next candidate, knot by knot, the four
// wavefronts taking the knots k < u.N round-robin: the polish record and C, D staged, delta = S^ delta~ (cost_knot_S),
//     zc = z + delta;   on the active rows  muc = mu + sig (G delta - rc);   elsewhere muc = 0
// with rc the constraint residual lin_polish_residual left of the iterate that is now z. A problem whose candidate is not
// finite ends as state 3 (the reductions keep a NaN). form == 0 (behind the last step): the commit alone. One lane owns the
// same entries in both parts.
//   grid (batch), block 256, dynamic LDS 4 lin_polish_wave_lds(n, m, p) doubles.
template <bool STRICT>
__global__ __launch_bounds__(256) void lin_polish_update(Dims u, Dims d, int p, int step, int form,
                                                         const unsigned long long* __restrict__ norms,
                                                         const double* __restrict__ sig, const double* __restrict__ rec,
                                                         const double* __restrict__ C, const double* __restrict__ D,
                                                         const unsigned char* __restrict__ code, const double* __restrict__ rc,
                                                         const double* __restrict__ delta, double* __restrict__ z,
                                                         double* __restrict__ mu, double* __restrict__ zc,
                                                         double* __restrict__ muc, int* __restrict__ state,
                                                         int* __restrict__ here, int* __restrict__ running) {
  extern __shared__ __attribute__((aligned(16))) double lin_polish_lds[];
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (state[b] != LIN_POLISH_RUNNING) return;  // (uniform over the workgroup)
  const int n = u.n, m = u.m, N = u.N;
  const size_t oz = (size_t)b * d.N * d.rows, ov = (size_t)b * N * p;
  if (step >= 2) {
    if (!refine_accepted(norms, d.batch, b, step - 1)) {
      if (tid == 0) {
        state[b] = LIN_POLISH_STOPPED;
        atomicSub(running, 1);
      }
      return;
    }
    for (int k = wave; k < N; k += 4) {
      const size_t ok = oz + (size_t)k * d.rows;
      for (int i = lane; i < n; i += 64) {
        z[ok + i] = zc[ok + i];
        z[ok + d.n + i] = zc[ok + d.n + i];
      }
      if (k < N - 1)
        for (int j = lane; j < m; j += 64) z[ok + 2 * d.n + j] = zc[ok + 2 * d.n + j];
      for (int r = lane; r < p; r += 64) mu[ov + (size_t)k * p + r] = muc[ov + (size_t)k * p + r];
    }
    if (tid == 0) here[b] = step - 1;
  }
  if (!form) return;
  const double s = sig[b];
  const LinPolishKnotLds S(lin_polish_lds + (size_t)wave * lin_polish_wave_lds(n, m, p), n, m, p);
  const size_t recd = cost_record_doubles(n, m);
  double big = 0.0;
  for (int k = wave; k < N; k += 4) {
    const bool last = k == N - 1;
    const size_t kb = (size_t)b * N + k, ok = oz + (size_t)k * d.rows;
    cost_stage_record(rec + kb * recd, n, m, !last, S.sL, S.sLR, S.sG, lane);
    for (int idx = lane; idx < p * n; idx += 64) S.sC[idx] = C[kb * p * n + idx];
    if (!last)
      for (int idx = lane; idx < p * m; idx += 64) S.sD[idx] = D[kb * p * m + idx];
    for (int i = lane; i < n; i += 64) {
      S.sl[i] = delta[ok + i];
      S.sx[i] = delta[ok + d.n + i];
    }
    if (!last)
      for (int j = lane; j < m; j += 64) S.su[j] = delta[ok + 2 * d.n + j];
    wave_lds_sync();
    // delta lambda -> S.dl, delta x -> S.sx, delta u -> S.ux
    cost_knot_S<true>(n, m, last, S.sL, S.sLR, S.sG, S.sl, S.sx, S.su, S.dl, S.sx, S.ux, lane);
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) {
      const double zl = z[ok + i] + S.dl[i], zx = z[ok + d.n + i] + S.sx[i];
      zc[ok + i] = zl;
      zc[ok + d.n + i] = zx;
      big = max_nan(big, max_nan(fabs(zl), fabs(zx)));
    }
    if (!last)
      for (int j = lane; j < m; j += 64) {
        const double zu = z[ok + 2 * d.n + j] + S.ux[j];
        zc[ok + 2 * d.n + j] = zu;
        big = max_nan(big, fabs(zu));
      }
    for (int r = lane; r < p; r += 64) {
      const size_t e = ov + (size_t)k * p + r;
      double mn = 0.0;
      if (code[e] >= 2) {
        const double gd = lin_polish_row(S.sC + r, p, last ? nullptr : S.sD + r, p, S.sx, S.ux, n, m);
        const double t = gd - rc[e];
        if constexpr (STRICT) {
          const double t2 = s * t;
          mn = mu[e] + t2;
        } else {
          mn = fma(s, t, mu[e]);
        }
        big = max_nan(big, fabs(mn));
      }
      muc[e] = mn;
    }
    wave_lds_sync();  // (the next knot's staging overwrites what these lanes read)
  }
  red[tid] = big;
  __syncthreads();
  for (int t = 128; t > 0; t >>= 1) {
    if (tid < t) red[tid] = max_nan(red[tid], red[tid + t]);
    __syncthreads();
  }
  if (tid == 0 && !isfinite(red[0])) {
    state[b] = LIN_POLISH_NAN;
    atomicSub(running, 1);
  }
}

// w = C x + D u of row r of knot k of problem b from global memory, in the order of lin_polish_row
__device__ __forceinline__ double lin_polish_row_global(const Dims& u, const Dims& d, const int p, const int b, const int k,
                                                        const int r, const double* __restrict__ C, const double* __restrict__ D,
                                                        const double* __restrict__ z) {
  const size_t kb = (size_t)b * u.N + k, ok = ((size_t)b * d.N + k) * d.rows;
  return lin_polish_row(C + kb * p * u.n + r, p, k == u.N - 1 ? nullptr : D + kb * p * u.m + r, p, z + ok + d.n, z + ok + 2 * d.n,
                        u.n, u.m);
}

// End of a round, for every problem that is running or stopped: its steps counted, and its last accepted iterate
// validated with exact comparisons -- mu >= 0 where the code is 3 and lo < hi, mu <= 0 where it is 2, lo <= w <= hi on
// every code-1 row, w = C x + D u formed as lin_polish_row forms it. Valid: state 1 when the round accepted a step, 2 when
// it did not. Not valid and final != 0: state 2. Not valid otherwise: the set is corrected -- a wrong-signed row is
// released (code 1, mu = 0), a code-1 row outside its bounds is fixed at the violated bound (mu = 0) -- and the problem
// runs again (state 0): words[0] counts the running problems, words[1] those whose set changed.
//   grid (batch), block 256.
static __global__ __launch_bounds__(256) void lin_polish_validate(Dims u, Dims d, int p, int final,
                                                                  const double* __restrict__ C, const double* __restrict__ D,
                                                                  const double* __restrict__ lo, const double* __restrict__ hi,
                                                                  size_t bstride, unsigned char* __restrict__ code,
                                                                  const double* __restrict__ z, double* __restrict__ mu,
                                                                  int* __restrict__ state, int* __restrict__ steps,
                                                                  int* __restrict__ here, int* __restrict__ words) {
  __shared__ int bad_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int st = state[b];
  if (st != LIN_POLISH_RUNNING && st != LIN_POLISH_STOPPED) return;  // (uniform over the workgroup)
  const unsigned np = (unsigned)(u.N * p);
  const size_t ov = (size_t)b * np;
  const double* lb = lo + (size_t)b * bstride;
  const double* hb = hi + (size_t)b * bstride;
  if (tid == 0) bad_s = 0;
  __syncthreads();
  // 0: as it is, 1: released, 2: fixed at lo, 3: fixed at hi
  const auto verdict = [&](unsigned e) -> int {
    const unsigned char cd = code[ov + e];
    if (cd == 0) return 0;
    const double l = lb[e], h = hb[e], mv = mu[ov + e];
    if (cd == 3) return (l < h && mv < 0.0) ? 1 : 0;
    if (cd == 2) return mv > 0.0 ? 1 : 0;
    const double w = lin_polish_row_global(u, d, p, b, (int)(e / (unsigned)p), (int)(e % (unsigned)p), C, D, z);
    return w > h ? 3 : w < l ? 2 : 0;
  };
  int bad = 0;
  for (unsigned e = tid; e < np; e += blockDim.x) bad |= verdict(e);
  if (bad) atomicOr(&bad_s, 1);
  __syncthreads();
  const int invalid = bad_s;
  if (!invalid || final) {
    if (tid == 0) {
      const int took = here[b];
      steps[b] += took;
      here[b] = 0;
      state[b] = (!invalid && took >= 1) ? LIN_POLISH_DONE : LIN_POLISH_KEPT;
    }
    return;
  }
  for (unsigned e = tid; e < np; e += blockDim.x) {
    const int vd = verdict(e);
    if (vd == 0) continue;
    code[ov + e] = vd == 1 ? 1 : (unsigned char)vd;
    mu[ov + e] = 0.0;
  }
  if (tid == 0) {
    steps[b] += here[b];
    here[b] = 0;
    state[b] = LIN_POLISH_RUNNING;
    atomicAdd(words, 1);
    atomicAdd(words + 1, 1);
  }
}

// End of a polish: the resident solution zs gets the polished z of the problems in state 1 and the saved z0 of every other
// (the factorisations overwrote it); for state 1 also, on the bounded rows, v <- clip(w) and y <- mu / rho, so that a
// warm-started ADMM begins at the polished point. v, y of every other problem are not written.
//   grid (d.N, batch), block 64.
static __global__ void lin_polish_finish(Dims u, Dims d, int p, const double* __restrict__ rhov, const int* __restrict__ state,
                                         const unsigned char* __restrict__ code, const double* __restrict__ C,
                                         const double* __restrict__ D, const double* __restrict__ lo,
                                         const double* __restrict__ hi, size_t bstride, const double* __restrict__ z,
                                         const double* __restrict__ mu, const double* __restrict__ z0, double* __restrict__ zs,
                                         double* __restrict__ v, double* __restrict__ y) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t oz = ((size_t)b * d.N + k) * d.rows;
  if (state[b] != LIN_POLISH_DONE) {
    for (int r = threadIdx.x; r < d.rows; r += blockDim.x) zs[oz + r] = z0[oz + r];
    return;
  }
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) zs[oz + r] = z[oz + r];
  if (k >= u.N) return;
  const double rho = rhov[b];
  const size_t ov = ((size_t)b * u.N + k) * p, ob = (size_t)b * bstride + (size_t)k * p;
  for (int r = threadIdx.x; r < p; r += blockDim.x) {
    if (code[ov + r] == 0) continue;
    const double w = lin_polish_row_global(u, d, p, b, k, r, C, D, z);
    v[ov + r] = fmin(fmax(w, lo[ob + r]), hi[ob + r]);
    y[ov + r] = mu[ov + r] / rho;
  }
}

// Multipliers [batch][N][p]: the polished mu of the problems in state 1, rho y of the others.
//   grid ceil(N p / 256), batch; block 256.
static __global__ void lin_polish_multipliers(int per_problem, const double* __restrict__ rhov, const double* __restrict__ y,
                                              const int* __restrict__ state, const double* __restrict__ mu,
                                              double* __restrict__ out) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_problem) return;
  const size_t at = (size_t)b * per_problem + e;
  out[at] = state[b] == LIN_POLISH_DONE ? mu[at] : rhov[b] * y[at];
}

}  // namespace ndlqr
