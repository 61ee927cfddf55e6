// kernels_box_accel.hpp -- internal: safeguarded Anderson acceleration (type II) of the box-constrained batch solve
// (ndlqr_hip_set_box_acceleration).
//
// The ADMM of kernels_box.hpp is a fixed-point iteration in one vector per problem, w = v + y on the bounded entries
// (v = clip(w), y = w - v). With F(w) one iteration as it stands -- the re-solve with q~ from v, y, then
// t = alpha z + (1 - alpha) v + y -- t is the plain successor of w and g = t - (v + y) the residual. box_update_accel
// takes the place of box_update while the memory is not zero: it does what box_update does, keeps a ring of the last
// mem + 1 pairs (t, g) per problem, and where the rule allows replaces the plain successor by
//     w+ = t - dT gamma,   (dG'dG + reg tr(dG'dG) / c I) gamma = dG'g,
// dG, dT the c <= mem columns of differences of consecutive ring entries. The safeguard: an iteration that started from
// an accelerated iterate and finds |g| > safeguard |g_prev| goes back to the plain successor the step before saved.
//
// Per problem, in AccelBufs: the ring [mem + 1][N][n+m] of t and of g, entry i (0 = oldest) in slot (start + i) mod
// (mem + 1); the saved plain v+, y+ (pv, py); the Gram matrix dG'dG, 17 x 17, row and column of a column of dG being the
// ring slot of its later entry (a push adds one row and column, nothing moves); |g_prev|; gamma [mem] of the latest
// accelerated step, oldest column first; and six words, meta [6][batch]: start, fill, accelerated (the iterate the next
// iteration starts from is an accelerated one), accepted, rejected, columns of the latest accelerated step.
// Every entry of the ring, of v, y, pv, py is read and written by the same thread in every launch (entry e: thread
// e mod 256), so no pass waits for another thread's global stores.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box.hpp"

namespace ndlqr {

constexpr int ACCEL_MEM_MAX = 16;
constexpr int ACCEL_RING_MAX = ACCEL_MEM_MAX + 1;
enum { ACCEL_START = 0, ACCEL_FILL, ACCEL_FLAG, ACCEL_ACCEPTED, ACCEL_REJECTED, ACCEL_COLUMNS, ACCEL_WORDS };

struct AccelParams {
  int mem;  // 1 .. ACCEL_MEM_MAX
  double safeguard, reg;
};

struct AccelBufs {
  double *ring_t, *ring_g;  // [batch][mem + 1][N][n+m]
  double *pv, *py;          // [batch][N][n+m]
  double* gram;             // [batch][17][17]
  double* gprev;            // [batch]
  double* gamma;            // [batch][mem]
  int* meta;                // [ACCEL_WORDS][batch]
};

// c + a b: separate multiply and add (STRICT), or one fma
template <bool STRICT>
__device__ __forceinline__ double accel_mad(double a, double b, double c) {
  if constexpr (STRICT) {
    const double p = a * b;
    return c + p;
  } else {
    return fma(a, b, c);
  }
}

// sum over the wavefront in lane 0: a fixed tree, the same from run to run
__device__ __forceinline__ double accel_wave_sum(double x) {
  for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);
  return x;
}

// One ADMM update of every running problem: box_update's arguments and its calls of the shared core of kernels_box.hpp
// (box_step with the clip to [lo, hi], box_judge, box_adapt_penalty and the two tails), so everything is judged on the
// plain v+, y+ before anything else; then per problem that keeps running with its penalty:
//   - started from an accelerated iterate and |g| > safeguard |g_prev|: v, y <- pv, py, the next right-hand side from
//     them, the history cleared, a rejection counted; |g_prev| stays;
//   - otherwise (t, g) is pushed; with c >= 1 columns and plain_only == 0 thread 0 solves for gamma by Cholesky; a
//     pivot that is not positive, or a gamma or w+ that is not finite: the plain step, the history cleared; else
//     pv, py <- v+, y+, v = clip(w+), y = w+ - v, the right-hand side from them, an acceptance counted; |g_prev| = |g|.
// A problem whose penalty moves takes the plain v+, y+ (y rescaled) and clears its history: w changes scale with rho.
// plain_only (the iteration before an infeasibility check and the check iteration): the history is recorded, the step
// is the plain one. Sums: per thread in entry order, per wavefront by accel_wave_sum, the four wavefronts in order by
// thread 0 -- no floating-point atomics.
//   grid (batch), block 256.
template <bool STRICT>
__global__ __launch_bounds__(256) void box_update_accel(Dims d, int it, int adapt, int plain_only, BoxParams P, AccelParams A,
                                                        const double* __restrict__ z, const double* __restrict__ lo,
                                                        const double* __restrict__ hi, size_t bstride, double* __restrict__ v,
                                                        double* __restrict__ y, const double* __restrict__ res,
                                                        const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                        double* __restrict__ rhov, int* __restrict__ status,
                                                        int* __restrict__ iters, double* __restrict__ resid,
                                                        int* __restrict__ running, AccelBufs X) {
  constexpr int OLD = ACCEL_MEM_MAX - 1;  // columns of dG that a push can find in the ring
  __shared__ double red[5][256];
  __shared__ double sums[2 * OLD + 3][4];  // per wavefront: a[OLD] | b[OLD] | a_new | b_new | g'g
  __shared__ double chol[ACCEL_MEM_MAX][ACCEL_MEM_MAX + 1];
  __shared__ double gam_s[ACCEL_MEM_MAX];
  __shared__ double rho_s;  // the new penalty when mode_s == 2
  __shared__ int mode_s;    // 0: plain step, 1: frozen, 2: a new penalty, 3: rejected, 4: accelerated step
  const int b = blockIdx.x, tid = threadIdx.x, batch = gridDim.x;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const double rho = rhov[b];
  const BoxViews V(d, b, z, v, y, res, rhs_cur, rhs_next);
  const unsigned nw = V.nw;
  const BoxBounds bounded(lo, hi, bstride, b);
  // the ring as this iteration's push leaves it: a full ring drops its oldest entry, the new one takes slot snew
  const int R = A.mem + 1;
  const int fill = X.meta[ACCEL_FILL * batch + b];
  const int start0 = X.meta[ACCEL_START * batch + b];
  const int start = fill == R ? (start0 + 1 == R ? 0 : start0 + 1) : start0;
  const int fp = fill == R ? A.mem : fill;  // entries kept
  const int snew = (start + fp) % R;
  const int slast = (start + fp + R - 1) % R;  // newest entry kept (fp >= 1)
  double* Tr = X.ring_t + (size_t)b * R * nw;
  double* Gr = X.ring_g + (size_t)b * R * nw;
  double* pvb = X.pv + (size_t)b * nw;
  double* pyb = X.py + (size_t)b * nw;
  BoxMaxima M;
  double acc_a[OLD], acc_b[OLD], a_new = 0.0, b_new = 0.0, gg = 0.0;
#pragma unroll
  for (int k = 0; k < OLD; ++k) acc_a[k] = acc_b[k] = 0.0;
  for (unsigned e = tid; e < nw; e += blockDim.x) {
    const double l = bounded.lb[e], h = bounded.hb[e];
    if (!box_bounded(l, h)) continue;
    const size_t oz = box_entry_offset(d, e);
    const double zi = V.zb[oz], v0 = V.vb[e], y0 = V.yb[e];
    const BoxStep st = box_step<STRICT>(P, zi, v0, y0, true, l, h);
    V.vb[e] = st.vn;
    V.yb[e] = st.yn;
    V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], st.vn, st.yn, rho);
    M.note(zi, v0, st.vn, st.yn);
    // the residual of the fixed-point map, the push, and this entry's terms of the new row of dG'dG and of dG'g
    const double t = st.t, g = t - (v0 + y0);
    gg = accel_mad<STRICT>(g, g, gg);
    if (fp > 0) {
      int s = slast;
      double gh = Gr[(size_t)s * nw + e];
      const double dgn = g - gh;  // the new column
      a_new = accel_mad<STRICT>(dgn, dgn, a_new);
      b_new = accel_mad<STRICT>(dgn, g, b_new);
#pragma unroll
      for (int c = 0; c < OLD; ++c) {  // the columns kept, newest first
        if (c < fp - 1) {
          s = s == 0 ? R - 1 : s - 1;
          const double gl = Gr[(size_t)s * nw + e];
          const double dg = gh - gl;
          acc_a[c] = accel_mad<STRICT>(dg, dgn, acc_a[c]);
          acc_b[c] = accel_mad<STRICT>(dg, g, acc_b[c]);
          gh = gl;
        }
      }
    }
    Tr[(size_t)snew * nw + e] = t;
    Gr[(size_t)snew * nw + e] = g;
  }
  {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < OLD; ++c) {
      if (c < fp - 1) {
        const double sa = accel_wave_sum(acc_a[c]), sb = accel_wave_sum(acc_b[c]);
        if (lane == 0) { sums[c][wave] = sa; sums[OLD + c][wave] = sb; }
      }
    }
    const double sa = accel_wave_sum(a_new), sb = accel_wave_sum(b_new), sg = accel_wave_sum(gg);
    if (lane == 0) { sums[2 * OLD][wave] = sa; sums[2 * OLD + 1][wave] = sb; sums[2 * OLD + 2][wave] = sg; }
  }
  M.reduce(red, tid);
  if (tid == 0) {
    const BoxVerdict J = box_judge(P, rho, red, b, it, status, iters, resid, running);
    int mode = J.frozen ? 1 : adapt && box_adapt_penalty(P, rho, J, b, rhov, running, &rho_s) ? 2 : 0;
    int* meta = X.meta + b;  // word q at meta[q * batch]
    if (mode == 2) {
      meta[ACCEL_FILL * batch] = 0;
      meta[ACCEL_FLAG * batch] = 0;
    } else if (mode == 0) {
      const auto total = [&](int q) { return (sums[q][0] + sums[q][1]) + (sums[q][2] + sums[q][3]); };
      const double gnorm = sqrt(total(2 * OLD + 2));
      if (meta[ACCEL_FLAG * batch] && gnorm > A.safeguard * X.gprev[b]) {
        mode = 3;
        meta[ACCEL_FILL * batch] = 0;
        meta[ACCEL_FLAG * batch] = 0;
        meta[ACCEL_REJECTED * batch] += 1;
      } else {
        double* gram = X.gram + (size_t)b * ACCEL_RING_MAX * ACCEL_RING_MAX;
        const int c = fp;  // columns after the push; column i (0 = oldest) lives in the slot of entry i + 1
        const auto slot = [&](int i) { return (start + i + 1) % R; };
        if (c >= 1) {
          for (int i = 0; i < c - 1; ++i) {
            const double a = total(c - 2 - i);
            gram[snew * ACCEL_RING_MAX + slot(i)] = a;
            gram[slot(i) * ACCEL_RING_MAX + snew] = a;
          }
          gram[snew * ACCEL_RING_MAX + snew] = total(2 * OLD);
        }
        int keep = fp + 1;
        if (c >= 1 && !plain_only) {
          double tr = 0.0;
          for (int i = 0; i < c; ++i) tr = tr + gram[slot(i) * ACCEL_RING_MAX + slot(i)];
          const double shift = A.reg * tr / c;
          for (int i = 0; i < c; ++i)
            for (int j = 0; j <= i; ++j) chol[i][j] = gram[slot(i) * ACCEL_RING_MAX + slot(j)] + (i == j ? shift : 0.0);
          bool ok = true;
          for (int j = 0; j < c && ok; ++j) {  // in place: row by row of the lower triangle, column j
            double dj = chol[j][j];
            for (int k = 0; k < j; ++k) dj = dj - chol[j][k] * chol[j][k];
            if (!(dj > 0.0)) { ok = false; break; }
            dj = sqrt(dj);
            chol[j][j] = dj;
            for (int i = j + 1; i < c; ++i) {
              double s = chol[i][j];
              for (int k = 0; k < j; ++k) s = s - chol[i][k] * chol[j][k];
              chol[i][j] = s / dj;
            }
          }
          if (ok) {
            for (int i = 0; i < c; ++i) {
              double s = i < c - 1 ? total(OLD + c - 2 - i) : total(2 * OLD + 1);
              for (int k = 0; k < i; ++k) s = s - chol[i][k] * gam_s[k];
              gam_s[i] = s / chol[i][i];
            }
            for (int i = c - 1; i >= 0; --i) {
              double s = gam_s[i];
              for (int k = i + 1; k < c; ++k) s = s - chol[k][i] * gam_s[k];
              gam_s[i] = s / chol[i][i];
            }
            for (int i = 0; i < c; ++i) ok = ok && isfinite(gam_s[i]);
          }
          if (ok) mode = 4;
          else keep = 0;  // the plain step, the history cleared
        }
        meta[ACCEL_START * batch] = start;
        meta[ACCEL_FILL * batch] = keep;
        meta[ACCEL_FLAG * batch] = 0;
        X.gprev[b] = gnorm;
      }
    }
    mode_s = mode;
  }
  __syncthreads();
  const int mode = mode_s;
  if (mode == 0) return;
  if (mode == 4) {  // w+ = t - dT gamma: the plain v+, y+ saved, v, y and the next right-hand side from w+
    const int c = fp;
    int bad = 0;
    for (unsigned e = tid; e < nw; e += blockDim.x) {
      const double l = bounded.lb[e], h = bounded.hb[e];
      if (!box_bounded(l, h)) continue;
      const size_t oz = box_entry_offset(d, e);
      pvb[e] = V.vb[e];
      pyb[e] = V.yb[e];
      int s = start;
      double tl = Tr[(size_t)s * nw + e], corr = 0.0;
#pragma unroll
      for (int q = 0; q < ACCEL_MEM_MAX; ++q) {  // oldest column first; the last th is t itself
        if (q < c) {
          s = s + 1 == R ? 0 : s + 1;
          const double th = Tr[(size_t)s * nw + e];
          corr = accel_mad<STRICT>(gam_s[q], th - tl, corr);
          tl = th;
        }
      }
      const double wn = tl - corr;
      if (!isfinite(wn)) bad = 1;
      const double vn = fmin(fmax(wn, l), h);
      const double yn = wn - vn;
      V.vb[e] = vn;
      V.yb[e] = yn;
      V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], vn, yn, rho);
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
      int* meta = X.meta + b;
      if (bad) {
        meta[ACCEL_FILL * batch] = 0;
      } else {
        meta[ACCEL_FLAG * batch] = 1;
        meta[ACCEL_ACCEPTED * batch] += 1;
        meta[ACCEL_COLUMNS * batch] = c;
        for (int q = 0; q < A.mem; ++q) X.gamma[(size_t)b * A.mem + q] = q < c ? gam_s[q] : 0.0;
      }
    }
    if (!bad) return;
  }
  if (mode == 3 || mode == 4) {  // rejected (or w+ not finite): the saved plain v+, y+ again
    for (unsigned e = tid; e < nw; e += blockDim.x) {
      if (!bounded(e)) continue;
      const size_t oz = box_entry_offset(d, e);
      const double vs = pvb[e], ys = pyb[e];
      V.vb[e] = vs;
      V.yb[e] = ys;
      V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], vs, ys, rho);
    }
    return;
  }
  if (mode == 2) box_tail_new_penalty<STRICT>(d, V, rho, rho_s, tid, bounded);
  else box_tail_frozen(d, V, tid, bounded);
}

}  // namespace ndlqr
