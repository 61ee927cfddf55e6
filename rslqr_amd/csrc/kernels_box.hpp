// kernels_box.hpp -- internal: the box-constrained batch solve by scaled ADMM on the kept factorisation
// (ndlqr_hip_set_bounds, ndlqr_hip_solve_box).
//
// The ADMM variables v (projected copy) and y (scaled dual) are shaped like the [x | u] part of every knot, in the device
// layout [batch][N][n+m] of QR; so are the bounds lo, hi ([N][n+m] once when they are shared by every problem). An entry
// is bounded (mask M = 1) when one of its bounds is finite; x of knot 0, u of the last knot and the pad entries of a
// padded shape are never bounded. The penalty is per problem, rho[batch] (a fixed-penalty solve fills it with one value;
// box_update may move it by powers of two: DESIGN.md section 3.11). With rho and alpha fixed, one iteration is a re-solve
// with the right-hand side
//     q~ = q + rho M (y - v)     (r~ likewise; x0 and d as resident)
// against the factorisation of Q~ = Q + rho M_x, R~ = R + rho M_u, followed by box_update:
//     zh = alpha z + (1 - alpha) v,   v+ = clip(zh + y, lo, hi),   y+ = (y + zh) - v+
// STRICT: separate mul and add in exactly that order, 1 - alpha computed once on the host, q~ as t = y - v, t = rho t,
// s = q + t, rhs = -s: numpy reproduces every value bit for bit. Unbounded entries are never touched by the update: their
// right-hand side is the resident one (written once per solve), y stays 0, and v = z is filled in by box_finish.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_box_core.hpp"
#include "kernels_common.hpp"

namespace ndlqr {

// Bounds in the caller's layout -- xlo, xhi [P][N][n], ulo, uhi [P][N][m], P = batch or 1 (shared); nullptr: unbounded --
// into the device layout lo, hi [P][N][n+m]. commit == 0: only check, *bad = 1 when lo > hi (or NaN) for an entry that is
// used. commit == 1: write lo, hi, and the bounded pattern into mask, *changed = 1 where it differs from what mask held.
// The caller's arrays have du.N knots, the device's d.N: the tail knots of a padded horizon (k >= du.N) and u of the
// caller's last knot du.N - 1 are unbounded whatever the bounds say, and the caller's arrays are not read there.
//   grid (d.N, P), block 64.
static __global__ void box_bounds(Dims du, Dims d, const double* __restrict__ xlo, const double* __restrict__ xhi,
                                  const double* __restrict__ ulo, const double* __restrict__ uhi, int commit,
                                  double* __restrict__ lo, double* __restrict__ hi, unsigned char* __restrict__ mask,
                                  int* __restrict__ bad, int* __restrict__ changed) {
  const int k = blockIdx.x, p = blockIdx.y;
  const size_t xo = ((size_t)p * du.N + k) * du.n, uo = ((size_t)p * du.N + k) * du.m;
  const size_t o = ((size_t)p * d.N + k) * d.w;
  for (int j = threadIdx.x; j < d.w; j += blockDim.x) {
    double l = -HUGE_VAL, h = HUGE_VAL;
    if (j < d.n) {
      if (j < du.n && k > 0 && k < du.N) {
        if (xlo) l = xlo[xo + j];
        if (xhi) h = xhi[xo + j];
      }
    } else {
      const int i = j - d.n;
      if (i < du.m && k < du.N - 1) {
        if (ulo) l = ulo[uo + i];
        if (uhi) h = uhi[uo + i];
      }
    }
    if (!commit) {
      if (!(l <= h)) *bad = 1;
      continue;
    }
    lo[o + j] = l;
    hi[o + j] = h;
    const unsigned char b = box_bounded(l, h) ? 1 : 0;
    if (mask[o + j] != b) {
      mask[o + j] = b;
      *changed = 1;
    }
  }
}

// rho[b] = value for every problem.
//   grid ceil(batch / 256), block 256.
static __global__ void box_fill_rho(int batch, double value, double* __restrict__ rho) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) rho[b] = value;
}

// QR <- QR + rho[b] M in place (the caller has saved QR). lo, hi of problem b at offset b * bstride.
//   grid (N, batch), block 64.
static __global__ void box_shift_qr(Dims d, const double* __restrict__ rhov, const double* __restrict__ lo,
                                    const double* __restrict__ hi, size_t bstride, double* __restrict__ QR) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double rho = rhov[b];
  const size_t ob = (size_t)b * bstride + (size_t)k * d.w, oq = ((size_t)b * d.N + k) * d.w;
  for (int j = threadIdx.x; j < d.w; j += blockDim.x)
    if (box_bounded(lo[ob + j], hi[ob + j])) QR[oq + j] = QR[oq + j] + rho;
}

// q~ of one bounded entry from the resident right-hand side entry res = -q
template <bool STRICT>
__device__ __forceinline__ double box_rhs_entry(double res, double v, double y, double rho) {
  const double q = -res;
  double t = y - v;
  if constexpr (STRICT) {
    t = rho * t;
    return -(q + t);
  } else {
    return -fma(rho, t, q);
  }
}

// Start of a solve: both ADMM right-hand sides from the resident one and v, y (zeroed first for a cold start; a warm
// start zeroes y of the entries the current bounds leave unbounded, which may have been bounded in the previous solve).
// prev_status (a warm start: the status words of the previous solve, which this launch precedes): a problem that ended
// as 4 -- certified infeasible, its y has diverged -- starts cold.
//   grid (N, batch), block 64.
template <bool STRICT>
__global__ void box_start(Dims d, const double* __restrict__ rhov, int cold_all, const int* __restrict__ prev_status,
                          const double* __restrict__ lo, const double* __restrict__ hi, size_t bstride,
                          const double* __restrict__ res, double* __restrict__ v, double* __restrict__ y,
                          double* __restrict__ rhs0, double* __restrict__ rhs1) {
  const int k = blockIdx.x, b = blockIdx.y;
  const bool cold = cold_all || prev_status[b] == 4;
  const double rho = rhov[b];
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w,
               ob = (size_t)b * bstride + (size_t)k * d.w;
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    double val = res[oz + r];
    if (r >= d.n) {
      const int j = r - d.n;
      const bool bounded = box_bounded(lo[ob + j], hi[ob + j]);
      if (cold) { v[ov + j] = 0.0; y[ov + j] = 0.0; }
      else if (!bounded) y[ov + j] = 0.0;
      if (bounded) val = box_rhs_entry<STRICT>(val, cold ? 0.0 : v[ov + j], cold ? 0.0 : y[ov + j], rho);
    }
    rhs0[oz + r] = val;
    rhs1[oz + r] = val;
  }
}

// ---- The update core shared by box_update, box_update_accel (kernels_box_accel.hpp), box_adjoint_update
// (kernels_box_grad.hpp) and lin_update (kernels_lin.hpp): kernels_box_core.hpp, box_adapt_penalty included. What follows
// here are the tails of the box kernels.

// Tail of a problem whose penalty moved from rho to rho_new: y <- y (rho / rho_new) on the entries that count (mu = rho y
// is kept) and the next right-hand side rewritten from rho_new and that y. Reads the v+, y+ this thread stored.
template <bool STRICT, class Counts>
__device__ __forceinline__ void box_tail_new_penalty(const Dims& d, const BoxViews& V, double rho, double rho_new, int tid,
                                                     Counts counts) {
  const double s = rho / rho_new;
  for (unsigned e = tid; e < V.nw; e += blockDim.x) {
    if (!counts(e)) continue;
    const size_t oz = box_entry_offset(d, e);
    const double ys = V.yb[e] * s;
    V.yb[e] = ys;
    V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], V.vb[e], ys, rho_new);
  }
}

// Tail of a frozen problem: the next right-hand side is the current one, so later re-solves reproduce its z.
template <class Counts>
__device__ __forceinline__ void box_tail_frozen(const Dims& d, const BoxViews& V, int tid, Counts counts) {
  for (unsigned e = tid; e < V.nw; e += blockDim.x) {
    if (!counts(e)) continue;
    const size_t oz = box_entry_offset(d, e);
    V.rn[oz] = V.rc[oz];
  }
}

// One ADMM update of every running problem (status[b] == 0) after re-solve `it`: z [batch][N][2n+m] is the re-solve's
// solution with the right-hand side rhs_cur; v, y are updated in place over the bounded entries (box_step with the clip
// to [lo, hi]), the next right-hand side -- from the resident one, res -- goes to rhs_next; then box_judge. adapt != 0: a
// problem that goes on may move its penalty (box_adapt_penalty, box_tail_new_penalty). A frozen problem never does.
//   grid (batch), block 256.
template <bool STRICT>
__global__ __launch_bounds__(256) void box_update(Dims d, int it, int adapt, BoxParams P, const double* __restrict__ z,
                                                  const double* __restrict__ lo, const double* __restrict__ hi, size_t bstride,
                                                  double* __restrict__ v, double* __restrict__ y, const double* __restrict__ res,
                                                  const double* __restrict__ rhs_cur, double* __restrict__ rhs_next,
                                                  double* __restrict__ rhov, int* __restrict__ status,
                                                  int* __restrict__ iters, double* __restrict__ resid,
                                                  int* __restrict__ running) {
  __shared__ double red[5][256];
  __shared__ double rho_s;  // the new penalty when conv_s == 2
  __shared__ int conv_s;    // 0: goes on, 1: frozen, 2: goes on with a new penalty
  const int b = blockIdx.x, tid = threadIdx.x;
  if (status[b] != 0) return;  // frozen (uniform over the workgroup)
  const double rho = rhov[b];
  const BoxViews V(d, b, z, v, y, res, rhs_cur, rhs_next);
  const BoxBounds bounded(lo, hi, bstride, b);
  BoxMaxima M;
  for (unsigned e = tid; e < V.nw; e += blockDim.x) {
    const double l = bounded.lb[e], h = bounded.hb[e];
    if (!box_bounded(l, h)) continue;
    const size_t oz = box_entry_offset(d, e);
    const double zi = V.zb[oz], v0 = V.vb[e], y0 = V.yb[e];
    const BoxStep s = box_step<STRICT>(P, zi, v0, y0, true, l, h);
    V.vb[e] = s.vn;
    V.yb[e] = s.yn;
    V.rn[oz] = box_rhs_entry<STRICT>(V.rs[oz], s.vn, s.yn, rho);
    M.note(zi, v0, s.vn, s.yn);
  }
  M.reduce(red, tid);
  if (tid == 0) {
    const BoxVerdict J = box_judge(P, rho, red, b, it, status, iters, resid, running);
    conv_s = J.frozen ? 1 : adapt && box_adapt_penalty(P, rho, J, b, rhov, running, &rho_s) ? 2 : 0;
  }
  __syncthreads();
  if (conv_s == 2) box_tail_new_penalty<STRICT>(d, V, rho, rho_s, tid, bounded);
  else if (conv_s == 1) box_tail_frozen(d, V, tid, bounded);
}

// End of a solve: the resident solution blocks zs get lambda from the last re-solve z and x, u from v (bounded entries)
// or z (unbounded ones, where v = z is stored too).
//   grid (N, batch), block 64.
static __global__ void box_finish(Dims d, const double* __restrict__ lo, const double* __restrict__ hi, size_t bstride,
                                  const double* __restrict__ z, double* __restrict__ v, double* __restrict__ zs) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t oz = ((size_t)b * d.N + k) * d.rows, ov = ((size_t)b * d.N + k) * d.w,
               ob = (size_t)b * bstride + (size_t)k * d.w;
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    double val = z[oz + r];
    if (r >= d.n) {
      const int j = r - d.n;
      if (box_bounded(lo[ob + j], hi[ob + j])) val = v[ov + j];
      else v[ov + j] = val;
    }
    zs[oz + r] = val;
  }
}

// Multipliers mu = rho[b] y into the caller's flat layout: mu_x [batch][N][n], mu_u [batch][N][m] (either may be nullptr).
//   grid (du.N, batch), block 64.
static __global__ void box_multipliers(Dims du, Dims d, const double* __restrict__ rhov, const double* __restrict__ y,
                                       double* __restrict__ mu_x, double* __restrict__ mu_u) {
  const int k = blockIdx.x, b = blockIdx.y;
  const double rho = rhov[b];
  const size_t ov = ((size_t)b * d.N + k) * d.w;
  for (int j = threadIdx.x; j < du.n + du.m; j += blockDim.x) {
    if (j < du.n) {
      if (mu_x) mu_x[((size_t)b * du.N + k) * du.n + j] = rho * y[ov + j];
    } else if (mu_u) {
      const int i = j - du.n;
      mu_u[((size_t)b * du.N + k) * du.m + i] = rho * y[ov + d.n + i];
    }
  }
}

}  // namespace ndlqr
