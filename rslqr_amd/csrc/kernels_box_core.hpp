// kernels_box_core.hpp -- internal: the ADMM update core of the constrained solves (DESIGN.md sections 3.9, 3.17): the
// parameters, the step of one constrained entry, the running maxima of a problem, its judgement and the decision of the
// adaptive penalty (sections 3.11, 3.19). No __global__ kernel lives here; kernels_box.hpp and its companions
// (hip_box.hip) and kernels_lin.hpp (hip_lin.hip) include it.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace ndlqr {

struct BoxParams {
  double alpha, oma;  // oma = 1 - alpha
  double eps_abs, eps_rel;
  double rho_min, rho_max;  // clamp of the adaptive penalty (read only when box_update / lin_update adapts)
};

__device__ __forceinline__ bool box_bounded(double lo, double hi) { return lo > -HUGE_VAL || hi < HUGE_VAL; }
// max that keeps a NaN of either operand (fmax drops it): a NaN iterate must not look converged
__device__ __forceinline__ double max_nan(double m, double a) { return (a > m || a != a) ? a : m; }

// ---- The update core shared by box_update, box_update_accel (kernels_box_accel.hpp) and box_adjoint_update
// (kernels_box_grad.hpp). One workgroup of 256 threads per problem; entry e of [N][w] belongs to thread e mod 256 in every
// pass (e = tid; e += blockDim.x), so a thread re-reads only what it wrote itself and no pass waits for global stores.

// offset of entry e of [N][w] (x or u entry j of knot k, e = k w + j) in a problem's [N][rows] block
__device__ __forceinline__ size_t box_entry_offset(const Dims& d, unsigned e) {
  const unsigned k = e / (unsigned)d.w, j = e - k * (unsigned)d.w;
  return (size_t)k * d.rows + d.n + j;
}

// Problem b's part of the arrays every update kernel works on.
struct BoxViews {
  unsigned nw;  // entries of [N][w]
  const double *zb, *rs, *rc;
  double *vb, *yb, *rn;
  __device__ __forceinline__ BoxViews(const Dims& d, int b, const double* z, double* v, double* y, const double* res,
                                      const double* rhs_cur, double* rhs_next)
      : nw((unsigned)(d.N * d.w)), zb(z + (size_t)b * d.N * d.rows), rs(res + (size_t)b * d.N * d.rows),
        rc(rhs_cur + (size_t)b * d.N * d.rows), vb(v + (size_t)b * nw), yb(y + (size_t)b * nw),
        rn(rhs_next + (size_t)b * d.N * d.rows) {}
};

// Problem b's bounds in a forward kernel, and the predicate "entry e is bounded" its tails take.
struct BoxBounds {
  const double *lb, *hb;
  __device__ __forceinline__ BoxBounds(const double* lo, const double* hi, size_t bstride, int b)
      : lb(lo + (size_t)b * bstride), hb(hi + (size_t)b * bstride) {}
  __device__ __forceinline__ bool operator()(unsigned e) const { return box_bounded(lb[e], hb[e]); }
};

// The five running maxima of a problem over its bounded entries: |z - v+|, |v+ - v|, |z|, |v+|, |y+|. They keep a NaN.
struct BoxMaxima {
  double rp = 0.0, rd = 0.0, zm = 0.0, vm = 0.0, ym = 0.0;
  __device__ __forceinline__ void note(double zi, double v0, double vn, double yn) {
    rp = max_nan(rp, fabs(zi - vn));
    rd = max_nan(rd, fabs(vn - v0));
    zm = max_nan(zm, fabs(zi));
    vm = max_nan(vm, fabs(vn));
    ym = max_nan(ym, fabs(yn));
  }
  // over the workgroup into red[q][0], by a tree in LDS: deterministic. Ends in a barrier.
  __device__ __forceinline__ void reduce(double (&red)[5][256], int tid) const {
    red[0][tid] = rp; red[1][tid] = rd; red[2][tid] = zm; red[3][tid] = vm; red[4][tid] = ym;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s)
        for (int q = 0; q < 5; ++q) red[q][tid] = max_nan(red[q][tid], red[q][tid + s]);
      __syncthreads();
    }
  }
};

// zh = alpha z + (1 - alpha) v
template <bool STRICT>
__device__ __forceinline__ double box_relaxed(const BoxParams& P, double zi, double v0) {
  if constexpr (STRICT) {
    const double a = P.alpha * zi;
    const double c = P.oma * v0;
    return a + c;
  } else {
    return fma(P.alpha, zi, P.oma * v0);
  }
}

struct BoxStep {
  double t, vn, yn;  // zh + y, v+, y+
};

// The step of one bounded entry from its z, v, y: t = zh + y, v+ = clip ? min(max(t, lo), hi) : t, y+ = (y + zh) - v+.
// Arithmetic only. Each kernel loads z before v and y, stores v+, y+, writes the next right-hand side entry
// (box_rhs_entry) and lets the maxima take note, in that order.
template <bool STRICT>
__device__ __forceinline__ BoxStep box_step(const BoxParams& P, double zi, double v0, double y0, bool clip, double lo,
                                            double hi) {
  const double zh = box_relaxed<STRICT>(P, zi, v0);
  const double t = zh + y0;
  const double vn = clip ? fmin(fmax(t, lo), hi) : t;
  const double yn = (y0 + zh) - vn;
  return {t, vn, yn};
}

struct BoxVerdict {
  double r_prim, r_dual, sp, sd;
  bool frozen;
};

// Thread 0's judgement of problem b after re-solve `it` (1-based), from the reduced maxima: r_prim = max |z - v+|,
// r_dual = rho max |v+ - v|, sp = max(max |z|, max |v+|), sd = rho max |y+|; converged when
//     r_prim <= eps_abs + eps_rel sp   and   r_dual <= eps_abs + eps_rel sd.
// A converged problem is frozen as status 1; one whose maxima are not finite (a NaN or an infinity in z, v+ or y+, from
// the problem data or a failed pivot) as status 3. A frozen problem leaves the running count by an ordinary global
// atomic. iters[b] = it, and the four numbers go to resid[b] (the read-outs ndlqr_CopyBatchBoxResiduals and
// ndlqr_CopyBatchBoxAdjointResiduals) whether or not the problem goes on.
__device__ __forceinline__ BoxVerdict box_judge(const BoxParams& P, double rho, const double (&red)[5][256], int b, int it,
                                                int* status, int* iters, double* resid, int* running) {
  const double r_prim = red[0][0], r_dual = rho * red[1][0];
  const double sp = max_nan(red[2][0], red[3][0]), sd = rho * red[4][0];
  const double tol_p = P.eps_abs + P.eps_rel * sp;
  const double tol_d = P.eps_abs + P.eps_rel * sd;
  const bool finite = isfinite(r_prim) && isfinite(r_dual) && isfinite(red[2][0]) && isfinite(red[3][0]) &&
                      isfinite(red[4][0]);
  const int conv = finite && r_prim <= tol_p && r_dual <= tol_d;
  iters[b] = it;
  resid[4 * (size_t)b] = r_prim;
  resid[4 * (size_t)b + 1] = r_dual;
  resid[4 * (size_t)b + 2] = sp;
  resid[4 * (size_t)b + 3] = sd;
  if (conv || !finite) {
    status[b] = conv ? 1 : 3;
    atomicSub(running, 1);
  }
  return {r_prim, r_dual, sp, sd, conv || !finite};
}

// The adaptive penalty of a problem that goes on (DESIGN.md sections 3.11 and 3.19), decided by thread 0 of box_update,
// box_update_accel or lin_update from the verdict's four numbers when all of them are finite and > 0:
//     k = (ilogb(r_prim / sp) - ilogb(r_dual / sd)) / 2 (toward zero) clamped to [-6, 6],
//     rho+ = ldexp(rho, k) clamped to [rho_min, rho_max].
// Exact or correctly rounded operations only: numpy reproduces the decision bit for bit. True when rho+ != rho: then
// *rho_next = rho[b] = rho+ and running[1] counts the problem (the host refactors).
__device__ __forceinline__ bool box_adapt_penalty(const BoxParams& P, double rho, const BoxVerdict& J, int b, double* rhov,
                                                  int* running, double* rho_next) {
  if (!(isfinite(J.sd) && J.r_prim > 0.0 && J.r_dual > 0.0 && J.sp > 0.0 && J.sd > 0.0)) return false;
  int k = (ilogb(J.r_prim / J.sp) - ilogb(J.r_dual / J.sd)) / 2;
  k = k < -6 ? -6 : k > 6 ? 6 : k;
  if (k == 0) return false;
  const double rn = fmin(fmax(ldexp(rho, k), P.rho_min), P.rho_max);
  if (rn == rho) return false;
  *rho_next = rn;
  rhov[b] = rn;
  atomicAdd(running + 1, 1);
  return true;
}

}  // namespace ndlqr
