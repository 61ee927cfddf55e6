// kernels_grad.hpp -- internal: the adjoint right-hand side and the parameter gradients of the batch solver
// (ndlqr_hip_solve_adjoint, ndlqr_hip_gradients).
//
// The KKT matrix K is symmetric, so the adjoint system K w = g of a loss L(z) with g = dL/dz is one more right-hand-side
// re-solve against the kept factorisation. With z and w resident, the gradients of L with respect to the problem data are
// outer products of blocks of the two vectors (zero for A, B, R, r, d of the last knot, which the problem does not use):
//     gx0 = -w_lam0        gq_k = -w_xk        gr_k = -w_uk        gd_k = -w_lam(k+1)
//     gQ_k[i] = -w_xk[i] z_xk[i]                gR_k[i] = -w_uk[i] z_uk[i]
//     gA_k(i, j) = -(w_lam(k+1)[i] z_xk[j] + z_lam(k+1)[i] w_xk[j])
//     gB_k(i, j) = -(w_lam(k+1)[i] z_uk[j] + z_lam(k+1)[i] w_uk[j])
// in the flat layout of ndlqr_InitializeBatchFlat (A, B column-major: (i, j) at i + n j; Q, R diagonals).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace ndlqr {

// The adjoint right-hand side: g [batch][nvars] in the caller's block sizes (the packing of ndlqr_CopyBatchSolutions)
// into the device blocks [batch][N][2n+m]; the input slot of the last knot and the pad entries of a padded shape are zero.
// The last knot is the caller's, du.N - 1; the tail knots of a padded horizon (k >= du.N) are zero and g is not read there.
//   grid (d.N, batch), block 64.
static __global__ void adjoint_rhs_generic(Dims du, Dims d, const double* __restrict__ g, double* __restrict__ rhs) {
  const int k = blockIdx.x, b = blockIdx.y;
  const size_t nvars = (size_t)du.rows * du.N - du.m;
  const double* gk = g + (size_t)b * nvars + (size_t)k * du.rows;
  double* rk = rhs + ((size_t)b * d.N + k) * d.rows;
  const bool last = k == du.N - 1, tail = k >= du.N;
  for (int r = threadIdx.x; r < d.rows; r += blockDim.x) {
    int e = -1;
    if (tail) e = -1;
    else if (r < d.n) e = r < du.n ? r : -1;
    else if (r < 2 * d.n) e = r - d.n < du.n ? du.n + (r - d.n) : -1;
    else e = (r - 2 * d.n < du.m && !last) ? 2 * du.n + (r - 2 * d.n) : -1;
    rk[r] = e >= 0 ? gk[e] : 0.0;
  }
}

enum { GRAD_A = 0, GRAD_B, GRAD_Q, GRAD_R, GRAD_q, GRAD_r, GRAD_d, GRAD_x0, GRAD_COUNT };

// Destinations of one gradient assembly: p[o] == nullptr: output o is not computed. Bit o of `sum`: output o is summed
// over the batch ([N][width], [n] for x0) -- into part (+ split x total + off[o]) when the batch is split over several
// workgroup rows, else straight into p[o].
struct GradOut {
  double* p[GRAD_COUNT];
  unsigned sum;
  size_t off[GRAD_COUNT];  // offset of output o in a split's partial sums
  size_t total;            // doubles of partial sums per split
};

// doubles per knot of output o in the caller's block sizes (x0: per problem)
__host__ __device__ inline int grad_width(const Dims& du, const int o) {
  const int n = du.n, m = du.m;
  switch (o) {
    case GRAD_A: return n * n;
    case GRAD_B: return n * m;
    case GRAD_Q: case GRAD_q: case GRAD_d: case GRAD_x0: return n;
    default: return m;
  }
}

// Per-problem gradients and / or batch sums of knots [k0, k0 + KC) of problems [p0, p1): grid (N / KC, nsplit, nslice),
// block 256, dynamic LDS 2 (KC + 1) (2n+m) doubles of z | w (device blocks, + the lambda of the knot after the chunk) and
// the accumulators of the summed outputs (KC x width each, n for x0 in the first chunk, one after the other in order of
// the outputs). Slice blockIdx.z holds accumulator entries [z EC, z EC + EC) of that sequence (one slice, EC >= all of
// them, where they fit the LDS; else the entries of one knot are spread over several workgroups), and slice 0 alone
// writes the per-problem outputs. Each workgroup takes its problems in order and every thread owns the same accumulator
// entries throughout, so the sums are deterministic. Outputs are written as contiguous runs of the flat layout:
// consecutive lanes, consecutive elements.
// A padded horizon (du.N < d.N): the grid and the chunks are the device's (the same workgroups, splits and order of
// summation as a solver of horizon d.N), the outputs the caller's -- [batch][du.N][width], [du.N][width] summed: a chunk
// covers its knots below du.N only, the last knot is du.N - 1.
// STRICT: no contraction, gA / gB as t1 = a b, t2 = c e, s = t1 + t2, out = -s (numpy reproduces them bit for bit).
template <bool STRICT>
__global__ __launch_bounds__(256) void grad_assemble(Dims du, Dims d, const int KC, const int ppb, const int EC,
                                                     const double* __restrict__ z, const double* __restrict__ w,
                                                     GradOut out, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = du.n, N = d.N, rows = d.rows, xo = d.n, uo = 2 * d.n;
  const int k0 = blockIdx.x * KC, nk1 = (KC + 1 < N - k0) ? KC + 1 : N - k0;
  if (k0 >= du.N) return;  // (a chunk in the tail of a padded horizon; uniform over the block)
  const int KU = KC < du.N - k0 ? KC : du.N - k0;  // the caller's knots of this chunk
  const int p0 = blockIdx.y * ppb, p1 = (p0 + ppb < du.batch) ? p0 + ppb : du.batch;
  double* zs = sm;
  double* ws = zs + (KC + 1) * rows;
  double* acc = ws + (KC + 1) * rows;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.z * EC, s1 = s0 + EC;  // this slice's accumulator entries: acc[j - s0] for j in [s0, s1)
  int aoff[GRAD_COUNT];
  {
    int a = 0;
    for (int o = 0; o < GRAD_COUNT; ++o) {
      aoff[o] = a;
      if (out.p[o] && (out.sum & (1u << o))) a += o == GRAD_x0 ? (k0 == 0 ? n : 0) : KU * grad_width(du, o);
    }
    if (blockIdx.z > 0 && a <= s0) return;  // (a further slice with no entries in this chunk; uniform over the block)
    for (int e = tid; e < (a < s1 ? a : s1) - s0; e += blockDim.x) acc[e] = 0.0;  // (the first barrier below orders these)
  }
  for (int p = p0; p < p1; ++p) {
    __syncthreads();  // the previous problem's blocks have been read
    const size_t base = ((size_t)p * N + k0) * rows;
    for (int e = tid; e < nk1 * rows; e += blockDim.x) {
      zs[e] = z[base + e];
      ws[e] = w[base + e];
    }
    __syncthreads();
    for (int o = 0; o < GRAD_COUNT; ++o) {
      double* dst = out.p[o];
      if (!dst) continue;
      const bool summed = (out.sum & (1u << o)) != 0;
      if (!summed && blockIdx.z > 0) continue;
      const int W = grad_width(du, o);
      const int E = o == GRAD_x0 ? (k0 == 0 ? n : 0) : KU * W;
      const int e0 = summed && s0 > aoff[o] ? s0 - aoff[o] : 0, e1 = summed && s1 - aoff[o] < E ? s1 - aoff[o] : E;
      for (int e = e0 + tid; e < e1; e += blockDim.x) {
        const int kk = e / W, rr = e - kk * W, k = k0 + kk;
        const bool last = k == du.N - 1;
        const double* Z = zs + kk * rows;
        const double* Wv = ws + kk * rows;
        double v;
        switch (o) {
          case GRAD_A:
          case GRAD_B: {
            if (last) { v = 0.0; break; }
            const int i = rr % n, j = rr / n, col = (o == GRAD_A ? xo : uo) + j;
            const double a = Wv[rows + i], bb = Z[col], c = Z[rows + i], ee = Wv[col];
            if constexpr (STRICT) {
              const double t1 = a * bb;
              const double t2 = c * ee;
              const double s = t1 + t2;
              v = -s;
            } else {
              v = -fma(a, bb, c * ee);
            }
            break;
          }
          case GRAD_Q: v = -(Wv[xo + rr] * Z[xo + rr]); break;
          case GRAD_R: v = last ? 0.0 : -(Wv[uo + rr] * Z[uo + rr]); break;
          case GRAD_q: v = -Wv[xo + rr]; break;
          case GRAD_r: v = last ? 0.0 : -Wv[uo + rr]; break;
          case GRAD_d: v = last ? 0.0 : -Wv[rows + rr]; break;
          default: v = -Wv[rr]; break;  // x0: lambda of knot 0
        }
        if (summed) acc[aoff[o] + e - s0] += v;
        else dst[(o == GRAD_x0 ? (size_t)p * n : ((size_t)p * du.N + k0) * W) + e] = v;
      }
    }
  }
  for (int o = 0; o < GRAD_COUNT; ++o) {
    if (!out.p[o] || !(out.sum & (1u << o))) continue;
    const int W = grad_width(du, o);
    const int E = o == GRAD_x0 ? (k0 == 0 ? n : 0) : KU * W;
    const int e0 = s0 > aoff[o] ? s0 - aoff[o] : 0, e1 = s1 - aoff[o] < E ? s1 - aoff[o] : E;
    double* dst = part ? part + (size_t)blockIdx.y * out.total + out.off[o] : out.p[o];
    const size_t at = o == GRAD_x0 ? 0 : (size_t)k0 * W;
    for (int e = e0 + tid; e < e1; e += blockDim.x) dst[at + e] = acc[aoff[o] + e - s0];
  }
}

// Second stage of a split batch sum: entry t of the summed outputs = sum over the splits in order (deterministic).
//   grid ceil(total / 256), block 256.
static __global__ __launch_bounds__(256) void grad_sum_splits(GradOut out, const int nsplit, const double* __restrict__ part) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= out.total) return;
  double s = 0.0;
  for (int j = 0; j < nsplit; ++j) s += part[(size_t)j * out.total + t];
  int o = GRAD_COUNT - 1;
  while (o > 0 && !(out.p[o] && (out.sum & (1u << o)) && t >= out.off[o])) --o;
  // (the summed outputs occupy [off[o], off[o] + size) in order of o; o found: the last summed one starting at or before t)
  out.p[o][t - out.off[o]] = s;
}

}  // namespace ndlqr
