// kernels_grad_dense.hpp -- internal: the parameter gradients of dense-cost and constrained batch solves
// (ndlqr_hip_gradients_dense).
//
// z and w are the solution and the adjoint solution in the CALLER's variables, packed [batch][nvars] as
// ndlqr_CopyBatchSolutions and ndlqr_CopyBatchAdjoint deliver them: per knot [lambda_k x_k u_k], no u at the last knot.
// With lam+ = lambda_(k+1) the nine gradients of a loss L(z), g = dL/dz, K w = g, are per knot
//     gA(i, j) = -(w_lam+[i] z_x[j] + z_lam+[i] w_x[j])        gB(i, j) = -(w_lam+[i] z_u[j] + z_lam+[i] w_u[j])
//     gH(i, j) = -(w_x[i] z_u[j] + z_x[i] w_u[j])
//     gQ(i, j) = -1/2 (w_x[i] z_x[j] + z_x[i] w_x[j])          gR(i, j) = -1/2 (w_u[i] z_u[j] + z_u[i] w_u[j])
//     gq = -w_x      gr = -w_u      gd = -w_lam+      gx0 = -w_lam0
// in the flat layout of ndlqr_InitializeBatchFlatDense (matrices column-major per knot: (i, j) at i + rows j), zero for
// A, B, H, R, r, d of the last knot. With w of the active-set system they are those of the constrained solve as well.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace ndlqr {

// workgroups the split of a batch sum aims at (ndlqr_hip_gradients_dense: problems per workgroup row), and the knots of a
// chunk at most
constexpr int kGradDenseWorkgroups = 2048;
constexpr int kGradDenseChunk = 8;

enum { GRADD_A = 0, GRADD_B, GRADD_Q, GRADD_H, GRADD_R, GRADD_q, GRADD_r, GRADD_d, GRADD_x0, GRADD_COUNT };

// Destinations of one assembly, as GradOut (kernels_grad.hpp): p[o] == nullptr: output o is not computed. Bit o of `sum`:
// output o is summed over the batch ([N][width], [n] for x0) -- into part (+ split x total + off[o]) when the batch is
// split over several workgroup rows, else straight into p[o].
struct GradDenseOut {
  double* p[GRADD_COUNT];
  unsigned sum;
  size_t off[GRADD_COUNT];  // offset of output o in a split's partial sums
  size_t total;             // doubles of partial sums per split
};

// doubles per knot of output o (x0: per problem)
__host__ __device__ inline int grad_dense_width(const int n, const int m, const int o) {
  switch (o) {
    case GRADD_A: case GRADD_Q: return n * n;
    case GRADD_B: case GRADD_H: return n * m;
    case GRADD_R: return m * m;
    case GRADD_r: return m;
    default: return n;
  }
}

// e = q w + r for 0 <= e < 2^24 and 0 < w: the quotient from one float multiplication (inv = 1.0f / w, at most one off),
// corrected by the remainder -- no integer division in the element loops
__device__ inline void grad_dense_divmod(const int e, const int w, const float inv, int& q, int& r) {
  q = (int)((float)e * inv);
  r = e - q * w;
  if (r < 0) { --q; r += w; }
  else if (r >= w) { ++q; r -= w; }
}

// Per-problem gradients and / or batch sums of knots [k0, k0 + KC) of problems [p0, p1): grid (ceil(N / KC), nsplit,
// nslice), block 256, dynamic LDS 2 (KC (2n+m) + n) doubles of z | w (the packed run of the chunk's knots and the lambda
// of the knot after it) and the accumulators of the summed outputs (KC x width each, n for x0 in the first chunk, one
// after the other in order of the outputs). Slices, splits and the order of summation are those of grad_assemble
// (kernels_grad.hpp): slice blockIdx.z holds accumulator entries [z EC, z EC + EC) of that sequence and slice 0 alone
// writes the per-problem outputs; each workgroup takes its problems in index order and every thread owns the same
// accumulator entries throughout, so the sums are deterministic. Outputs are written as contiguous runs of the flat
// layout: consecutive lanes, consecutive elements.
// skip (may be null): the status words of a constrained adjoint; a problem with skip[p] == 3 was not iterated -- exact
// zeros in its per-problem outputs, left out of the sums.
// STRICT: no contraction, every matrix entry as t1 = a b (the w factor first), t2 = c e, s = t1 + t2, out = -s (-0.5 s for
// Q, R): numpy reproduces them bit for bit. Otherwise A, B, H are -fma(a, b, c e); Q and R stay uncontracted in both
// modes, so that (i, j) and (j, i) carry the same bits (t1 and t2 change places, and the sum commutes).
template <bool STRICT>
__global__ __launch_bounds__(256) void grad_assemble_dense(const int n, const int m, const int N, const int batch,
                                                           const int KC, const int ppb, const int EC,
                                                           const double* __restrict__ z, const double* __restrict__ w,
                                                           const int* __restrict__ skip, GradDenseOut out,
                                                           double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int rows = 2 * n + m;
  const size_t nvars = (size_t)rows * N - m;
  const int k0 = blockIdx.x * KC;
  const int KU = KC < N - k0 ? KC : N - k0;  // knots of this chunk
  // the packed run of the chunk: its knots and the lambda behind them (the last chunk ends with the vector)
  const size_t run0 = (size_t)k0 * rows;
  const int nrun = (size_t)KU * rows + n < nvars - run0 ? KU * rows + n : (int)(nvars - run0);
  const int p0 = blockIdx.y * ppb, p1 = (p0 + ppb < batch) ? p0 + ppb : batch;
  double* zs = sm;
  double* ws = zs + KC * rows + n;
  double* acc = ws + KC * rows + n;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.z * EC, s1 = s0 + EC;  // this slice's accumulator entries: acc[j - s0] for j in [s0, s1)
  int aoff[GRADD_COUNT];
  {
    int a = 0;
    for (int o = 0; o < GRADD_COUNT; ++o) {
      aoff[o] = a;
      if (out.p[o] && (out.sum & (1u << o))) a += o == GRADD_x0 ? (k0 == 0 ? n : 0) : KU * grad_dense_width(n, m, o);
    }
    if (blockIdx.z > 0 && a <= s0) return;  // (a further slice with no entries in this chunk; uniform over the block)
    for (int e = tid; e < (a < s1 ? a : s1) - s0; e += blockDim.x) acc[e] = 0.0;  // (the first barrier below orders these)
  }
  const float inv_n = 1.0f / (float)n, inv_m = 1.0f / (float)m;
  for (int p = p0; p < p1; ++p) {
    const bool skipped = skip && skip[p] == 3;  // (uniform over the block)
    __syncthreads();  // the previous problem's run has been read
    if (!skipped) {
      const size_t base = (size_t)p * nvars + run0;
      for (int e = tid; e < nrun; e += blockDim.x) {
        zs[e] = z[base + e];
        ws[e] = w[base + e];
      }
    }
    __syncthreads();
    for (int o = 0; o < GRADD_COUNT; ++o) {
      double* dst = out.p[o];
      if (!dst) continue;
      const bool summed = (out.sum & (1u << o)) != 0;
      if (summed ? skipped : blockIdx.z > 0) continue;
      // output o: (i, j) of a matrix from the blocks at ra (rows, rd of them) and ca (columns) of a knot's run --
      // rows = 2n+m is the lambda of the next knot --, or entry i of the block at ra of w
      int ra, ca = -1, rd = 1;
      bool half = false, zero_last = true;
      switch (o) {
        case GRADD_A: ra = rows; ca = n; rd = n; break;
        case GRADD_B: ra = rows; ca = 2 * n; rd = n; break;
        case GRADD_Q: ra = n; ca = n; rd = n; half = true; zero_last = false; break;
        case GRADD_H: ra = n; ca = 2 * n; rd = n; break;
        case GRADD_R: ra = 2 * n; ca = 2 * n; rd = m; half = true; break;
        case GRADD_q: ra = n; zero_last = false; break;
        case GRADD_r: ra = 2 * n; break;
        case GRADD_d: ra = rows; break;
        default: ra = 0; zero_last = false; break;  // x0: lambda of knot 0
      }
      const int W = grad_dense_width(n, m, o);
      const float inv_W = 1.0f / (float)W, inv_rd = rd == n ? inv_n : inv_m;
      const int E = o == GRADD_x0 ? (k0 == 0 ? n : 0) : KU * W;
      const int e0 = summed && s0 > aoff[o] ? s0 - aoff[o] : 0, e1 = summed && s1 - aoff[o] < E ? s1 - aoff[o] : E;
      double* run = summed ? nullptr : dst + (o == GRADD_x0 ? (size_t)p * n : ((size_t)p * N + k0) * W);
      for (int e = e0 + tid; e < e1; e += blockDim.x) {
        double v = 0.0;
        if (!skipped) {
          int kk, rr;
          grad_dense_divmod(e, W, inv_W, kk, rr);
          const double* Z = zs + kk * rows;
          const double* Wv = ws + kk * rows;
          if (zero_last && k0 + kk == N - 1) {
            v = 0.0;
          } else if (ca < 0) {
            v = -Wv[ra + rr];
          } else {
            int i, j;
            grad_dense_divmod(rr, rd, inv_rd, j, i);
            const double a = Wv[ra + i], bb = Z[ca + j], c = Z[ra + i], ee = Wv[ca + j];
            if (STRICT || half) {
              const double t1 = a * bb;
              const double t2 = c * ee;
              const double s = t1 + t2;
              v = half ? -0.5 * s : -s;
            } else {
              v = -fma(a, bb, c * ee);
            }
          }
        }
        if (summed) acc[aoff[o] + e - s0] += v;
        else run[e] = v;
      }
    }
  }
  for (int o = 0; o < GRADD_COUNT; ++o) {
    if (!out.p[o] || !(out.sum & (1u << o))) continue;
    const int W = grad_dense_width(n, m, o);
    const int E = o == GRADD_x0 ? (k0 == 0 ? n : 0) : KU * W;
    const int e0 = s0 > aoff[o] ? s0 - aoff[o] : 0, e1 = s1 - aoff[o] < E ? s1 - aoff[o] : E;
    double* dst = part ? part + (size_t)blockIdx.y * out.total + out.off[o] : out.p[o];
    const size_t at = o == GRADD_x0 ? 0 : (size_t)k0 * W;
    for (int e = e0 + tid; e < e1; e += blockDim.x) dst[at + e] = acc[aoff[o] + e - s0];
  }
}

// Second stage of a split batch sum, as grad_sum_splits: entry t of the summed outputs = the sum over the splits in
// order (deterministic).
//   grid ceil(total / 256), block 256.
static __global__ __launch_bounds__(256) void grad_dense_sum_splits(GradDenseOut out, const int nsplit,
                                                                    const double* __restrict__ part) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= out.total) return;
  double s = 0.0;
  for (int j = 0; j < nsplit; ++j) s += part[(size_t)j * out.total + t];
  int o = GRADD_COUNT - 1;
  while (o > 0 && !(out.p[o] && (out.sum & (1u << o)) && t >= out.off[o])) --o;
  // (the summed outputs occupy [off[o], off[o] + size) in order of o; o found: the last summed one starting at or before t)
  out.p[o][t - out.off[o]] = s;
}

}  // namespace ndlqr
