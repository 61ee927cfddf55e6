// kernels_reduced_solve.hpp -- what follows the factorisation of the runtime-sized separator-only schedule
// (kernels_reduced_mfma.hpp: the algebra, the records and the slots): the rhs-only re-solve on the kept records and
// the back-substitution. Runtime-sized, not instantiated per tile count: compiled once, by the unit that launches them.
#pragma once
#include "kernels_reduced_mfma.hpp"

namespace ndlqr {

// ------------------------------------------------------------------------------------- rhs-only re-solve
// New q, r, d, x0 against the factorisation a separator_reduced_mfma sweep left behind (the solver
// keeps it when NDLQR_FLAG_KEEP_RECORDS is set): per level, vector work only --
//     b~ = leafb - gL - gR,   y~ = L^-1 b~  -> record,   z_sep = L^-T y~,   gR[A] (+)= r_a' z_sep,   gL[B] (+)= r_bb' z_sep
// with L (packed, the inverses of its diagonal blocks in their place) from the separator's compact record, r_a = -CA,
// r_bb = -CB from the slots (level 0: from the problem data). The back-substitution then runs as after a full solve.
// Runtime-sized; np = padded block size of the factorisation.
//   grid (N >> (l+1), batch), block 256, dynamic LDS = 2 (n + m) + n + 3 np + 256 + n (n + 1) / 2 doubles.
static __global__ __launch_bounds__(256) void rhs_reduced_generic(Dims d, int l, int np, const double* __restrict__ AB,
                                                                  const double* __restrict__ QR,
                                                                  const double* __restrict__ rhs, double* red,
                                                                  double* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int nl = d.n, nnl = nl * nl, w = d.w, N = d.N, rows = d.rows;
  const int b = blockIdx.y;
  const int T = 2 << l, base = blockIdx.x * T, s = base + (1 << l) - 1;
  const bool hasA = base > 0, hasB = base + T < N, first = s == 0, level0 = l == 0;
  double* dq = sm;        // 1 / [Q_s | R_s] (state entries of knot 0: zero)
  double* zc = dq + w;    // rhs(s).xu scaled likewise (state entries of knot 0: -x0)
  double* q1 = zc + w;    // 1 / Q_{s+1}
  double* bz = q1 + nl;   // b~
  double* yv = bz + np;   // scratch of the block substitutions
  double* zs = yv + np;   // z_sep
  double* part = zs + np; // partial column sums: 256 / np segments of the summation index per column
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* ab = AB + ((size_t)b * N + s) * nl * w;
  const double* ab1 = ab + (size_t)nl * w;
  const double* qr = QR + ((size_t)b * N + s) * w;
  const double* r0 = rhs + ((size_t)b * N + s) * rows;
  const double* myslot = reduced_slot(red, d, b, level0 ? 1 : s);
  double* slotA = reduced_slot(red, d, b, hasA ? base - 1 : 1);
  double* slotB = reduced_slot(red, d, b, hasB ? base + T - 1 : 1);
  double* myrec = rec + ((size_t)b * N + s) * (2 * (size_t)nnl + nl);
  double* Lp = part + 256;  // the separator's factor from its compact record: packed lower triangle, staged
  auto P = [&](const int r, const int c) -> double { return Lp[r * (r + 1) / 2 + c]; };
  auto wave_sum = [](double v) -> double {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  };
  {  // the factor: every load in flight before the first LDS store
    const int WF = nl * (nl + 1) / 2;
    for (int e0 = 0; e0 < WF; e0 += 8 * 256) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int e = e0 + tid + 256 * u; t[u] = myrec[e < WF ? e : WF - 1]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int e = e0 + tid + 256 * u; if (e < WF) Lp[e] = t[u]; }
    }
  }

  for (int k = tid; k < w; k += 256) {
    const bool fx = first && k < nl;
    const double inv = 1.0 / qr[k];
    dq[k] = fx ? 0.0 : inv;
    zc[k] = fx ? -r0[k] : r0[nl + k] * inv;
  }
  for (int i = tid; i < nl; i += 256) q1[i] = 1.0 / qr[w + i];
  __syncthreads();
  // b~: a row per wavefront and round, lanes along the row
  for (int i = wave; i < np; i += 4) {
    double acc = 0.0;
    if (i < nl)
      for (int k = lane; k < w; k += 64) acc = fma(ab[(size_t)i * w + k], zc[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) {
      double v = 0.0;
      if (i < nl) {
        v = acc - fma(r0[rows + nl + i], q1[i], r0[rows + i]);
        if (!level0) v -= myslot[4 * nnl + i] + myslot[4 * nnl + nl + i];
      }
      bz[i] = v;
    }
  }
  __syncthreads();
  // y~ = L^-1 b~ -> record, and z_sep = L^-T y~ for the pushes (block substitutions, first wavefront)
  if (wave == 0) {
    const int nblk = (nl + 15) >> 4;
    for (int ib = 0; ib < nblk; ++ib) tri_forward_block(ib, nl, bz, yv, lane, P, P);
    for (int i = lane; i < np; i += 64) {
      if (i < nl) myrec[2 * nnl + i] = bz[i];
      zs[i] = i < nl ? bz[i] : 0.0;
    }
    wave_lds_order();
    for (int ib = nblk - 1; ib >= 0; --ib) tri_backward_block(ib, nl, zs, yv, lane, P, P);
  }
  __syncthreads();
  // column sums sum_k f(k, j): thread (j, seg) takes k = seg, seg + nseg, ..; consecutive threads read consecutive
  // words of a row of the operand
  const int nseg = 256 / np, cj = tid % np, cseg = tid / np;
  auto column_sums = [&](auto f, const int kend) -> double {  // returns the sum of column cj to the threads of segment 0
    double acc = 0.0;
    if (cseg < nseg)
      for (int k = cseg; k < kend; k += nseg) acc += f(k, cj);
    if (cseg < nseg) part[cseg * np + cj] = acc;
    __syncthreads();
    double tot = 0.0;
    if (cseg == 0)
      for (int g = 0; g < nseg; ++g) tot += part[g * np + cj];
    __syncthreads();
    return tot;
  };
  // gR[A] (+)= r_a' z_sep: a column of r_a per thread
  if (hasA) {  // (uniform)
    double* dst = slotA + 4 * nnl + nl;
    const double g = column_sums([&](const int k, const int j) {
      if (j >= nl) return 0.0;
      return (level0 ? -ab[(size_t)k * w + j] * dq[j] : -myslot[2 * nnl + k * nl + j]) * zs[k];
    }, nl);
    if (cseg == 0 && cj < nl) dst[cj] = level0 ? g : dst[cj] + g;
  }
  // gL[B] (+)= r_bb' z_sep; level 0: r_bb(k, j) = -A_{s+1}(j, k) / Q_{s+1}(k) -- a row of A_{s+1} per wavefront and round
  if (hasB) {
    double* dst = slotB + 4 * nnl;
    if (level0) {
      for (int j = wave; j < nl; j += 4) {
        double acc = 0.0;
        for (int k = lane; k < nl; k += 64) acc = fma(-q1[k] * ab1[(size_t)j * w + k], zs[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) dst[j] = acc;
      }
    } else {
      const double g = column_sums([&](const int k, const int j) {
        return j < nl ? -myslot[3 * nnl + k * nl + j] * zs[k] : 0.0;
      }, nl);
      if (cseg == 0 && cj < nl) dst[cj] += g;
    }
  }
}

// ------------------------------------------------------------------------------------- back-substitution, levels >= 1
// Multipliers of the separators of level l >= 1 from the compact records, top-down (one launch per level):
//     y_s = S-bar^-1 (b~ - r_a y_A - r_bb y_B) = L^-T (y~ + L^-1 (CA y_A + CB y_B))
// with CA = -r_a, CB = -r_bb where the factorisation read them (the separator's slot: nothing writes it after its
// elimination), L and y~ from the record; y_A, y_B are final (higher levels) in the lambda rows of knots A + 1, B + 1.
// One workgroup per separator: the rows of CA | CB are dealt to the wavefronts eight at a time (lanes along a row:
// coalesced, sixteen loads in flight per lane), the two block substitutions run on the first wavefront.
//   grid (N >> (l+1), batch), block 64 / 128 / 256 (by block size: a workgroup of four wavefronts per 16 x 16 separator left
//   three of them idle and the CU a quarter full), dynamic LDS = n (n + 1) / 2 + 2 n + 16 doubles. (A step that wants a knot range
//   alone runs the separators above it: Dims::xoff = the first one's index on the level, a shorter grid.)
static __global__ __launch_bounds__(256) void backsub_multipliers_compact(Dims d, int l, const double* __restrict__ red,
                                                                          const double* __restrict__ recs, double* z) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = d.n, nn = n * n, rows = d.rows, N = d.N, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, nwave = nthr >> 6;
  const int T = 2 << l, base = (blockIdx.x + d.xoff) * T, s = base + (1 << l) - 1;
  const bool hasA = base > 0, hasB = base + T < N;
  double* Lp = sm;                     // L / inverses of its diagonal blocks, packed lower triangle
  double* tv = Lp + n * (n + 1) / 2;   // CA y_A + CB y_B, then the substitutions
  double* yt = tv + n;                 // y~
  double* tmp = yt + n;                // scratch of the substitutions (16)
  const double* rc = recs + ((size_t)b * N + s) * (2 * (size_t)nn + n);
  const double* slot = red + ((size_t)b * (N >> 1) + (s >> 1)) * (4 * (size_t)nn + 2 * n);
  const double* CA = slot + 2 * (size_t)nn;
  const double* CB = slot + 3 * (size_t)nn;
  const double* yA = z + ((size_t)b * N + base) * rows;      // y_A lives in the lambda rows of knot A + 1 = base
  const double* yB = z + ((size_t)b * N + base + T) * rows;
  double* out = z + ((size_t)b * N + s + 1) * rows;
  {  // the factor: every load in flight before the first LDS store
    const int np = n * (n + 1) / 2;
    for (int e0 = 0; e0 < np; e0 += 8 * nthr) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int e = e0 + tid + nthr * u; t[u] = rc[e < np ? e : np - 1]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int e = e0 + tid + nthr * u; if (e < np) Lp[e] = t[u]; }
    }
    for (int i = tid; i < n; i += nthr) yt[i] = rc[2 * (size_t)nn + i];
  }
  for (int r0 = 8 * wave; r0 < n; r0 += 8 * nwave) {
    double part[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) part[u] = 0.0;
    for (int c = lane; c < n; c += 64) {
      double fa[8], fb[8], ya = 0.0, yb = 0.0;
      if (hasA) {  // uniform
        ya = yA[c];
#pragma unroll
        for (int u = 0; u < 8; ++u) fa[u] = CA[(size_t)(r0 + u < n ? r0 + u : n - 1) * n + c];
      }
      if (hasB) {
        yb = yB[c];
#pragma unroll
        for (int u = 0; u < 8; ++u) fb[u] = CB[(size_t)(r0 + u < n ? r0 + u : n - 1) * n + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (hasA) part[u] = fma(fa[u], ya, part[u]);
        if (hasB) part[u] = fma(fb[u], yb, part[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      double p = part[u];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
      if (lane == 0 && r0 + u < n) tv[r0 + u] = p;
    }
  }
  __syncthreads();
  if (wave == 0) {
    auto P = [&](const int i, const int k) -> double { return Lp[i * (i + 1) / 2 + k]; };
    const int nblk = (n + 15) >> 4;
    for (int ib = 0; ib < nblk; ++ib) tri_forward_block(ib, n, tv, tmp, lane, P, P);
    for (int i = lane; i < n; i += 64) tv[i] += yt[i];
    wave_lds_order();
    for (int ib = nblk - 1; ib >= 0; --ib) tri_backward_block(ib, n, tv, tmp, lane, P, P);
    for (int i = lane; i < n; i += 64) out[i] = tv[i];
  }
}

// ------------------------------------------------------------------------------------- back-substitution, level 0
// The last step of the back-substitution of the separator-only schedule above, one workgroup per level-0
// separator s = 2 j, i.e. per pair of knots (s, s + 1): its multiplier from the compact record
//     y_s = L^-T (y~ - L^-1 (r_a y_{s-1} + r_bb y_{s+1})),   r_a = -A_s Q_s^-1,  r_bb = -Q_{s+1}^-1 A_{s+1}'
// (the multipliers next to it are final: levels >= 1 ran before, backsub_multipliers_compact), then the states
// and inputs of both knots (the arithmetic of backsub_states_generic) -- [A | B] of the two knots comes from HBM
// once for both, and level 0's f_a | f_bb never exist in memory.
//   grid (N / 2, batch), block 64 / 128 / 256 (by block size), dynamic LDS = n (n + 1) / 2 + 5 n + 4 (n + m) +
//   2 (2 n + m) + block doubles.
static __global__ __launch_bounds__(256) void backsub_level0_states_generic(Dims d, const double* __restrict__ AB,
                                                                            const double* __restrict__ QR,
                                                                            const double* __restrict__ rhs,
                                                                            const double* __restrict__ rec,
                                                                            double* z) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = d.n, w = d.w, N = d.N, rows = d.rows, nn = n * n;
  const int b = blockIdx.y, s = 2 * (blockIdx.x + d.xoff);
  const bool hasA = s > 0, hasB = s + 2 < N;
  double* Wp = sm;                      // L (the inverses of its diagonal blocks in their place), packed lower triangle
  double* yA = Wp + n * (n + 1) / 2;    // y_{s-1}, then y_{s-1} / Q_s
  double* yB = yA + n;                  // y_{s+1}
  double* ys = yB + n;                  // y_s
  double* tv = ys + n;                  // r_a y_A + r_bb y_B, then the substitutions
  double* zs = tv + n;                  // y~ of the record
  double* d0 = zs + n;                  // [A_s | B_s]' y_s
  double* d1 = d0 + w;                  // [A_{s+1} | B_{s+1}]' y_{s+1}
  double* qv = d1 + w;                  // [Q | R] of knots s, s + 1
  double* rv = qv + 2 * w;              // raw right-hand sides of knots s, s + 1
  double* part = rv + 2 * rows;         // partial column sums (one per thread)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, nwave = nthr >> 6;
  const double* ab = AB + ((size_t)b * N + s) * n * w;
  const double* ab1 = ab + (size_t)n * w;
  const double* qr = QR + ((size_t)b * N + s) * w;
  const double* r0 = rhs + ((size_t)b * N + s) * rows;
  const double* myrec = rec + ((size_t)b * N + s) * (2 * (size_t)nn + n);
  double* zk = z + ((size_t)b * N + s) * rows;  // knot s; y_{s-1} lives in its lambda rows, y_s in those of knot s + 1
  auto wave_sum = [](double v) -> double {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  };
  // out[c] = sum_j m[j * w + c] y[j], c < w (a block transposed times a vector): thread (c, seg) sums the rows
  // j = seg, seg + nseg, .. -- consecutive threads read consecutive words of a row of the block
  // (m: first column of the range, nc columns, row pitch w)
  auto block_t_times = [&](const double* m, const int nc, const double* y, double* out) {
    const int nseg = 2 * nc <= nthr ? nthr / nc : 1;
    if (nseg > 1) {
      const int c = tid % nc, seg = tid / nc;
      double acc = 0.0;
      if (seg < nseg) {
        for (int j0 = seg; j0 < n; j0 += 8 * nseg) {  // eight loads in flight
          double mv[8], yv8[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int j = j0 + u * nseg, jc = j < n ? j : n - 1;
            mv[u] = m[(size_t)jc * w + c];
            yv8[u] = j < n ? y[jc] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = fma(mv[u], yv8[u], acc);
        }
        part[tid] = acc;
      }
      __syncthreads();
      if (seg == 0) {
        double tot = 0.0;
        for (int g = 0; g < nseg; ++g) tot += part[g * nc + c];
        out[c] = tot;
      }
      __syncthreads();
    } else {
      for (int c = tid; c < nc; c += nthr) {
        double acc = 0.0;
        for (int j = 0; j < n; ++j) acc = fma(m[(size_t)j * w + c], y[j], acc);
        out[c] = acc;
      }
      __syncthreads();
    }
  };

  // (requested first, consumed behind the pass over [A_{s+1} | B_{s+1}]: see the product with A_s below)
  const bool wide = n > 64;  // (uniform) more than 64 states: A_s does not fit the registers this way, it is read twice
  double areg[16];
  {
    const int jc = lane < n ? lane : n - 1;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = wave + u * nwave;
      areg[u] = wide ? 0.0 : ab[(size_t)(i < n ? i : n - 1) * w + jc];
    }
  }
  for (int e = tid; e < n * (n + 1) / 2; e += nthr) Wp[e] = myrec[e];
  for (int i = tid; i < n; i += nthr) {
    yA[i] = hasA ? zk[i] : 0.0;
    yB[i] = hasB ? zk[2 * rows + i] : 0.0;
    zs[i] = myrec[2 * nn + i];
  }
  for (int e = tid; e < 2 * w; e += nthr) qv[e] = qr[e];
  for (int e = tid; e < 2 * rows; e += nthr) rv[e] = r0[e];
  __syncthreads();
  block_t_times(ab1, w, yB, d1);  // [A_{s+1} | B_{s+1}]' y_{s+1}: enters t, x_{s+1} and u_{s+1}
  // t = r_a y_A + r_bb y_B = -A_s (y_A / Q_s) - (A_{s+1}' y_{s+1}) / Q_{s+1}. A_s stays in registers for the second
  // product with it further down (A_s' y_s), up to 64 states: wavefront wv holds the rows wv, wv + nwave, .. (at most
  // sixteen: n <= 64 with four wavefronts, <= 32 with two, <= 16 with one), lane = column -- every row is one coalesced request, all of
  // them in flight together, and the block comes from HBM once.
  if (!wide) {
    const double yq = (hasA && lane < n) ? yA[lane] / qv[lane] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = wave + u * nwave;
      const double a = wave_sum(areg[u] * yq);
      if (lane == 0 && i < n) tv[i] = -a - (hasB ? d1[i] / qv[w + i] : 0.0);
    }
  } else {
    for (int i0 = 4 * wave; i0 < n; i0 += 4 * nwave) {  // four rows of A_s per wavefront and round, lanes along the row
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      if (hasA) {
        for (int j = lane; j < n; j += 64) {
          const double yq = yA[j] / qv[j];
          double av[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) av[u] = ab[(size_t)(i0 + u < n ? i0 + u : n - 1) * w + j];
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = fma(av[u], yq, acc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double a = wave_sum(acc[u]);
        const int i = i0 + u;
        if (lane == 0 && i < n) tv[i] = -a - (hasB ? d1[i] / qv[w + i] : 0.0);
      }
    }
  }
  __syncthreads();
  // y_s = L^-T (y~ - L^-1 t): two block substitutions on the packed factor (first wavefront)
  if (wave == 0) {
    auto P = [&](const int i, const int k) -> double { return Wp[i * (i + 1) / 2 + k]; };
    const int nblk = (n + 15) >> 4;
    for (int ib = 0; ib < nblk; ++ib) tri_forward_block(ib, n, tv, part, lane, P, P);
    for (int i = lane; i < n; i += 64) tv[i] = zs[i] - tv[i];
    wave_lds_order();
    for (int ib = nblk - 1; ib >= 0; --ib) tri_backward_block(ib, n, tv, part, lane, P, P);
  }
  __syncthreads();
  if (tid < n) {
    const double yi = tv[tid];
    ys[tid] = yi;
    zk[rows + tid] = yi;  // lambda rows of knot s + 1
  }
  __syncthreads();
  // [A_s | B_s]' y_s: the state columns from the registers (partial sums per wavefront, then across them), the input
  // columns from memory (their first and only pass)
  if (!wide) {
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = wave + u * nwave;
      acc = fma(areg[u], i < n ? ys[i] : 0.0, acc);
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < n) {
      double tot = 0.0;
      for (int g = 0; g < nwave; ++g) tot += part[64 * g + tid];
      d0[tid] = tot;
    }
    __syncthreads();
    if (w > n) block_t_times(ab + n, w - n, ys, d0 + n);
  } else {
    block_t_times(ab, w, ys, d0);
  }
  // states and inputs of knots s and s + 1 (the arithmetic of backsub_states_generic); thread -> (knot, row)
  for (int e = tid; e < 2 * rows; e += nthr) {
    const int kk = e / rows, r = e - kk * rows, k = s + kk;
    if (r < n && k > 0) continue;  // lambda rows of knots >= 1 are the multipliers already
    const double* ykm = kk ? ys : yA;     // y_{k-1}
    const double* q = qv + kk * w;
    const double* rr = rv + kk * rows;
    const int col = r < n ? r : r - n;    // column of [A_k | B_k] this row meets
    double dot = 0.0;
    if (k < N - 1 && !(k == 0 && r >= n && r < 2 * n)) dot = (kk ? d1 : d0)[col];
    double out;
    if (r < n) out = fma(-q[r], rr[r], -rr[n + r]) + dot;                                 // knot 0: Q x0 + q + A_0' y_0
    else if (r < 2 * n) out = (k == 0) ? -rr[r - n] : (rr[r] - dot + ykm[r - n]) / q[r - n];  // x_k
    else out = (k == N - 1) ? rr[r] : (rr[r] - dot) / q[r - n];                            // u_k
    zk[(size_t)kk * rows + r] = out;
  }
}

}  // namespace ndlqr
