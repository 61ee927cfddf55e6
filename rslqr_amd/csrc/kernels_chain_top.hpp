// kernels_chain_top.hpp -- the top of the separator-only schedule as ONE BLOCK-TRIDIAGONAL CHAIN per problem.
//
// Once the tree levels below l0 are eliminated, the separators of level >= l0 of a problem form a block-tridiagonal SPD
// system: block j = separator (j + 1) 2^l0 - 1, C = 2^(K - l0) - 1 blocks of n x n,
//     D_j y_j + E_{j-1}' y_{j-1} + E_j y_{j+1} = b_j,
//     D_j = leaf tile - DL - DR,   b_j = leaf rhs - gL - gR        (what reduced_separator_mc assembles from the slot)
//     E_j = r_bb(j) = -CB_j  (j even: a separator of level l0, whose children wrote both couplings of its slot)
//     E_j = r_a(j + 1)' = -CA_{j+1}'  (j odd: the slot of a higher separator has no couplings yet -- the tree would write
//           them level by level; its coupling to a neighbour is the transpose of that neighbour's panel).
// The tree eliminates it by cyclic reduction: a two-sided panel of 2n + 1 columns per separator, fill-in between the
// neighbours, K - l0 dependent launches or workgroup barriers. Plain block Cholesky along the chain has a one-sided panel
// of n + 1 columns -- [E_j | b_j] --, no fill-in, and a fifth of the arithmetic per block:
//     L_j L_j' = D_j,  [Y_j | v_j] = L_j^-1 [E_j | b_j],  D_{j+1} -= Y_j'Y_j,  b_{j+1} -= Y_j'v_j      (forward)
//     y_j = L_j^-T (v_j - Y_j y_{j+1})                                                               (backward)
// n + 1 <= 16 columns are one 16-lane DPP row (kernels_rowbcast.hpp: lane i holds row i of D_j and column i of the panel,
// every product is a v_fmac_f64_dpp with row_newbcast), so a wavefront carries FOUR problems, one per row, and no
// instruction crosses rows: a member never sees its neighbours' data. The chain is serial; the batch is the parallelism.
// It is eaten from both ends: wavefront 0 of the workgroup eliminates blocks 0, 1, .. mid - 1, wavefront 1 blocks
// C - 1, C - 2, .. mid + 1 (towards lower indices: panel [E_{j-1}' | b_j]); wavefront 1 hands its update of the middle
// block over through LDS, wavefront 0 solves it and hands y_mid back, both sweep outwards.
//   reduced_chain_top   grid (ceil(batch / 4)), block 128, dynamic LDS 4 (N / 8) n doubles (the sweep arrays); K - l0 <= 5
// Scratch: L_j, Y_j, v_j stay in the record slot of the block's separator (2 n^2 + n doubles: Y row-major | L row-major |
// v) -- the schedules that run this keep no records of level >= l0. Levels 3 .. l0 - 1 (horizons beyond 256 knots)
// keep reduced_level_mc and their records; the top-down sweep over those runs behind the chain (backsub_top_body).
#pragma once
#include "kernels_bottom_reduced.hpp"
#include "kernels_rowbcast.hpp"

namespace ndlqr {

// the panel is one DPP row: n coupling columns and the right-hand side. The leaf tile is rb_leaf's where [A | B] has at most
// 16 columns (one per lane); wider ones take it as two products, A Q^-1 A' and B R^-1 B' (kChainTopSplit)
template <int NX, int NU>
constexpr bool kChainTopFits = NX + 1 <= 16 && NU <= 16;
template <int NX, int NU>
constexpr bool kChainTopSplit = NX + NU > 16;

constexpr int kChainTopThreads = 128;
constexpr int kChainTopMaxLevels = 5;  // at most 31 blocks per chain

// what the workgroup keeps in LDS next to the sweep arrays
template <int NX>
struct alignas(16) ChainTopLds {
  double hand[4][NX + 1][16];  // wavefront 1's update of the middle block: [row][column | rhs][lane]
  double lmid[4][NX][NX + 1];  // L of the middle block (read back by columns)
  double ymid[4][16];          // y of the middle block
};

// Operands of one chain block as they come from memory (nothing is computed on them before the pass of the block in
// front has been issued: the loads have that pass to arrive).
template <int NX, int NU>
struct ChainOps {
  double abrow[NX + NU];  // row i of [A_s | B_s]
  double tcol[NX];        // column i of [A_s | B_s] (split leaf tile: of A_s)
  double tcolb[kChainTopSplit<NX, NU> ? NX : 1];  // split leaf tile: column i of B_s, its weight R_s(i) and cost entry
  double qkb, zkb;
  double dl[NX], dr[NX];  // row i of DL, DR
  double cpl[NX];         // column i of the coupling block towards the middle
  double qk, zk;          // [Q_s | R_s](i), cost row of rhs(s)
  double q1, z1l, z1x;    // Q_{s+1}(i), rhs(s+1).lambda / .x
  double gl, gr;
};

// dir: +1 the panel couples block j to j + 1, -1 to j - 1, 0 none (the middle block)
template <int NX, int NU>
__device__ __forceinline__ void chain_load(const Dims& d, const int l0, const int b, const int j, const int dir, const int ic,
                                           const int kc, const double* __restrict__ AB, const double* __restrict__ QR,
                                           const double* __restrict__ rhs, const double* red, ChainOps<NX, NU>& o) {
  constexpr int W = NX + NU, ROWS = 2 * NX + NU, NN = NX * NX, TRI = RedSlot<NX>::TRI, SLOT = RedSlot<NX>::SIZE;
  const int N = d.N, s = ((j + 1) << l0) - 1;
  const size_t kn = (size_t)b * N + s;
  const double* abm = AB + kn * NX * W;
#pragma unroll
  for (int k = 0; k < W; ++k) o.abrow[k] = abm[ic * W + k];
#pragma unroll
  for (int c = 0; c < NX; ++c) o.tcol[c] = abm[c * W + kc];
  o.qk = QR[kn * W + kc];
  o.zk = rhs[kn * ROWS + NX + kc];
  if constexpr (kChainTopSplit<NX, NU>) {
    const int kb = NX + (kc < NU ? kc : NU - 1);
#pragma unroll
    for (int c = 0; c < NX; ++c) o.tcolb[c] = abm[c * W + kb];
    o.qkb = QR[kn * W + kb];
    o.zkb = rhs[kn * ROWS + NX + kb];
  }
  o.q1 = QR[(kn + 1) * W + ic];
  o.z1l = rhs[(kn + 1) * ROWS + ic];
  o.z1x = rhs[(kn + 1) * ROWS + NX + ic];
  const double* sl = red + ((size_t)b * (N >> 2) + (s >> 2)) * SLOT;
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    const int tix = RedSlot<NX>::tri(ic, c);
    o.dl[c] = sl[tix];
    o.dr[c] = sl[TRI + tix];
  }
  o.gl = sl[2 * TRI + 2 * NN + ic];
  o.gr = sl[2 * TRI + 2 * NN + NX + ic];
  if (dir != 0) {
    // an even block reads its own panel (column ic of CB / CA), an odd one the transpose of its neighbour's (row ic of the
    // neighbour's CA / CB)
    const bool own = (j & 1) == 0;
    const int sn = own ? s : s + dir * (1 << l0);
    const double* cs = red + ((size_t)b * (N >> 2) + (sn >> 2)) * SLOT + 2 * TRI + (((dir > 0) == own) ? NN : 0);
    const double* cp = cs + (own ? ic : ic * NX);
    const int sk = own ? NX : 1;
#pragma unroll
    for (int k = 0; k < NX; ++k) o.cpl[k] = cp[k * sk];
  } else {
#pragma unroll
    for (int k = 0; k < NX; ++k) o.cpl[k] = 0.0;
  }
}

// [D_j | b_j] from the operands and what the block in front left (U, ub: the negated products, added)
template <int NX, int NU>
__device__ __forceinline__ void chain_assemble(const int i, ChainOps<NX, NU>& o, const double (&U)[NX], const double ub,
                                               double (&S)[NX], double& bz) {
  constexpr int W = NX + NU;
  const double wk = rb_rcp(o.qk);
  double T[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) T[c] = o.tcol[c] * wk;
  if constexpr (kChainTopSplit<NX, NU>) {
    const double wb = rb_rcp(o.qkb), q1 = rb_rcp(o.q1);
    double Tb[NX], brow[NU];
#pragma unroll
    for (int c = 0; c < NX; ++c) Tb[c] = o.tcolb[c] * wb;
#pragma unroll
    for (int k = 0; k < NU; ++k) brow[k] = o.abrow[NX + k];
    rb_mul<NX, NX, true>(o.abrow, T, S);
    rb_mul<NU, NX, false>(brow, Tb, S);
    bz = rb_mulv<NU>(brow, o.zkb * wb, rb_mulv<NX>(o.abrow, o.zk * wk)) - fma(o.z1x, q1, o.z1l);
#pragma unroll
    for (int c = 0; c < NX; ++c) S[c] += (c == i) ? q1 : 0.0;
  } else {
    rb_leaf<NX, W>(i, o.abrow, T, o.zk * wk, rb_rcp(o.q1), o.z1l, o.z1x, S, bz);
  }
#pragma unroll
  for (int c = 0; c < NX; ++c) S[c] = (S[c] - (o.dl[c] + o.dr[c])) + U[c];
  bz = (bz - (o.gl + o.gr)) + ub;
}

template <int NX, int NU>
__global__ __launch_bounds__(kChainTopThreads) void reduced_chain_top(Dims d, const int l0, const double* __restrict__ AB,
                                                                      const double* __restrict__ QR,
                                                                      const double* __restrict__ rhs, const double* red,
                                                                      double* rec, int* __restrict__ info,
                                                                      double* __restrict__ ytop) {
  static_assert(kChainTopFits<NX, NU>, "panel and leaf tile fit a DPP row");
  constexpr int NN = NX * NX, REC = 2 * NN + NX;
  extern __shared__ double chain_ys[];  // [4][N / 8][NX]: y of separator 8 q + 7 of the workgroup's four problems
  __shared__ ChainTopLds<NX> lds;
  const int N = d.N, K = d.K;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = lane >> 4, i = lane & 15;
  const int ic = i < NX ? i : NX - 1;  // lanes >= NX of a row repeat row / column NX - 1 (lane NX: the rhs column of the panel)
  // the column of [A | B] this lane scales for the leaf tile (split tile: of A, and the lane's column of B is derived from it)
  const int kc = kChainTopSplit<NX, NU> ? (i < 16 ? i : 15) : (i < NX + NU ? i : NX + NU - 1);
  const int bm = 4 * (int)blockIdx.x + r;
  const bool valid = bm < d.batch;  // (a clamped row works on the last problem again and stores nothing)
  const int b = valid ? bm : d.batch - 1;
  const int C = (1 << (K - l0)) - 1, mid = C >> 1;
  const int dir = wave ? -1 : 1;
  double* const ys = chain_ys + (size_t)r * (N >> 3) * NX;
  auto sep_of = [&](const int j) { return ((j + 1) << l0) - 1; };

  // ---------------------------------------------------------------- forward: towards the middle
  double U[NX], ub = 0.0;  // what the eliminated block leaves to the next one: -Y'Y, -Y'v
#pragma unroll
  for (int c = 0; c < NX; ++c) U[c] = 0.0;
  ChainOps<NX, NU> o;
  if (mid > 0) chain_load<NX, NU>(d, l0, b, wave ? C - 1 : 0, dir, ic, kc, AB, QR, rhs, red, o);
  for (int step = 0; step < mid; ++step) {
    const int j = wave ? C - 1 - step : step;
    double S[NX], w[NX], bz;
    chain_assemble<NX, NU>(i, o, U, ub, S, bz);
    // the panel, one column per lane: [E | b]; the rhs column is lane NX's, gathered from the rows
    dpp_fence(bz);
    sfor<NX>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      const double bk = row_bc<k>(bz);
      w[k] = (i == NX) ? bk : -o.cpl[k];
    });
    // the next block's operands travel while this one is factored
    const int jn = j + dir;
    chain_load<NX, NU>(d, l0, b, jn, jn == mid ? 0 : dir, ic, kc, AB, QR, rhs, red, o);
    if (rb_chol_inv<NX, false>(i, S, w) && i == 0 && valid) {
      // one count per tree level this launch stands for (ndlqr_hip.h: what the count means)
      atomicAdd(info + b, K - l0);
      atomicAdd(info + d.batch, K - l0);
    }
    if (valid) {
      double* const sc = rec + ((size_t)b * N + sep_of(j)) * REC;
      if (i < NX) {
#pragma unroll
        for (int k = 0; k < NX; ++k) sc[k * NX + i] = w[k];   // Y(k, i)
        store_row<NX>(sc + NN + i * NX, S);                   // L(i, :)
      } else if (i == NX) {
#pragma unroll
        for (int k = 0; k < NX; ++k) sc[2 * NN + k] = w[k];   // v(k)
      }
    }
    // U(i, c) = -sum_k Y(k, i) Y(k, c), ub(i) = -sum_k Y(k, i) v(k): column c's entry from lane c inside the FMA
#pragma unroll
    for (int c = 0; c < NX; ++c) U[c] = 0.0;
    ub = 0.0;
    dpp_fence(w);
    sfor<NX>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      sfor<NX>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        fnmac_bc<c>(U[c], w[k], w[k]);
      });
      fnmac_bc<NX>(ub, w[k], w[k]);
    });
  }
  if (mid == 0 && wave == 0) chain_load<NX, NU>(d, l0, b, 0, 0, ic, kc, AB, QR, rhs, red, o);

  // ---------------------------------------------------------------- the middle block
  if (wave == 1) {
#pragma unroll
    for (int c = 0; c < NX; ++c) lds.hand[r][c][i] = U[c];
    lds.hand[r][NX][i] = ub;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's scratch is in L2 before it is read back
  __syncthreads();
  double ynext;
  if (wave == 0) {
    double S[NX], w[NX], bz;
#pragma unroll
    for (int c = 0; c < NX; ++c) U[c] += lds.hand[r][c][i];
    ub += lds.hand[r][NX][i];
    chain_assemble<NX, NU>(i, o, U, ub, S, bz);
    if (rb_chol_inv<NX>(i, S, w) && i == 0 && valid) {
      atomicAdd(info + b, K - l0);
      atomicAdd(info + d.batch, K - l0);
    }
    if (i < NX) {
#pragma unroll
      for (int c = 0; c < NX; ++c) lds.lmid[r][i][c] = S[c];
    }
    wave_lds_sync();
    double lrow[NX], lcol[NX];
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      const double up = lds.lmid[r][c][ic];
      lrow[c] = (c < i && i < NX) ? S[c] : 0.0;
      lcol[c] = (c > i && i < NX) ? up : 0.0;
    }
    const double dinv = rb_rcp(lds.lmid[r][ic][ic]);
    ynext = rb_llt_solve<NX>(bz, lrow, lcol, dinv);
    lds.ymid[r][i] = ynext;
    if (i < NX) ys[(sep_of(mid) >> 3) * NX + i] = ynext;
  }
  __syncthreads();
  if (wave == 1) ynext = lds.ymid[r][i];

  // ---------------------------------------------------------------- backward: outwards, y_j = L^-T (v - Y y_next)
  // (unit-diagonal form like rb_backsub_cols: L = L~ D, so that a substitution step is one DPP FMA)
  struct Back { double yrow[NX], lcol[NX], ld, v; };
  auto back_load = [&](const int j, Back& k) {
    const double* sc = rec + ((size_t)b * N + sep_of(j)) * REC;
#pragma unroll
    for (int c = 0; c < NX; ++c) k.yrow[c] = sc[ic * NX + c];
#pragma unroll
    for (int e = 0; e < NX; ++e) k.lcol[e] = sc[NN + e * NX + ic];
    k.ld = sc[NN + ic * NX + ic];
    k.v = sc[2 * NN + ic];
  };
  Back cur;
  if (mid > 0) back_load(wave ? mid + 1 : mid - 1, cur);
  for (int step = mid - 1; step >= 0; --step) {
    const int j = wave ? C - 1 - step : step;
    Back nxt;
    back_load(step > 0 ? j - dir : j, nxt);  // (the last round reloads its own block: nobody uses it)
    double x0 = cur.v, x1 = 0.0;
    dpp_fence(ynext);
    sfor<NX>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      if constexpr (c % 2 == 0) fnmac_bc<c>(x0, ynext, cur.yrow[c]);
      else fnmac_bc<c>(x1, ynext, cur.yrow[c]);
    });
    const double dinv = rb_rcp(cur.ld);
    double lc[NX];
#pragma unroll
    for (int e = 0; e < NX; ++e) lc[e] = (e > i && i < NX) ? cur.lcol[e] * dinv : 0.0;
    double x = (x0 + x1) * dinv;
    sfor<NX - 1>([&](auto cc) {
      constexpr int e = NX - 1 - decltype(cc)::value;
      dpp_fence(x);
      fnmac_bc<e>(x, x, lc[e]);
    });
    ynext = x;
    if (i < NX) ys[(sep_of(j) >> 3) * NX + i] = x;
    cur = nxt;
  }
  __syncthreads();

  // ---------------------------------------------------------------- levels l0 - 1 .. 3 from their records, and the results
  for (int q = 0; q < 4; ++q) {
    const int bq = 4 * (int)blockIdx.x + q;
    if (bq < d.batch)  // (uniform over the workgroup)
      backsub_top_body<NX>(d, bq, threadIdx.x, rec, ytop, chain_ys + (size_t)q * (N >> 3) * NX, -1, nullptr, l0,
                           kChainTopThreads);
  }
}

}  // namespace ndlqr
