// launch_small.hpp -- internal: launch sequences of the size-specialised kernels and the table entry
// (SmallInstance) the core unit, ndlqr_hip.hip, reaches them through, instantiated once per (nstates, ninputs) in its own
// translation unit (small_instance.hip) so that the instances compile in parallel.
#pragma once
#include "hip_context.hpp"
#include "kernels_leaf.hpp"
#include "kernels_small.hpp"
#include "kernels_bottom_reduced.hpp"
#include "kernels_rowbcast.hpp"
#include "kernels_chain_top.hpp"

// Size-specialised launch sequences.
//   separator-only ("reduced"): bottom kernel (leaf phase + levels 0, 1) -> one launch per upper level
//       -> back-substitution; fast mode without KEEP, shapes with matrix-core products
//   knot-based: bottom_small (leaf phase + levels 0, 1 on the knot states) -> level_small per upper
//       level (separator + the two boundary knots of every subtree) -> backsub_small (fast mode
//       without KEEP: solution from the records) or apply_small (strict / KEEP: every knot through all
//       upper levels in registers, one pass)
constexpr int kBottomLevels = 2;  // tree levels fused with the leaf phase

// What launch_small does for a context with these flags: decided once per solve by the instance's `plan` entry (plan_solve
// in ndlqr_hip.hip), before the launch sequence is enqueued (and possibly captured), so that the host layer can allocate
// what the schedule needs and knows what it leaves. launch_small only issues the launches this names.
struct SmallPlan {
  bool strict, keep;  // NDLQR_FLAG_STRICT_FP, NDLQR_FLAG_KEEP_FACT: the instance of the knot-based kernels
  bool lean;     // solution by back-substitution from the separator records (fast mode, no KEEP)
  int store_l;   // keep the separator factors for a record-based re-solve (KEEP_RECORDS)
  bool reduced;  // separator-only schedule (bottom_reduced_mc + reduced_level_mc)
  bool tree;     // ... with the whole factorisation in one launch (small batches)
  bool compact;  // ... with compact level-0 records and the two-launch back-substitution (kernels_rowbcast.hpp)
  bool rowbcast; // ... and the bottom levels on the row-broadcast core (four separators per wavefront)
  bool fuse2;    // ... or tree level 2 inside the bottom launch (bottom8_reduced_mc)
  bool compact1; // ... and compact records for the level-1 separators as well (rb_backsub_cols substitutes with L_t)
  bool pair1;    // ... whose two Cholesky passes per workgroup of the fused bottom launch run as one (bottom8_reduced_mc<.., P1>)
  bool lds16;    // ... in at most 16 KB of LDS per workgroup: ten workgroups per CU (bottom8_reduced_mc<.., P1, L16>)
  int level0;    // first tree level with a launch of its own (reduced_level_mc), up to ...
  int ltop;      // ... the first one inside reduced_top_mc (== K: no such launch), which starts at ...
  int top_l0;    // ... this level (level 2 may have gone with the bottom launch)
  bool chain;       // the levels from ltop up as one block-tridiagonal chain per problem (reduced_chain_top) instead of reduced_top_mc
  bool top_sweeps;  // reduced_top_mc also runs the top-down sweep over the records of level >= 3 (else rb_backsub_top does)
  size_t top_lds;   // the sweep array of rb_backsub_top
  const char* schedule;  // ndlqr_hip_schedule
  bool rec_complete, rec_compact;  // KeptState
  bool needs_F;  // the schedule reads or writes the factor array
};

// rb_backsub's thread roles (and those of the re-solve on its records) need eight knots of 2 nx + nu rows in a workgroup
template <int NX, int NU>
constexpr bool kRbBacksubFits = 8 * (2 * NX + NU) <= 256;

// An MPC step that wants nothing but a knot range (NDLQR_SOLN_ONLY): the last launch of a back-substitution whose workgroups
// take eight knots each runs those of the range -- grid and Dims::xoff of that launch.
static inline unsigned apply_grid(const NdlqrHipCtx* c, const ndlqr::Dims& d) {
  return (unsigned)(c->apply_nblk > 0 ? c->apply_nblk : d.N / 8);
}
static inline ndlqr::Dims apply_dims(const NdlqrHipCtx* c, const ndlqr::Dims& d) {
  ndlqr::Dims da = d;
  if (c->apply_nblk > 0) da.xoff += c->apply_blk0;
  return da;
}

// Last launch of the two-launch back-substitution. Instances with nstates + ninputs <= 16 have two bodies (DESIGN.md
// section 3.4): the one that keeps [A | B] in registers -- the default: same-box A/B against the staged body at
// (12,4), (10,4), (9,3), (8,4), (6,3) x 1024 and (12,4,1024) x 512, faster at each -- and,
// with NDLQR_BACKSUB_COLS=0, the LDS-staged one that the larger instances run.
// compact1: the level-1 records are compact too (a full solve of a plan with SmallPlan::compact1 alone).
template <int NX, int NU>
constexpr bool kCompact1Fits = ndlqr::P1OnMatrixCores<NX, NU>::value && NX >= 9 && NX + NU <= 16;

// pair1: the paired level-1 pass of the fused bottom launch leaves a wavefront's tile and couplings of t in its buffer
template <int NX, int NU>
constexpr bool kPair1Fits = kCompact1Fits<NX, NU> && ndlqr::McPair1Layout<NX>::SIZE <= ndlqr::ReducedLds<NX, NU>::NBUF;

// top chain (reduced_chain_top): the instances where it measured faster than the launches it replaces (plan_small)
template <int NX, int NU>
constexpr bool kChainTopMeasured = (NX == 12 && NU == 4) || (NX == 10 && NU == 4) || (NX == 9 && NU == 3) ||
                                   (NX == 8 && NU == 4) || (NX == 6 && NU == 3) || (NX == 13 && NU == 4);

template <int NX, int NU, bool MULTI, class... Args>
static void launch_rb_backsub(const NdlqrHipCtx* c, const dim3 grid, hipStream_t stream, const bool compact1,
                              const Args&... args) {
  if constexpr (NX + NU <= 16) {
    if constexpr (kCompact1Fits<NX, NU> && !MULTI) {
      if (compact1) {
        hipLaunchKernelGGL((ndlqr::rb_backsub<NX, NU, false, true, true>), grid, dim3(ndlqr::kRbBacksubColsThreads), 0, stream,
                           args...);
        return;
      }
    }
    if (c->knobs.backsub_cols != 0) {
      hipLaunchKernelGGL((ndlqr::rb_backsub<NX, NU, MULTI, true>), grid, dim3(ndlqr::kRbBacksubColsThreads), 0, stream, args...);
      return;
    }
  }
  hipLaunchKernelGGL((ndlqr::rb_backsub<NX, NU, MULTI, false>), grid, dim3(256), 0, stream, args...);
}

template <int NX, int NU>
static SmallPlan plan_small(const NdlqrHipCtx* c, const bool strict, const bool keep) {
  const ndlqr::Dims& d = c->d;
  const BufferSet& s = c->set[0];  // (the alternate set is allocated with the same optional buffers: ensure_alt)
  SmallPlan p = {};
  p.strict = strict;
  p.keep = keep;
  // fast mode without KEEP: solution by back-substitution from the separator records (backsub_small
  // resolves K + 4 separators of NX rows in one 256-thread workgroup)
  p.lean = !strict && !keep && (d.K + 4) * NX <= 256;
  p.store_l = (c->flags & NDLQR_FLAG_KEEP_RECORDS) ? 1 : 0;  // factors for a record-based re-solve
  // the record-based re-solve needs every separator's record and factor: KEEP writes them all,
  // KEEP_RECORDS adds the factors to the lean schedule
  p.rec_complete = !strict && (keep || (p.lean && p.store_l));
  p.level0 = p.ltop = p.top_l0 = d.K;
  p.schedule = p.lean ? "knot-lean" : (strict ? "knot-strict" : "knot-keep");
  if constexpr (ndlqr::P1OnMatrixCores<NX, NU>::value) {
    if (p.lean && s.red) {
      p.reduced = true;
      // tree schedule for small batches (at most half a resident round of bottom wavefronts): three
      // launches instead of K + 1; measured cross-over at batch x N / 4 ~ 4096 wavefronts
      p.tree = s.tree_cnt && (c->knobs.tree == 1 || (c->knobs.tree < 0 && (size_t)d.batch * (d.N >> 2) <= 2048));
      // compact level-0 records (L of S-bar only) and the two-launch back-substitution: the tree schedule keeps the
      // one-kernel back-substitution; rb_backsub's thread roles need 8 (2 nx + nu) <= 256 (and rb_backsub_top's sweep
      // array, N / 8 multipliers, has to fit the LDS of its one workgroup per problem). With KEEP_RECORDS (round 4): the
      // same schedule, which then also keeps the factors of the separators of level >= 1 in the slack of the level-0
      // record slots (store_l = 2; the record-based re-solve rb_forward / rb_forward_top works on that: four sweep
      // arrays in the LDS of its one workgroup per problem)
      p.top_lds = sizeof(double) * (size_t)(d.N >> 3) * NX;
      p.compact = !p.tree && d.N >= 16 && kRbBacksubFits<NX, NU> && p.top_lds * (p.store_l ? 4 : 1) <= kLdsMax;
      if (p.compact && p.store_l) p.store_l = 2;
      p.rec_compact = p.compact && p.store_l == 2;
      // row-broadcast bottom kernel (one DPP row holds the rows of S-bar and of [A | B]'): its cost falls
      // with the block size, the matrix-core kernel's does not (16x16 tiles whatever n is). Measured bottom
      // kernel, N = 256 x 1024: (6,3) 0.105 vs 0.170 ms, (8,4) 0.144 vs 0.190, (9,3) 0.202 vs 0.244,
      // (10,4) 0.230 vs 0.271, (12,4) 0.301 vs 0.290 in round 2. Round 3 (paired Cholesky pass that carries the panel):
      // (10,4) 0.230 vs 0.207, (9,3) 0.203 vs 0.187, (8,4) 0.143 vs 0.152, (6,3) 0.104 vs 0.134 -- so it serves n <= 8
      // (NDLQR_ROWBCAST=0/1 overrides)
      p.rowbcast = p.compact && !p.store_l && NX <= 16 && NX + NU <= 16 && (c->knobs.rowbcast == 1 || (c->knobs.rowbcast < 0 && NX <= 8));
      // Levels 0-2 in one launch (bottom8_reduced_mc: two wavefronts per eight knots, the level-2 slot in LDS): 12 % less
      // HBM traffic and one launch less per step; the level-2 work costs inside the bottom launch about what it costs
      // outside, so the step gains little -- and only at the (12,4) instance, where it is the default (same box,
      // profiles/r04_fuse2_ab.txt: (12,4,256) x 1024 0.587 -> 0.579 ms, (12,4,1024) x 512 1.20 -> 1.16, the padded (11,3)
      // 0.578 -> 0.569; (12,8) +2.5 %, (13,4) +0.9 %, (9,3) / (10,4) / (15,2) +-0). NDLQR_FUSE2=0 / 1 overrides.
      p.fuse2 = !p.rowbcast && p.compact && !p.store_l && (c->knobs.fuse2 > 0 || (c->knobs.fuse2 < 0 && NX == 12 && NU == 4));
      // Compact level-1 records: the bottom launch drops W = L^-1, X = W'Y and three quarters of the record stores of
      // its level-1 separators, rb_backsub_cols reads 78 instead of 300 doubles for each and substitutes three times in
      // turn instead of once. Only with the matrix-core bottom kernel and the column back-substitution (n >= 9,
      // n + m <= 16). The default where the slowest of five runs was below the parent's fastest on the same box
      // (profiles/compact1_ab.txt): the (12,4) instance on its default schedule (fused level 2) -- (12,4,256) x 1024
      // 0.537-0.548 -> 0.527-0.533 ms, (12,4,1024) x 512 1.146-1.162 -> 1.072-1.078, the padded (11,3) 0.535-0.539 ->
      // 0.518-0.522 -- and (10,4): 0.473-0.475 -> 0.448-0.456; (9,3) 0.389-0.391 -> 0.383-0.389 touches the parent's range
      // and stays off. NDLQR_COMPACT1=0 / 1 overrides.
      p.compact1 = kCompact1Fits<NX, NU> && p.compact && !p.store_l && !p.rowbcast && c->knobs.backsub_cols != 0 &&
                   (c->knobs.compact1 > 0 ||
                    (c->knobs.compact1 < 0 && ((NX == 12 && NU == 4 && p.fuse2) || (NX == 10 && NU == 4))));
      // Paired level-1 pass: with compact level-1 records the pass of one t has both halves of its wavefront on the same
      // tile, so the fused bottom launch can take the t of its two groups through ONE pass on its first wavefront (two more
      // workgroup barriers, the tiles exchanged through LDS): four Cholesky passes per eight knots instead of five, the
      // same records and, bit for bit, the same solutions. Only where the fused launch runs with compact level-1
      // records. The default where the slowest of five runs was below the parent's fastest on the same box
      // (profiles/pair1_ab.txt): the (12,4) instance -- (12,4,256) x 1024 0.5391-0.5444 -> 0.5248-0.5347 ms,
      // (12,4,1024) x 512 1.0643-1.0761 -> 1.0399-1.0492, the padded (11,3) 0.5169-0.5236 -> 0.5044-0.5106. With
      // NDLQR_FUSE2=1 it also cleared the rule against the present defaults of (10,4), 0.4530-0.4598 -> 0.4447-0.4464 (the
      // fused launch without pairing: 0.4533-0.4593, +-0 as in round 4), and of (9,3) with NDLQR_COMPACT1=1 too,
      // 0.3905-0.3961 -> 0.3804-0.3842; those instances keep their schedule ("reduced", which
      // tests/test_compact1_records.py holds them to) and pair on request. NDLQR_PAIR1=0 / 1 overrides.
      p.pair1 = kPair1Fits<NX, NU> && p.fuse2 && p.compact1 &&
                (c->knobs.pair1 > 0 || (c->knobs.pair1 < 0 && NX == 12 && NU == 4));
      // The paired launch in 16 KB of LDS (bottom8_reduced_mc<.., P1, L16>, Bottom8Lds16): ten workgroups per CU instead of
      // eight (five wavefronts per SIMD at <= 90 VGPRs), no zeroing of the level-2 slot, and the level >= 3 slots next to a
      // workgroup stored once instead of stored, acknowledged and added to atomically. Same records, bit-equal solutions.
      // The default wherever the paired launch runs -- at each of its three instances the slowest of five runs was below
      // the parent's fastest on the same box (profiles/lds16_ab.txt): (12,4,256) x 1024 0.5187-0.5336 -> 0.4965-0.5075 ms
      // pipelined (bottom launch 0.283 -> 0.260: 0.270 from the occupancy alone), (12,4,1024) x 512 1.0640-1.0675 ->
      // 1.0170-1.0239, the padded (11,3) 0.5132-0.5164 -> 0.4897-0.4942; with NDLQR_FUSE2=1 NDLQR_COMPACT1=1 NDLQR_PAIR1=1
      // on both sides (10,4) 0.4476-0.4500 -> 0.4195-0.4250 and (9,3) 0.3809-0.3882 -> 0.3690-0.3763.
      // NDLQR_BOTTOM_LDS16=0 keeps the 20 KB launch.
      p.lds16 = p.pair1 && c->knobs.bottom_lds16 != 0;
      p.schedule = p.tree ? "reduced-tree"
                   : !p.compact ? "reduced-records"
                   : p.store_l ? "reduced-compact-records" : (p.fuse2 ? "reduced-fused2" : "reduced");
      if (!p.tree) {
        // upper levels: one launch per level while a level has more than four separators per problem, then the
        // last three levels in one launch (reduced_top_mc; NDLQR_NO_TOP=1: a launch per level to the root)
        const int top_levels = d.K - c->knobs.top_levels >= 3 ? c->knobs.top_levels : 3;
        p.level0 = p.fuse2 ? 3 : 2;
        p.ltop = (d.K >= 5 && !c->knobs.no_top) ? d.K - top_levels : d.K;
        p.top_l0 = (p.fuse2 && p.ltop < 3) ? 3 : p.ltop;  // (level 2 went with the bottom launch)
        // ... which also runs the top-down sweep over the records of level >= 3 when the back-substitution is the
        // two-launch form and its array fits the workgroup's LDS
        p.top_sweeps = p.ltop < d.K && p.compact && p.top_lds <= 4 * sizeof(ndlqr::ReducedLds<NX, NU, false>);
        // The separators of level >= max(3, K - 5) as one block-tridiagonal chain per problem (reduced_chain_top,
        // kernels_chain_top.hpp: at most 31 blocks, four problems per wavefront, one launch) in place of the level launches
        // above that level and of reduced_top_mc; the levels below it keep reduced_level_mc, and the chain's launch runs the
        // top-down sweep over their records. Only where no records of those levels are kept (the chain's scratch lies in
        // their slots) and the sweep arrays of a workgroup's four problems fit its LDS. NDLQR_NO_TOP / NDLQR_TOP_LEVELS
        // (A/B of reduced_top_mc) keep the tree. The default where the slowest of five runs was below
        // the parent's fastest on the same box (profiles/chain_top_ab.txt): horizons of 256 knots at (12,4) 0.4911-0.4998
        // -> 0.4636-0.4686 ms, the padded (11,3) 0.4786-0.4868 -> 0.4499-0.4554, (10,4) 0.4486-0.4506 -> 0.4202-0.4245, (9,3)
        // 0.3858-0.3881 -> 0.3726-0.3777, (8,4) 0.3114-0.3195 -> 0.2951-0.3044, (6,3) 0.2217-0.2251 -> 0.2068-0.2088, (13,4)
        // 0.7004-0.7134 -> 0.6651-0.6748 (x 1024). (12,4,1024) x 512, two level launches under a 31-block chain, touches the
        // parent's range (0.9893-0.9995 -> 0.9762-0.9938) and stays on request, like every horizon that was not measured.
        // NDLQR_TOP_CHAIN=0 / 1 overrides.
        if constexpr (ndlqr::kChainTopFits<NX, NU>) {
          p.chain = p.compact && !p.store_l && d.K >= 4 && !c->knobs.no_top && !c->knobs.top_levels_set &&
                    sizeof(ndlqr::ChainTopLds<NX>) + 4 * p.top_lds <= kLdsMax &&
                    (c->knobs.top_chain > 0 || (c->knobs.top_chain < 0 && d.K == 8 && kChainTopMeasured<NX, NU>));
          if (p.chain) {
            p.ltop = p.top_l0 = d.K - ndlqr::kChainTopMaxLevels > 3 ? d.K - ndlqr::kChainTopMaxLevels : 3;
            p.top_sweeps = true;
          }
        }
      }
    }
  }
  // the separator-only schedule touches F only to park the factors of KEEP_RECORDS under its full-record forms
  p.needs_F = !(p.reduced && p.store_l != 1);
  return p;
}

template <int NX, int NU, bool STRICT, bool KEEP>
static int launch_small(NdlqrHipCtx* c, const SmallPlan& plan) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  using Sh = ndlqr::SchurShape<NX, NU>;
  constexpr int JB = kBottomLevels;
  const bool lean = plan.lean;
  const int store_l = plan.store_l;
  if constexpr (!STRICT && !KEEP && ndlqr::P1OnMatrixCores<NX, NU>::value) {
    if (plan.reduced) {
      {
        ScopedSlot t(c, SLOT_BOTTOM);
        if (plan.rowbcast) {  // one separator per DPP row, four per wavefront
          if constexpr (NX <= 16 && NX + NU <= 16)
            hipLaunchKernelGGL((ndlqr::rb_bottom<NX, NU>), dim3(d.N >> 4, d.batch), dim3(64), 0, s.stream, d, c->AB,
                               c->QR, s.rhs, s.red, s.rec, c->info);
        } else if (plan.fuse2) {
          bool done = false;
          if constexpr (kPair1Fits<NX, NU>) {
            if (plan.lds16) {
              hipLaunchKernelGGL((ndlqr::bottom8_reduced_mc<NX, NU, true, true, true>), dim3(d.N >> 3, d.batch), dim3(128), 0,
                                 s.stream, d, c->AB, c->QR, s.rhs, s.red, s.rec, c->info);
              done = true;
            } else if (plan.pair1) {
              hipLaunchKernelGGL((ndlqr::bottom8_reduced_mc<NX, NU, true, true>), dim3(d.N >> 3, d.batch), dim3(128), 0, s.stream,
                                 d, c->AB, c->QR, s.rhs, s.red, s.rec, c->info);
              done = true;
            }
          }
          if constexpr (kCompact1Fits<NX, NU>) {
            if (!done && plan.compact1) {
              hipLaunchKernelGGL((ndlqr::bottom8_reduced_mc<NX, NU, true>), dim3(d.N >> 3, d.batch), dim3(128), 0, s.stream, d,
                                 c->AB, c->QR, s.rhs, s.red, s.rec, c->info);
              done = true;
            }
          }
          if (!done)
            hipLaunchKernelGGL((ndlqr::bottom8_reduced_mc<NX, NU>), dim3(d.N >> 3, d.batch), dim3(128), 0, s.stream, d,
                               c->AB, c->QR, s.rhs, s.red, s.rec, c->info);
        } else if (plan.tree)
          hipLaunchKernelGGL((ndlqr::bottom_reduced_mc<NX, NU, true>), dim3(d.N >> 2, d.batch), dim3(64), 0, s.stream,
                             d, c->AB, c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l, s.tree_cnt, 0);
        else if (plan.compact) {
          bool done = false;
          if constexpr (kCompact1Fits<NX, NU>) {
            if (plan.compact1) {
              hipLaunchKernelGGL((ndlqr::bottom_reduced_mc<NX, NU, false, true, true>), dim3(d.N >> 2, d.batch), dim3(64), 0,
                                 s.stream, d, c->AB, c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l, nullptr, 1);
              done = true;
            }
          }
          if (!done)
            hipLaunchKernelGGL((ndlqr::bottom_reduced_mc<NX, NU, false, true>), dim3(d.N >> 2, d.batch), dim3(64), 0, s.stream,
                               d, c->AB, c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l, nullptr, 1);
        } else
          hipLaunchKernelGGL((ndlqr::bottom_reduced_mc<NX, NU, false>), dim3(d.N >> 2, d.batch), dim3(64), 0, s.stream,
                             d, c->AB, c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l, nullptr, 0);
      }
      for (int l = plan.level0; l < plan.ltop; ++l) {
        ScopedSlot t(c, SLOT_UPPER);
        hipLaunchKernelGGL((ndlqr::reduced_level_mc<NX, NU>), dim3(d.N >> (l + 1), d.batch), dim3(64), 0, s.stream,
                           d, l, c->AB, c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l);
      }
      bool chained = false;
      if constexpr (ndlqr::kChainTopFits<NX, NU>) {
        if (plan.chain) {
          ScopedSlot t(c, SLOT_TOP);
          const size_t lds = 4 * plan.top_lds;
          (void)allow_dynamic_lds(&ndlqr::reduced_chain_top<NX, NU>, lds);
          hipLaunchKernelGGL((ndlqr::reduced_chain_top<NX, NU>), dim3((d.batch + 3) / 4), dim3(ndlqr::kChainTopThreads), lds,
                             s.stream, d, plan.ltop, c->AB, c->QR, s.rhs, s.red, s.rec, c->info, s.ytop);
          chained = true;
        }
      }
      if (!chained && plan.ltop < d.K) {
        ScopedSlot t(c, SLOT_TOP);  // (a profile slot of its own: one kernel name per slot, like rocprofv3's per-kernel averages)
        hipLaunchKernelGGL((ndlqr::reduced_top_mc<NX, NU>), dim3(d.batch), dim3(256), 0, s.stream, d, plan.top_l0, c->AB,
                           c->QR, s.rhs, s.red, s.rec, c->F, c->info, store_l, plan.top_sweeps ? s.ytop : (double*)nullptr);
      }
      ScopedSlot t(c, SLOT_APPLY);
      if (plan.compact) {
        if (!plan.top_sweeps) {  // (beyond the default limit of dynamic LDS: horizons of 8192 knots at 12 states)
          (void)allow_dynamic_lds(&ndlqr::rb_backsub_top<NX>, plan.top_lds);
          hipLaunchKernelGGL((ndlqr::rb_backsub_top<NX>), dim3(d.batch), dim3(256), plan.top_lds, s.stream, d, s.rec, s.ytop);
        }
        // (an MPC step that asked for nothing but a knot range -- NDLQR_SOLN_ONLY -- runs the workgroups of that range)
        launch_rb_backsub<NX, NU, false>(c, dim3(apply_grid(c, d), d.batch), s.stream, plan.compact1,
                           apply_dims(c, d), c->AB, c->QR, s.rhs, s.rec, s.ytop, s.z);
      } else {
        hipLaunchKernelGGL((ndlqr::backsub_small<NX, NU>), dim3(apply_grid(c, d), d.batch), dim3(256), 0, s.stream, apply_dims(c, d), c->AB,
                           c->QR, s.rhs, s.rec, s.z);
      }
      return NDLQR_OK;
    }
  }
  {
    ScopedSlot t(c, SLOT_BOTTOM);
    hipLaunchKernelGGL((ndlqr::bottom_small<NX, NU, STRICT, KEEP, JB>), dim3(d.N >> JB, d.batch), dim3(32 << JB), 0,
                       s.stream, d, c->AB, c->QR, s.rhs, c->F, s.z, c->info, s.rec, lean ? 1 : 0,
                       ((lean || (KEEP && !STRICT)) ? 1 : 0) | (store_l ? 2 : 0));
  }
  for (int l = JB; l < d.K; ++l) {  // separator + boundary update of a level in one launch
    ScopedSlot t(c, SLOT_UPPER);
    hipLaunchKernelGGL((ndlqr::level_small<NX, NU, STRICT, KEEP>), dim3(d.N >> (l + 1), d.batch), dim3(64), 0,
                       s.stream, d, l, c->AB, c->F, s.z, s.rec, c->info, store_l);
  }
  ScopedSlot t(c, SLOT_APPLY);
  if (lean) {
    if constexpr (!STRICT && !KEEP)
      hipLaunchKernelGGL((ndlqr::backsub_small<NX, NU>), dim3(apply_grid(c, d), d.batch), dim3(256), 0, s.stream, apply_dims(c, d), c->AB,
                         c->QR, s.rhs, s.rec, s.z);
    return NDLQR_OK;
  }
  const size_t lds = sizeof(double) * (size_t)(d.K - JB) * Sh::REC;
  hipLaunchKernelGGL((ndlqr::apply_small<NX, NU, STRICT, KEEP>), dim3(d.N / Sh::KPB, d.batch), dim3(256), lds,
                     s.stream, d, JB, c->F, s.z, s.rec);
  return NDLQR_OK;
}

// Record-based re-solve (fast mode, specialised sizes): forward pass over the separators, then
// the same back-substitution as the full solve: right-hand side `rhs`, solution into `z`.
template <int NX, int NU>
static void launch_rhs_records(NdlqrHipCtx* c, const double* rhs, double* z) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  if constexpr (ndlqr::P1OnMatrixCores<NX, NU>::value && kRbBacksubFits<NX, NU>) {
    if (c->kept.rec_compact) {
      // the compact records of the default schedule (round 4): forward pass over the separators with the right-hand-side
      // column alone, then the back-substitution of a full solve. s.red (the accumulator slots, idle here) holds what
      // the eight-knot blocks push to the separators between them: [batch][N / 8][2][NX].
      {
        ScopedSlot t(c, SLOT_SEP);
        hipLaunchKernelGGL((ndlqr::rb_forward<NX, NU>), dim3(d.N / 8, d.batch), dim3(256), 0, s.stream, d, c->AB, c->QR,
                           rhs, s.rec, s.red);
      }
      {
        ScopedSlot t(c, SLOT_UPPER);
        const size_t lds = sizeof(double) * 4 * (size_t)(d.N >> 3) * NX;
        (void)allow_dynamic_lds(&ndlqr::rb_forward_top<NX, NU>, lds);
        hipLaunchKernelGGL((ndlqr::rb_forward_top<NX, NU>), dim3(d.batch), dim3(256), lds, s.stream, d, c->AB, c->QR,
                           rhs, s.rec, (const double*)s.red, s.ytop);
      }
      ScopedSlot t(c, SLOT_APPLY);
      launch_rb_backsub<NX, NU, false>(c, dim3(apply_grid(c, d), d.batch), s.stream, false,
                         apply_dims(c, d), c->AB, c->QR, rhs, s.rec, s.ytop, z);
      return;
    }
  }
  {
    ScopedSlot t(c, SLOT_SEP);
    hipLaunchKernelGGL((ndlqr::rhs_forward_small<NX, NU>), dim3(d.N / 8, d.batch), dim3(64), 0, s.stream, d, c->AB,
                       c->QR, rhs, c->F, s.rec, z);
  }
  if (d.K > 3) {
    ScopedSlot t(c, SLOT_UPPER);
    const size_t lds = sizeof(double) * (size_t)(d.N / 8) * NX;
    hipLaunchKernelGGL((ndlqr::rhs_forward_upper<NX, NU>), dim3(d.batch), dim3(512), lds, s.stream, d, c->AB, c->QR,
                       rhs, c->F, s.rec, z);
  }
  {
    ScopedSlot t(c, SLOT_APPLY);
    hipLaunchKernelGGL((ndlqr::backsub_small<NX, NU>), dim3(apply_grid(c, d), d.batch), dim3(256), 0, s.stream, apply_dims(c, d), c->AB,
                       c->QR, rhs, s.rec, z);
  }
}

// Several right-hand sides per problem against the compact records (SURVEY.md 8(f)-2 "multiple right-hand sides";
// ndlqr_hip_solve_multi_rhs): `count` right-hand sides in all, right-hand side j belongs to problem j % batch; rhs / zsep /
// fsum / ytop / z are arrays of `count` entries, the inputs and records those of the context. Returns false when the
// shape has no such form.
template <int NX, int NU>
static bool launch_multi_rhs(NdlqrHipCtx* c, const int count, const double* rhs, double* zsep, double* fsum, double* ytop,
                             double* z) {
  if constexpr (ndlqr::P1OnMatrixCores<NX, NU>::value && kRbBacksubFits<NX, NU>) {
    const ndlqr::Dims& d = c->d;
    BufferSet& s = c->set[c->cur];
    const size_t lds = sizeof(double) * 4 * (size_t)(d.N >> 3) * NX;
    if (lds > kLdsMax) return false;
    (void)allow_dynamic_lds(&ndlqr::rb_forward_top<NX, NU, true>, lds);
    hipLaunchKernelGGL((ndlqr::rb_forward<NX, NU, true>), dim3(d.N / 8, count), dim3(256), 0, s.stream, d, c->AB, c->QR, rhs,
                       s.rec, fsum, d.batch, zsep);
    hipLaunchKernelGGL((ndlqr::rb_forward_top<NX, NU, true>), dim3(count), dim3(256), lds, s.stream, d, c->AB, c->QR, rhs,
                       s.rec, (const double*)fsum, ytop, d.batch, zsep);
    // (a knot range alone: ndlqr_hip_solve_multi_rhs_slices)
    launch_rb_backsub<NX, NU, true>(c, dim3(apply_grid(c, d), count), s.stream, false,
                       apply_dims(c, d), c->AB, c->QR, rhs, (const double*)s.rec, (const double*)ytop, z, d.batch,
                       (const double*)zsep);
    return true;
  } else {
    return false;
  }
}

// Time-axis sharding of the separator-only schedule: the horizon is cut into G
// chunks of N / G knots, rank g works on chunk g. The tree levels 0 .. K - log2(G) - 1 lie inside a chunk; what a
// chunk exposes to the rest of the tree is what any subtree exposes: the blocks it adds to the slots of the G - 1
// separators between the chunks (and the couplings between those). Phase 0 (here): bottom kernel and level launches
// restricted to the chunk (Dims::xoff). Between the phases the caller sums the top slots over the ranks (one
// all-reduce of (G - 1) slots per problem: every rank contributes the halves its chunk wrote, zeros elsewhere).
// Phase 1: the top log2(G) levels -- G - 1 separators, eliminated REDUNDANTLY by every rank, which saves sending
// multipliers back --, the top-down sweep, and the back-substitution of the chunk's knots.
// Inputs are resident for the whole horizon on every rank (this prototype shards the work, not the storage).
template <int NX, int NU>
static int launch_time_shard(NdlqrHipCtx* c, const int phase, const int g, const int G) {
  ndlqr::Dims d = c->d;
  BufferSet& bs = c->set[c->cur];
  int lg = 0;
  while ((1 << lg) < G) ++lg;
  if (G < 2 || (1 << lg) != G || g < 0 || g >= G) return NDLQR_ERR_INVALID;
  if constexpr (!ndlqr::P1OnMatrixCores<NX, NU>::value) {
    return NDLQR_ERR_INVALID;
  } else {
    const int ltop = d.K - lg;  // levels [0, ltop) lie inside a chunk
    if (!bs.red || !bs.ytop || ltop < 4 || !kRbBacksubFits<NX, NU> || (c->flags & ~NDLQR_FLAG_PROFILE)) return NDLQR_ERR_INVALID;
    const size_t top_lds = sizeof(double) * (size_t)(d.N >> 3) * NX;
    if (top_lds > kLdsMax) return NDLQR_ERR_INVALID;  // (rb_backsub_top's sweep array has to fit one workgroup's LDS)
    (void)allow_dynamic_lds(&ndlqr::rb_backsub_top<NX>, top_lds);
    constexpr size_t SLOT = ndlqr::RedSlot<NX>::SIZE;
    if (phase == 0) {
      // whatever an earlier exchange left in the top slots goes: this rank's chunk writes its halves afresh
      for (int j = 1; j < G; ++j) {
        const int s = j * (d.N / G) - 1;
        double* p = bs.red + (size_t)(s >> 2) * SLOT;
        if (hipMemset2DAsync(p, sizeof(double) * (size_t)(d.N >> 2) * SLOT, 0, sizeof(double) * SLOT, (size_t)d.batch,
                             bs.stream) != hipSuccess)
          return NDLQR_ERR_NO_DEVICE;
      }
      {
        ScopedSlot t(c, SLOT_BOTTOM);
        const int cnt = (d.N >> 2) / G;
        d.xoff = g * cnt;
        hipLaunchKernelGGL((ndlqr::bottom_reduced_mc<NX, NU, false, true>), dim3(cnt, d.batch), dim3(64), 0, bs.stream, d,
                           c->AB, c->QR, bs.rhs, bs.red, bs.rec, c->F, c->info, 0, nullptr, 1);
      }
      for (int l = 2; l < ltop; ++l) {
        ScopedSlot t(c, SLOT_UPPER);
        const int cnt = (d.N >> (l + 1)) / G;
        d.xoff = g * cnt;
        hipLaunchKernelGGL((ndlqr::reduced_level_mc<NX, NU>), dim3(cnt, d.batch), dim3(64), 0, bs.stream, d, l, c->AB,
                           c->QR, bs.rhs, bs.red, bs.rec, c->F, c->info, 0);
      }
    } else {
      d.xoff = 0;
      for (int l = ltop; l < d.K; ++l) {
        ScopedSlot t(c, SLOT_TOP);
        hipLaunchKernelGGL((ndlqr::reduced_level_mc<NX, NU>), dim3(d.N >> (l + 1), d.batch), dim3(64), 0, bs.stream, d,
                           l, c->AB, c->QR, bs.rhs, bs.red, bs.rec, c->F, c->info, 0);
      }
      ScopedSlot t(c, SLOT_APPLY);
      // (the sweep runs over every separator of level >= 3; those of other chunks have no records here and resolve to
      //  garbage nobody reads: a separator depends on its ancestors only, which are in this chunk or among the top ones)
      hipLaunchKernelGGL((ndlqr::rb_backsub_top<NX>), dim3(d.batch), dim3(256), top_lds, bs.stream, d, bs.rec, bs.ytop);
      const int cnt = (d.N >> 3) / G;
      d.xoff = g * cnt;
      launch_rb_backsub<NX, NU, false>(c, dim3(cnt, d.batch), bs.stream, false, d, c->AB, c->QR,
                         bs.rhs, bs.rec, bs.ytop, bs.z);
    }
    c->kept.schedule = "reduced-time-shard";
    c->kept.family = Family::Small;
    c->kept.time_shard = true;
    return NDLQR_OK;
  }
}

// The entry points of one size-specialised instance, as ndlqr_hip.hip dispatches to them: one object per line of
// small_instances.def, exported by that line's translation unit (small_instance.hip)
struct SmallInstance {
  int nx, nu;
  int kpb;   // knots per workgroup of its Schur kernels
  int slot;  // doubles per accumulator slot
  SmallPlan (*plan)(const NdlqrHipCtx*, bool strict, bool keep);  // what `solve` would do (plan_small)
  int (*solve)(NdlqrHipCtx*, const SmallPlan&);                   // factor + solve launch sequence (launch_small)
  void (*rhs)(NdlqrHipCtx*, const double* rhs, double* z);        // record-based re-solve of `rhs` into `z` (launch_rhs_records)
  int (*tshard)(NdlqrHipCtx*, int phase, int g, int G);           // time-axis sharding: chunk g of G, phase 0 / 1 (launch_time_shard)
  // several right-hand sides per problem (launch_multi_rhs)
  bool (*multi)(NdlqrHipCtx*, int count, const double* rhs, double* zsep, double* fsum, double* ytop, double* z);
};

template <int NX, int NU>
static int solve_small(NdlqrHipCtx* c, const SmallPlan& p) {
  if (p.strict) return p.keep ? launch_small<NX, NU, true, true>(c, p) : launch_small<NX, NU, true, false>(c, p);
  return p.keep ? launch_small<NX, NU, false, true>(c, p) : launch_small<NX, NU, false, false>(c, p);
}

// (not constexpr: a constant-initialised const object would be emitted for the device as well, where these host
//  functions do not exist)
template <int NX, int NU>
static SmallInstance make_small_instance() {
  return {NX, NU, ndlqr::SchurShape<NX, NU>::KPB, (int)ndlqr::RedSlot<NX>::SIZE, plan_small<NX, NU>, solve_small<NX, NU>,
          launch_rhs_records<NX, NU>, launch_time_shard<NX, NU>, launch_multi_rhs<NX, NU>};
}
// the name of the instance's object
#define NDLQR_SMALL_NAME_(NX_, NU_) ndlqr_small_##NX_##_##NU_
#define NDLQR_SMALL_NAME(NX_, NU_) NDLQR_SMALL_NAME_(NX_, NU_)
