// launch_reduced.hpp -- internal: the plan of the runtime-sized separator-only schedule (kernels_reduced_mfma.hpp), the
// one table of its workgroup sizes, and the object (ReducedInstance) ndlqr_hip.hip reaches the separator kernel
// through, instantiated once per tile count NB = ceil(nstates / 16) in its own translation unit (reduced_instance.hip)
// -- the way launch_small.hpp does it per block size.
#pragma once
#include "hip_context.hpp"
#include "kernels_reduced_mfma.hpp"

#pragma GCC visibility push(hidden)

// Workgroup size and LDS of separator_reduced_mfma, or ok == false when the shape does not qualify (-> generic-lean);
// by plan_reduced_generic (ndlqr_hip.hip)
struct ReducedGenericPlan {
  bool ok;
  int threads;
  size_t lds;
  int nb;    // 16 x 16 tiles per block row
  bool pad;  // the block does not fill them
  bool keep; // NDLQR_FLAG_KEEP_RECORDS
};

// Workgroup sizes of separator_reduced_mfma per NB: [0] a wavefront per 16-column tile ("two rounds",
// kernels_reduced_mfma.hpp: small workgroups, three or more of them per CU) where the weights fit its lanes, else [1],
// about twice that (0: none -- beyond 64 states the second panel array does not fit the LDS). The plan picks from this
// row and the instance of NB instantiates exactly its entries.
constexpr int kReducedMaxNB = 8;
constexpr int kReducedThreads[kReducedMaxNB + 1][2] = {{0, 0},     {64, 256},  {128, 256}, {192, 512}, {256, 512},
                                                       {320, 0},   {384, 0},   {448, 0},   {512, 0}};

// The entry point of one tile count, as ndlqr_hip.hip dispatches to it: the separator launch of tree level `level`
// on the current buffer set's stream
struct ReducedInstance {
  int nb;
  void (*separator)(NdlqrHipCtx* c, const ReducedGenericPlan& p, int level);
};

template <int NB, int NT>
static void launch_separator_reduced(NdlqrHipCtx* c, const ReducedGenericPlan& p, const int l) {
  const ndlqr::Dims& d = c->d;
  BufferSet& s = c->set[c->cur];
  const dim3 grid(d.N >> (l + 1), d.batch);
#define NDLQR_LAUNCH_SEP2(L0_, PAD_)                                                                            \
  hipLaunchKernelGGL((ndlqr::separator_reduced_mfma<NB, NT, L0_, PAD_>), grid, dim3(NT), p.lds, s.stream, d, l, \
                     c->AB, c->QR, s.rhs, s.red, s.rec, c->info)
  if (l == 0 && p.pad) NDLQR_LAUNCH_SEP2(true, true);
  else if (l == 0) NDLQR_LAUNCH_SEP2(true, false);
  else if (p.pad) NDLQR_LAUNCH_SEP2(false, true);
  else NDLQR_LAUNCH_SEP2(false, false);
#undef NDLQR_LAUNCH_SEP2
}

template <int NB>
static void separator_reduced(NdlqrHipCtx* c, const ReducedGenericPlan& p, const int l) {
  if constexpr (kReducedThreads[NB][1] != 0) {
    if (p.threads == kReducedThreads[NB][1]) return launch_separator_reduced<NB, kReducedThreads[NB][1]>(c, p, l);
  }
  launch_separator_reduced<NB, kReducedThreads[NB][0]>(c, p, l);
}

template <int NB>
static ReducedInstance make_reduced_instance() {
  return ReducedInstance{NB, separator_reduced<NB>};
}

#define NDLQR_REDUCED_NAME_(NB_) ndlqr_reduced_##NB_
#define NDLQR_REDUCED_NAME(NB_) NDLQR_REDUCED_NAME_(NB_)
// one line per tile count: NDLQR_REDUCED_INSTANCE(NB), as small_instances.def lists the block sizes
#define NDLQR_REDUCED_INSTANCES \
  NDLQR_REDUCED_INSTANCE(1) NDLQR_REDUCED_INSTANCE(2) NDLQR_REDUCED_INSTANCE(3) NDLQR_REDUCED_INSTANCE(4) \
  NDLQR_REDUCED_INSTANCE(5) NDLQR_REDUCED_INSTANCE(6) NDLQR_REDUCED_INSTANCE(7) NDLQR_REDUCED_INSTANCE(8)

#pragma GCC visibility pop
