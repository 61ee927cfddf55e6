// reduced_instance.hip -- the separator kernel of the runtime-sized separator-only schedule (kernels_reduced_mfma.hpp)
// for one tile count. Compiled once per NB = 1 .. 8 with -DNDLQR_RED_NB=<NB>; exports (inside the library) the one
// object ndlqr_hip.hip dispatches through, ndlqr_reduced_<NB>: the ReducedInstance of launch_reduced.hpp.
#include "launch_reduced.hpp"

#if !defined(NDLQR_RED_NB)
#error "compile with -DNDLQR_RED_NB=1..8"
#endif

#pragma GCC visibility push(hidden)
extern const ReducedInstance NDLQR_REDUCED_NAME(NDLQR_RED_NB);
const ReducedInstance NDLQR_REDUCED_NAME(NDLQR_RED_NB) = make_reduced_instance<NDLQR_RED_NB>();
#pragma GCC visibility pop
