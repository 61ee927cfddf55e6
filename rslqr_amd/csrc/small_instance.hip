// small_instance.hip -- one size-specialised instance of the kernels in kernels_small.hpp.
// Compiled once per line of small_instances.def with -DNDLQR_INST_NX=<nstates>
// -DNDLQR_INST_NU=<ninputs>; exports the one object ndlqr_hip.hip dispatches through,
// ndlqr_small_<nx>_<nu>: the SmallInstance of launch_small.hpp.
#include "launch_small.hpp"

#if !defined(NDLQR_INST_NX) || !defined(NDLQR_INST_NU)
#error "compile with -DNDLQR_INST_NX=... -DNDLQR_INST_NU=..."
#endif

extern const SmallInstance NDLQR_SMALL_NAME(NDLQR_INST_NX, NDLQR_INST_NU);
const SmallInstance NDLQR_SMALL_NAME(NDLQR_INST_NX, NDLQR_INST_NU) = make_small_instance<NDLQR_INST_NX, NDLQR_INST_NU>();
