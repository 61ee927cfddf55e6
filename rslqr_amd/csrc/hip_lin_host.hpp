// hip_lin_host.hpp -- internal: what the units of the solve with linear inequality constraints share on the host side
// (hip_lin.hip: the solve, its adjoint and its read-outs; hip_lin_polish.hip: the active-set polish). Declarations and
// inline helpers only; no kernel is launched from here.
#pragma once
#include "hip_host.hpp"

// (the kernels hold static LDS next to the dynamic: ask well below the default limit. `asked`: what this context has
//  asked for this kernel already -- one of the lds_asked of the feature's state --, so that a call does not ask again)
template <class Kernel>
static hipError_t allow_lin_lds(Kernel* kernel, size_t lds, size_t& asked) {
  if (lds <= 32 * 1024 || lds <= asked) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) asked = lds;
  return e;
}

static inline int need_constrained(const NdlqrHipCtx* c, const char* who) {
  if (c->lin.active && c->cost.dense) return NDLQR_OK;
  return refuse(std::string(who) + ": the solver is not in constrained mode (ndlqr_InitializeBatchFlatConstrained first; "
                "every other initialiser leaves it)");
}

// The shifted reduced problem in force instead of the plain one, with the flags of the shifted factorisation instead of
// the caller's: from open() to close(). A scope left without close() (an early return) restores the same: the plain
// reduced problem of CostState packed again, the caller's flags, and the kept factorisation -- which belongs to the
// shifted problem -- forgotten for the plain API.
struct ShiftedReduction {
  NdlqrHipCtx* c;
  const unsigned user_flags;
  bool open_ = false;
  explicit ShiftedReduction(NdlqrHipCtx* ctx) : c(ctx), user_flags(ctx->flags) {}
  ShiftedReduction(const ShiftedReduction&) = delete;
  ~ShiftedReduction() { (void)close(); }
  // (ndlqr_hip_pack_flat_device is an initialiser: it leaves both modes, which last through this scope)
  int pack(const double* At, const double* Bt, const double* qt, const double* rt, const double* dt, const double* x0t) {
    const size_t kn = (size_t)c->du.batch * c->du.N;
    const int err = ndlqr_hip_pack_flat_device(c, At, Bt, c->cost.ones, c->cost.ones + kn * c->du.n, qt, rt, dt, x0t);
    c->cost.dense = true;
    c->lin.active = true;
    return err;
  }
  int open(unsigned flags) {
    open_ = true;
    c->flags = flags;
    return repack();
  }
  // the shifted reduced problem packed (again: LinState's arrays were written anew for new penalties)
  int repack() {
    const LinState& k = c->lin;
    return pack(k.At, k.Bt, k.qt, k.rt, k.dt, k.x0t);
  }
  int close() {
    if (!open_) return NDLQR_OK;
    open_ = false;
    const CostState& k = c->cost;
    const int err = pack(k.At, k.Bt, k.qt, k.rt, k.dt, k.x0t);
    c->flags = user_flags;
    c->kept.forget_factorisation();
    return err;
  }
};

#pragma GCC visibility push(hidden)
// hip_lin_polish.hip: mu [batch][N][p] of a polished resident solution into `out` (this device's memory) on `st` -- the
// polished mu of the problems the polish ended as 1, rho y of the others
hipError_t launch_lin_polish_multipliers(NdlqrHipCtx* c, double* out, hipStream_t st);
#pragma GCC visibility pop
