// lm_family.hip — one kernel family (LM_FAMILY) and part (LM_PART) of the step kernels; see lm_step.h.
// The library links one object per family and part (five parts per row of lm_families.h: 0-2 the kernel kinds' parts, 3 and 4 the policy
// kernels of the fused and of the replay kinds; parts 2-4 of the generic family hold nothing) so that `make -j`
// builds them in parallel.
#include "lm_step.h"

namespace lmk {
#define LM_CAT2(a, b, c, d) a##b##c##d
#define LM_CAT(a, b, c, d) LM_CAT2(a, b, c, d)

bool LM_CAT(launch_f, LM_FAMILY, p, LM_PART)(const LaunchCtx& L0, const KArgs& a, int kind) {
  constexpr Family F = family(LM_FAMILY);      // the family's row (lm_families.h): everything its kernels are compiled for
  static_assert(F.present, "LM_FAMILY is not a row of LM_FAMILY_LIST");
#if LM_PART >= 3
  // the POLICY instantiations of the fused and replay kinds (lm_step.h launch_family_policy); the generic family has no fused kernels
#if LM_FAMILY != LM_GENERIC_FAMILY
  return launch_family_policy<F.MC, F.NS, F.RK4, F.CONE, F.NM, LM_PART, F.PM>(L0, a, kind);
#else
  return false;
#endif
#elif LM_FAMILY != LM_GENERIC_FAMILY
  return launch_family<F.MC, F.NS, F.RK4, F.CONE, F.NM, LM_PART, F.PM>(L0, a, kind);
#elif LM_PART == 2
  return false;          // the generic family has no kernels with per-environment parameters
#else
  // generic fallbacks (cone read at run time, plain layout only); kind = LMK_FWD or LMK_REP1; `a.T.max_links`, the
  // integrator pick the instance. PART 0: Euler, PART 1: RK4
  LaunchCtx L = L0;
  L.stat_bytes = static_lds_bytes(0);      // (no muscles)
  const dim3 grid((L.N + L.epb - 1) / L.epb), block(4 * L.epb);
  const size_t groups = (block.x + 15) / 16;
  constexpr bool RK = LM_PART == 1;
  constexpr Family S = generic_instance(3, RK), B = generic_instance(5, RK);      // (lm_families.h: chains of up to three links | of up to five)
  const bool big = generic_instance(a.T.max_links, RK).MC == B.MC;
  if (kind == LMK_FWD) {
    if (!big) launch_one(step_kernel<S.MC, S.NS, RK, true, S.CONE>, grid, block, (size_t)lm::LaneMem<S.MC, S.NS>::kGroup * groups, L, a);
    else launch_one(step_kernel<B.MC, B.NS, RK, true, B.CONE>, grid, block, (size_t)lm::LaneMem<B.MC, B.NS>::kGroup * groups, L, a);
  } else if (kind == LMK_REP1) {
    if (!big) launch_term(step_kernel<S.MC, S.NS, RK, false, S.CONE>, step_kernel<S.MC, S.NS, RK, false, S.CONE, 0, 0, 1, false, 0, true>, grid, block, (size_t)lm::LaneMem<S.MC, S.NS>::kGroup * groups, L, a);
    else launch_term(step_kernel<B.MC, B.NS, RK, false, B.CONE>, step_kernel<B.MC, B.NS, RK, false, B.CONE, 0, 0, 1, false, 0, true>, grid, block, (size_t)lm::LaneMem<B.MC, B.NS>::kGroup * groups, L, a);
  } else return false;
  return true;
#endif
}

}  // namespace lmk
