// lm_family.hip — one kernel family (LM_FAMILY) and part (LM_PART) of the step kernels; see lm_step.h.
// The library links one object per family and part (three parts per row of lm_families.h; part 2 of the generic family holds nothing) so that `make -j`
// builds them in parallel.
#include "lm_step.h"

namespace lmk {
#define LM_CAT2(a, b, c, d) a##b##c##d
#define LM_CAT(a, b, c, d) LM_CAT2(a, b, c, d)

bool LM_CAT(launch_f, LM_FAMILY, p, LM_PART)(const LaunchCtx& L0, const KArgs& a, int kind) {
  constexpr Family F = family(LM_FAMILY);      // the family's row (lm_families.h): everything its kernels are compiled for
  static_assert(F.present, "LM_FAMILY is not a row of LM_FAMILY_LIST");
#if LM_FAMILY != LM_GENERIC_FAMILY
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
  const bool big = a.T.max_links > 3;
  constexpr bool RK = LM_PART == 1;
  if (kind == LMK_FWD) {
    if (!big) launch_one(step_kernel<3, 4, RK, true, -1>, grid, block, (size_t)lm::LaneMem<3, 4>::kGroup * groups, L, a);
    else launch_one(step_kernel<5, 8, RK, true, -1>, grid, block, (size_t)lm::LaneMem<5, 8>::kGroup * groups, L, a);
  } else if (kind == LMK_REP1) {
    if (!big) launch_term(step_kernel<3, 4, RK, false, -1>, step_kernel<3, 4, RK, false, -1, 0, 0, 1, false, 0, true>, grid, block, (size_t)lm::LaneMem<3, 4>::kGroup * groups, L, a);
    else launch_term(step_kernel<5, 8, RK, false, -1>, step_kernel<5, 8, RK, false, -1, 0, 0, 1, false, 0, true>, grid, block, (size_t)lm::LaneMem<5, 8>::kGroup * groups, L, a);
  } else return false;
  return true;
#endif
}

}  // namespace lmk
