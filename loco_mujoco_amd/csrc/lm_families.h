// lm_families.h — THE description of the kernel families (LM_FAMILY_LIST, pick_family) and kernel kinds (kKinds, pick_kind): read by
// lm_family.hip, lm_step.h and lm_kernels.hip. Plain C++17, no HIP. Family ids and kind numbers are ABI (lm_lds_bytes, include/locohip.h).
#pragma once
#include "../../include/lm_layout.h"

// A/B switches of the probe builds (tools/probes: `make EXTRA=-D...`): the defaults feed the table below
#ifndef LM_A1_NS
#define LM_A1_NS 6
#endif
#ifndef LM_A1_PAIRS
// 2: the pair pass WITHOUT the inlined convex collider in the regular kernels: a control step that brings a box / cylinder pair within
// reach is abandoned and run by the family's replay kernel (lm_step.h). Measured at the end of round 4, same box, two runs each
// (tools/probes/r4/ab_a1_variants.sh): 1.558 ms per control step of the bench rollout against 1.629 ms with the collider inlined (1):
// -4.4 % — the native box / cylinder colliders had taken the kernel's scratch from 608 to 896 bytes per lane. The bench rollout
// abandons no control step, a random policy two environments per launch (taken over by the pollers beside the launch). Other
// variants of the same A/B: max-ILP scheduler +3.0 %, iterative-minreg +9.0 %, -O2 +2.0 %, five slots +1.0 %.
#define LM_A1_PAIRS 2
#endif
#ifndef LM_SIX_PAIRS
// 1: the whole pair pass in the regular kernels (lane memory 32.8 KB + 9.4 KB of constants: THREE workgroups per CU — a batch of 4096
// runs its last quarter of workgroups behind the first finishers). 3: detection only (39.2 KB, four per CU; a self-contact hands the
// control step to the replay kernel): right for gaits — but robots that stumble under a random policy touch themselves in a quarter of
// their control steps, and 1100 replays per launch at one environment per workgroup cost 129 ms per step (measured, round 4).
#define LM_SIX_PAIRS 1
#endif
#ifndef LM_HESS_ENV_VOTE
// 1: in the kernels with elliptic contacts (the quadruped's and the generic ones; the pyramidal families compile the 6-wide code out) an
// environment takes ONE instantiation of the Hessian accumulation per Newton iteration — the 6-wide one as soon as one of its floor
// contacts with a Hessian block has condim > 3 (lm_core.h kHessEnvVote: same numbers either way). 0: every slot by its own condim, as before.
#define LM_HESS_ENV_VOTE 1
#endif
#ifndef LM_DPP_BCAST
// 1: in the four-replica kernels compiled for the elliptic cone (the quadruped's regular, fused and replay kernels) the exchanges
// between the replicas of an environment (the line search's four points, the floor pass's contact counts) and between the lanes of a
// quad (the pair pass) are DPP moves — row_newbcast, row_ror, quad_perm: VALU, no address arithmetic, no LDS wait — instead of
// ds_bpermute through the LDS crossbar (lm_step.h QuadDppT::kDppBcast, lm_core.h kDppBcast: same values either way). 0: ds_bpermute
// everywhere, as before. The sixteen-replica and the plain layout, the pyramidal families, the generic family and the forward-only
// kernels keep ds_bpermute (their objects do not change with the switch).
#define LM_DPP_BCAST 1
#endif
#ifndef LM_LS_FLOOR_SPLIT
// 1: in the kernels compiled for the elliptic cone with the pair pass (the quadruped's regular, fused and replay kernels) the line
// search visits the floor slots [0, nfloor) and the self-contact slots [nfloor, nslot) in loops of their own (lm_core.h kLsFloorSplit):
// a floor slot's weight is an opaque 1.0f (lm_step.h LM_OPAQUE_ONE) instead of the slot's pair code read from lane memory and taken
// apart — the same multiplies and the same sums in the same order, so the same numbers. 0: one loop over all slots, as before. Every
// other family and the forward-only kernels keep the one loop (their objects do not change with the switch).
#define LM_LS_FLOOR_SPLIT 1
#endif
// One row per family: X(id, MC, NS, RK4, CONE, NM, PM, flags) of struct Family. Ids 1 and 3 (four contact slots per chain) went in round 5.
// A family listed here and not in FAMILIES of csrc/Makefile, or the reverse, fails when the library is linked: no checker is needed.
#define LM_GENERIC_FAMILY 6
#define LM_FAMILY_LIST(X)                                                                                                          \
  X(0, 3, LM_A1_NS, false, LM_CONE_ELLIPTIC, 0, LM_A1_PAIRS, F_SPEC | F_PARAMS | F_NO_ACTIVE) /* quadruped: 2 + 2 + 1 floor contacts per leg + a self-contact */ \
  X(2, 5, 8, true, LM_CONE_PYRAMIDAL, 0, 0, F_SPEC | F_PARAMS)             /* five-link humanoids, RK4 (Atlas: two boxes per foot) */         \
  X(4, 5, 8, false, LM_CONE_PYRAMIDAL, 0, 0, F_SPEC | F_PARAMS)            /* five-link humanoids, Euler (Talos, the carry tasks) */          \
  X(5, 5, 4, false, LM_CONE_PYRAMIDAL, LM_MAXMUS, 0, F_SPEC | F_PARAMS)    /* muscle humanoid */                                              \
  X(6, 0, 0, false, -1, 0, 0, 0)                                           /* generic (lm_family.hip): run-time cone and chain length, plain layout; part 0 Euler, 1 RK4 */ \
  X(7, 6, 8, false, LM_CONE_PYRAMIDAL, 0, LM_SIX_PAIRS, F_SPEC | F_PARAMS) /* six-link chains: UnitreeG1, UnitreeH1 with its arms */          \
  X(8, 5, 8, true, LM_CONE_PYRAMIDAL, 0, 1, F_SPEC | F_PARAMS)             /* HumanoidTorque, bone hulls colliding (RK4) */                   \
  X(9, 5, 8, false, LM_CONE_PYRAMIDAL, 0, 1, F_SPEC | F_PARAMS)            /* UnitreeH1: cylinders and link meshes colliding (Euler) */       \
  X(10, 5, 8, false, LM_CONE_PYRAMIDAL, LM_MAXMUS, 1, F_SPEC | F_PARAMS)   /* HumanoidMuscle, bone hulls colliding */                         \
  X(11, 7, 8, true, LM_CONE_PYRAMIDAL, 0, 1, F_SPEC | F_PARAMS)            /* mesh-foot HumanoidTorque: seven-link legs, joint equality rows (RK4) */

namespace lmk {
// the task facts of a model that the step kernels take by value (lm_step.h KArgs::T; derived from the blob by lm_model_parse.h)
struct Task {
  int nv, nu, nobs, ngoal, nsub, reward_type, n_chains, max_links, na, ngrf, cm_used, max_contacts, all_pyr3, npair;
  float rp[8];
};
constexpr int LMK_NFAMILY = 12;
enum { F_SPEC = 1, F_PARAMS = 2, F_NO_ACTIVE = 4 };
struct Family {      // links and contact slots per chain, integrator, compiled-in cone, muscles per chain, pair pass of the regular kernels (0 none, 1 with the convex collider, 2 without, 3 detection only)
  bool present; int MC, NS; bool RK4; int CONE, NM, PM, flags;
  constexpr bool specialised() const { return flags & F_SPEC; }             // replicated layout, fused kernels and a replay kernel
  constexpr bool env_params() const { return flags & F_PARAMS; }            // lm_set_dof_params, lm_set_model_variants
  constexpr bool no_active_lists() const { return flags & F_NO_ACTIVE; }    // lm_batch_set_active is refused
  constexpr bool pairs() const { return PM != 0; }        // a pair pass: self-collision tables are simulated
  constexpr bool eq_rows() const { return MC >= 7; }      // joint equality rows (lm_core.h EQ_ROWS)
};
// the traits of family `id`; of no family (ids 1 and 3, -1: a model that no kernel is compiled for) all false
constexpr Family family(int id) {
  switch (id) {
#define LM_X(id, ...) case id: return Family{true, __VA_ARGS__};
    LM_FAMILY_LIST(LM_X)
#undef LM_X
  }
  return Family{};
}

// Which kernel family serves a model: the quadruped family gets a specialised step kernel <3 links, 6 slots, Euler, elliptic,
// self-collisions>; the humanoid families (five- and six-link chains) are compiled for condim-3 pyramids only (all_pyr3, checked when
// the model is created): the elliptic code compiles out and the contact slots are compact. Everything else: generic kernels, cone read
// at run time, plain layout only — and no muscles: a muscle model that no muscle family fits has no kernel. -1: no kernel is compiled
// for the model (lm_model_create refuses it with no_family_reason).
struct ModelFacts { int max_links, max_contacts, integrator, cone, na, npair; bool all_pyr3, root_xyz; };
constexpr int pick_family(const ModelFacts& m, bool generic_probe /* A/B: run-time cone for the humanoids */) {
  const bool big = m.max_links > 3, six = m.max_links > 5, rk4 = m.integrator == LM_INT_RK4, few = m.max_contacts <= 4;
  const bool pyr3 = m.all_pyr3 && !generic_probe;
  // seven-link chains (the mesh-foot humanoid): RK4, condim-3 pyramids, no muscles, the pair pass and the joint equality rows
  if (m.max_links > 6) return (rk4 && m.na == 0 && pyr3) ? 11 : -1;
  if (six) return (!rk4 && m.na == 0 && pyr3) ? 7 : -1;      // (with or without self-collision tables: its regular kernels detect, its replay kernel collides)
  // five-link humanoids whose lowering carries self-collision tables (bone hulls, link meshes, cylinders): the pair families
  if (big && m.npair > 0 && pyr3) return rk4 ? (m.na == 0 ? 8 : -1) : (m.na == 0 ? 9 : 10);
  // (the quadruped family's Hessian takes the root's translation columns as unit rows: lm_core.h ROOT_XYZ; another root -> generic kernels)
  if (!big && !rk4 && m.na == 0 && m.cone == LM_CONE_ELLIPTIC && m.root_xyz) return 0;
  if (big && rk4 && m.na == 0 && pyr3) return 2;
  if (big && !rk4 && m.na == 0 && pyr3) return 4;
  if (big && !rk4 && m.na > 0 && few && pyr3) return 5;
  return m.na > 0 ? -1 : LM_GENERIC_FAMILY;      // (the generic kernels are compiled without muscles: NM = 0 would step the robot with its muscles slack)
}
// why pick_family found no kernel for the model
constexpr const char* no_family_reason(const ModelFacts& m) {
  return m.max_links > 5 ? "no kernel is compiled for this model: chains of six links are compiled for Euler, of seven links for RK4 — condim-3 pyramids, no muscles only"
                         : "no kernel is compiled for this model: muscle models need five-link chains, the Euler integrator and condim-3 contacts under pyramidal cones "
                           "(the generic kernels that serve other cones and integrators have no muscles)";
}
// the instance of the generic family that serves a model (lm_family.hip): links and contact slots per chain by the longest chain, the
// integrator by the part; the cone is read at run time, no muscles, no pair pass, plain layout only
constexpr Family generic_instance(int max_links, bool rk4) { return max_links > 3 ? Family{true, 5, 8, rk4, -1, 0, 0, 0} : Family{true, 3, 4, rk4, -1, 0, 0, 0}; }

// ---- kernel kinds of one family (picked by the host, lm_kernels.hip::launch_variant)
enum { LMK_FWD = 0, LMK_REP4, LMK_REP1, LMK_DR_REP4, LMK_DR_REP1, LMK_FUSED, LMK_FUSED_DR, LMK_DRV_REP4, LMK_DRV_REP1, LMK_FUSED_DRV,
       LMK_BIG, LMK_BIG_DR, LMK_BIG_DRV /* the replay kernels, one per part */, LMK_NKINDS };
enum Layout { kRep4, kPlain, kReplay };      // replicated: 4 quads per environment, workgroups of <= 4 environments | plain | one environment per workgroup
// part: the object lm_family_f<k>p<part>.o that holds it; DR: 0 the model's joint parameters | 1 per-environment | 2 + model variants
struct Kind { int id; const char* name; int part, DR; Layout layout; bool fused; };
constexpr Kind kKinds[] = {
    {LMK_FWD, "forward", 0, 0, kPlain, false},           // (lm_forward_debug: run-time cone, any number of environments per workgroup)
    {LMK_REP4, "replicated", 0, 0, kRep4, false},
    {LMK_REP1, "plain", 0, 0, kPlain, false},
    {LMK_DR_REP4, "replicated, joint parameters", 1, 1, kRep4, false},
    {LMK_DR_REP1, "plain, joint parameters", 1, 1, kPlain, false},
    {LMK_FUSED, "fused", 1, 0, kRep4, true},
    {LMK_FUSED_DR, "fused, joint parameters", 1, 1, kRep4, true},
    {LMK_DRV_REP4, "replicated, model variants", 2, 2, kRep4, false},
    {LMK_DRV_REP1, "plain, model variants", 2, 2, kPlain, false},
    {LMK_FUSED_DRV, "fused, model variants", 2, 2, kRep4, true},
    {LMK_BIG, "replay", 0, 0, kReplay, true},
    {LMK_BIG_DR, "replay, joint parameters", 1, 1, kReplay, true},
    {LMK_BIG_DRV, "replay, model variants", 2, 2, kReplay, true}};
constexpr bool kinds_in_order(int k = 0) { return k == LMK_NKINDS || (kKinds[k].id == k && kKinds[k].part >= 0 && kKinds[k].part <= 2 && kinds_in_order(k + 1)); }
static_assert(sizeof(kKinds) / sizeof(kKinds[0]) == LMK_NKINDS && kinds_in_order(), "kKinds: one row per LMK_* kind in enum order, each in part 0, 1 or 2");

// the kind with joint parameters `dr` in `layout`, fused or not; pick_kind: the regular kernel of a launch (fused: replicated layout only)
constexpr int find_kind(int dr, Layout layout, bool fused, int k = LMK_FWD + 1) {
  return k == LMK_NKINDS ? -1 : (kKinds[k].DR == dr && kKinds[k].layout == layout && kKinds[k].fused == fused) ? k : find_kind(dr, layout, fused, k + 1);
}
constexpr int pick_kind(bool forward, bool fused, bool variants, bool dofprm, bool replicated) {
  return forward ? (int)LMK_FWD : find_kind(variants ? 2 : (dofprm ? 1 : 0), (fused || replicated) ? kRep4 : kPlain, fused);
}
// is kind `k` of family `f` launched at `epb` environments per workgroup
constexpr bool kind_runs_at(const Family& f, int k, int epb) {
  return k == LMK_FWD || kKinds[k].layout == kReplay || (kKinds[k].layout == kRep4 ? epb <= 4 : (epb > 4 || !f.specialised()));
}

}  // namespace lmk
