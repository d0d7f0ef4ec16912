// lm_kernels.hip — the C-ABI (include/locohip.h) of the batched LocoEnv.step(): models, batches, state transfer and the
// launches of the step kernels. The kernels themselves live in lm_step.h / lm_core.h and are compiled per family in
// lm_family.hip (one object per family and part, so the library builds in parallel).
#include "lm_step.h"
#include "lm_compile.h"
#include "lm_snapshot.h"
#include "lm_state_io.h"
#include "../../include/locostate.h"
#include "lm_model_parse.h"
#include "lm_policy.h"
#include <memory>

using lmk::KArgs; using lmk::Task; using lmk::DevStats; using lmk::LaunchCtx;

namespace {
thread_local std::string g_err;
thread_local const char* g_launch_err = nullptr;
thread_local std::string g_layout_err;
int fail(const std::string& m) { g_err = m; return 1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

}  // namespace

// ================================================================================================================
// C-ABI
// ================================================================================================================
struct lm_model {
  int device;
  // the tables of lm_model_parse.h ParsedModel on the device: constant, geom, muscle (models with muscles), geom-pair, hull vertices, their
  // neighbour lists, body pairs, adjacency blocks of the hull vertices; n_gpt_floats: size of the geom-pair table (0: no self-collision pairs)
  float *d_cm, *d_gt, *d_mt, *d_gpt, *d_meshv, *d_meshn, *d_bpt, *d_meshadj; int n_gpt_floats;
  std::vector<float> nominal;  // [3][nv] damping | stiffness | frictionloss of the model
  int *d_qobs, *d_vobs;        // [nv] observation column of qpos[d] / qvel[d], -1: not observed (lm_model_parse.h; read by lm_state_io.h)
  lm::Params P; Task T;
  int family;                // the kernel family that serves the model (lm_families.h pick_family; -1: none is compiled for it)
  bool root_limited;         // a root dof with an active-able limit (lm_batch_set_replay)
  size_t lds_limit;          // LDS of one CU in bytes: what the runtime reports, or kLdsAssumed where it reports the 64 KB default only
  bool lds_reported;         // true: lds_limit is the runtime's figure
};

struct lm_batch {
  lm_model* m;
  int N;
  float *qpos, *qvel, *warm, *goal, *action, *obs, *reward, *table;
  float* act;                // muscle activations [na][N]
  float* dofprm;             // per-environment joint parameters [3][nv][N] (allocated by lm_set_dof_params)
  float* drspec;             // redraw rules [3][nv][3] (lm_set_dof_randomization)
  unsigned char* done;
  unsigned char* flags;      // validity flags of the last control step per environment (lm_get_flags)
  int* ep_step; unsigned* ep_count;
  DevStats* stats;
  int table_rows; unsigned long long seed; long long env_offset; int auto_reset, horizon; unsigned step_index;
  int epb, nblocks;
  int lds_ok[2];             // environments per workgroup at which the LDS of the step kernels [0] / the forward kernel [1] was found to fit (0: not checked yet)
  unsigned long long* timers;
  unsigned long long* tline;     // LM_TIMERS builds: time line of the last launch (lm_step.h KArgs::tline)
  hipStream_t stream;
  lm_stats acc;            // host-side accumulation (double)
  hipEvent_t ev0, ev1;
  hipEvent_t ev_ext;       // orders the library's stream behind a launch on a caller's stream (lm_step_device)
  float *vrec, *vgt, *vgpt; int* var; int nvar, gpt_floats, var_rows; bool dofprm_of_variants;   // model variants (lm_set_model_variants, lm_set_variant_rows)
  // the model compiler on the device (lm_set_model_compiler, lm_compile.hip): its program, per environment the restart flag, the draw
  // counter and the values drawn; the variant tables above then hold ONE slot per environment
  int* mc_ib; double* mc_db; int mc_ndraw; unsigned char *vdirty, *mc_mask; unsigned* vgen; double* vdraws; unsigned long long mc_seed;
  float* scr; int* scr_idx; size_t scr_cap;   // staging for masked uploads (rows of the masked environments only)
  // speculate / replay (lm_step.h): list of the environments whose control step left the regular kernel's capacity, its control
  // words, the fused step at which each left; `replay` = 0 switches the mechanism off (contacts beyond the slots are then dropped)
  int *replay_list, *replay_ctl, *stall; int replay;
  int* premark;                              // prediction (lm_step.h KArgs::premark): environments that start their next control step in the replay kernel
  float *hq, *hv, *hw; int* hsub;            // resume (lm_step.h KArgs::hq): substep-start states of the control steps that leave the regular kernel
  unsigned char* replay_mark;
  // the replay kernel's pollers run beside the regular launch on `stream2`, forked from / joined into the launch stream with the two
  // events; `h_hint` (pinned) receives the number of abandoned control steps of a completed launch: how many pollers the next one gets
  int stat_pre_off, nstat; int* h_hint; int hint, hint_seen; int epoch;
  hipStream_t stream2; hipEvent_t ev_fork, ev_join, ev_done[2];
  float* slack;              // detection slack + speed memory of the self-collision pass, [3][4][N] (lm_step.h KArgs::slack)
  // the float64 host surface (lm_step_pinned): pinned action staging, the pinned ring of result sets [obs f64 | reward f64 | done]
  float* h_act; unsigned char* h_out64[LM_PINNED_SLOTS]; int* d_perm; size_t out64_bytes;
  int* env_map; int n_active;    // active list (lm_batch_set_active): device copy of the environment ids, their number (N: all)
  float* mprc; int mprc_pairs;   // warm-start cache of the convex collider, [N][mprc_pairs][lm::kMprCacheFloats] (lm_step.h KArgs::mprc), or null
  // terminal observations (lm_set_terminal_obs, lm_step.h KArgs::term_obs): the buffer the kernels write (null: off), the one the batch
  // owns (null with a caller's buffer), and the fourth array of every pinned result set, [N][nobs] float64 (lm_pinned_terminal_obs)
  float *term_obs, *term_own; double* h_term64[LM_PINNED_SLOTS];
  // policy rollouts (lm_rollout_policy, lm_step.h KArgs::pol): the lanes' hand-over rows [N][2 * lmp::kPolicyMaxWidth] and, for batches
  // that collect no terminal observations, the sink [N][nobs] the policy kernels' terminal store writes to (they are compiled with
  // that store only). Scratch of a launch, allocated by the first policy call: nothing of it is state, nothing enters a snapshot
  float *pol_hand, *pol_sink;
  // the policy's input normalisation (lm_set_policy_obs_norm): the caller's device tensors, read in place by every policy evaluation; mean
  // null: off. A setting like the terminal-observation buffer: not state, not in a snapshot
  lmp::PolicyNorm pol_norm;
  // every device or pinned array above that the batch owns: its field's address, entered by batch_array where the array is allocated.
  // lm_batch_destroy releases what these fields hold at that moment and names none of them
  struct Owned { void** field; bool pinned; };
  std::vector<Owned> owned;
};
namespace lmp {
// policy_row for every (active) environment: 4 environments per wave-sized workgroup, 16 lanes each. Used in front of every control
// step that runs as a launch of its own; the step kernel then reads the action row in action_mode 0, on the same stream.
struct PolicyArgs {
  lm_mlp_policy p;
  PolicyNorm norm;           // the input normalisation (lm_set_policy_obs_norm; mean null: off)
  const float* obs;          // [N][nobs]: the observation the action is computed from
  float* act;                // [N][nu]: this control step's row of the action tape
  const int* env_map; int n_active;      // the active list (lm_step.h KArgs): slot -> environment, or null
  unsigned long long noise_seed; long long env_offset; unsigned step_index;
};

__global__ __launch_bounds__(64) void policy_kernel(PolicyArgs a) {
  __shared__ float hand[4][2 * kPolicyMaxWidth];
  const int lane = threadIdx.x & 15, e_local = threadIdx.x >> 4;
  const int slot = blockIdx.x * 4 + e_local;
  if (slot >= a.n_active) return;           // (nothing below joins the whole workgroup)
  const int e = a.env_map ? a.env_map[slot] : slot;
  const int nobs = a.p.sizes[0], nu = a.p.sizes[a.p.n_layers];
  policy_row(a.p, a.norm, a.obs + (long long)e * nobs, a.act + (long long)e * nu, hand[e_local], lane, a.noise_seed, a.env_offset + e, a.step_index);
}

static void launch_policy(const PolicyArgs& a, hipStream_t stream) {
  if (a.n_active <= 0) return;
  hipLaunchKernelGGL(policy_kernel, dim3((a.n_active + 3) / 4), dim3(64), 0, stream, a);
}
}  // namespace lmp

// A/B switches of the probe builds (tools/probes: `make EXTRA=-DLM_PROBES ...`). The shipped library reads NO environment variable:
// tests/test_abi_exports.py checks that `getenv` is not among its undefined symbols.
#ifdef LM_PROBES
#define LM_PROBE_ENV(name) getenv(name)
#else
#define LM_PROBE_ENV(name) ((const char*)nullptr)
#endif

static lmk::Family traits(const lm_batch* b) { return lmk::family(b->m->family); }      // (lm_families.h; of a model without a family: all false)
static bool one_layout_only(const lm_batch* b) { return b->m->family >= 0 && !traits(b).specialised(); }

static bool replicas_off() { static const bool off = LM_PROBE_ENV("LM_NO_REPLICAS") != nullptr; return off; }      // A/B switch

constexpr size_t kLdsAssumed = 160 * 1024;      // LDS of a gfx950 CU (lm_core.h: LaneMem)

// a device allocation that lives for one call: released on every return path
struct HipFree { void operator()(void* p) const { (void)hipFree(p); } };
template <class T> using dev_temp = std::unique_ptr<T, HipFree>;
template <class T> static int dev_temp_alloc(dev_temp<T>* out, size_t count) {
  T* p = nullptr;
  HIPCHK(hipMalloc(&p, sizeof(T) * count));
  out->reset(p);
  return 0;
}

// THE allocation of a batch's array: `count` zeroed elements on the device (or in pinned host memory) behind `*field`. What the field
// held before is released first (arrays that are replaced: the reset table, the variant tables, the staging rows ...); the field is
// entered into b->owned, so nothing else has to remember it
static void batch_release(void** field, bool pinned) {
  if (*field) (void)(pinned ? hipHostFree(*field) : hipFree(*field));
  *field = nullptr;
}
template <class T> static void batch_release(T** field) { batch_release((void**)field, false); }
template <class T> static int batch_array(lm_batch* b, T** field, size_t count, bool pinned = false) {
  void** f = (void**)field;
  batch_release(f, pinned);
  bool known = false;
  for (const lm_batch::Owned& o : b->owned) known = known || o.field == f;
  if (!known) b->owned.push_back({f, pinned});
  const size_t bytes = sizeof(T) * (count ? count : 1);
  if (pinned) { HIPCHK(hipHostMalloc(f, bytes, hipHostMallocDefault)); memset(*f, 0, bytes); }
  else { HIPCHK(hipMalloc(f, bytes)); HIPCHK(hipMemset(*f, 0, bytes)); }
  return 0;
}

// the launch functions of the lm_family.hip objects, [family][part]: from the one list of families (absent ids: null)
static lmk::family_fn kFamilyTable[lmk::LMK_NFAMILY][5];
#define LM_X(id, ...) kFamilyTable[id][0] = lmk::launch_f##id##p0; kFamilyTable[id][1] = lmk::launch_f##id##p1; kFamilyTable[id][2] = lmk::launch_f##id##p2; \
  kFamilyTable[id][3] = lmk::launch_f##id##p3; kFamilyTable[id][4] = lmk::launch_f##id##p4;
static const bool kFamilyTableFilled = [] { LM_FAMILY_LIST(LM_X) return true; }();
#undef LM_X

// The LDS a launch of `kind` (lm_step.h LMK_*) of family `fam` takes at `epb` environments per workgroup for a model whose constant table
// uses `cm_used` floats: asked of the launch code itself (LaunchCtx::probe — nothing is launched, no device is touched). false: the
// family has no kernel of that kind.
static bool lds_of(int fam, int kind, int epb, int cm_used, int max_links, lmk::LdsUse* out) {
  if (!lmk::family(fam).present || kind < 0 || kind >= lmk::LMK_NKINDS || epb < 1) return false;      // (whether it has the kind: the object answers)
  KArgs a; memset(&a, 0, sizeof(a));
  a.T.cm_used = cm_used; a.T.max_links = max_links; a.epb = epb; a.N = epb;
  lmk::LdsUse u = {0, 0}; const LaunchCtx L = {nullptr, epb, epb, 0, nullptr, &u, 0};
  const bool has = kFamilyTable[fam][lmk::kKinds[kind].part](L, a, kind);
  if (has) *out = u;
  return has;
}

// Why the batch cannot step at `epb` environments per workgroup: the first kernel of that layout — regular, per-environment parameters,
// model variants, fused, replay — whose static + dynamic LDS a CU cannot hold, with the byte counts; empty: all fit. `fwd`: the same
// question for lm_forward_debug's kernel alone (run-time cone, full slot records: at 16 per workgroup it does not fit for most humanoid
// models whose step kernels do, so lm_forward_debug is refused at its own call and not with the layout).
static std::string layout_refusal(const lm_batch* b, int epb, bool fwd) {
  const int fam = b->m->family;
  if (fam < 0) return "";
  for (int kind = 0; kind < lmk::LMK_NKINDS; kind++) {
    if ((kind == lmk::LMK_FWD) != fwd || !lmk::kind_runs_at(traits(b), kind, epb)) continue;
    lmk::LdsUse u;
    if (!lds_of(fam, kind, epb, b->m->T.cm_used, b->m->T.max_links, &u)) continue;
    if (u.stat + u.dyn > b->m->lds_limit) {
      char why[400];
      snprintf(why, sizeof(why), "%d environments per workgroup: the %s kernel of family %d needs %zu B of LDS per workgroup (%zu B static + %zu B dynamic, "
               "%d B of it this model's constant table), a compute unit has %zu B (%s)", epb, lmk::kKinds[kind].name, fam, u.stat + u.dyn, u.stat, u.dyn,
               (int)sizeof(float) * b->m->T.cm_used, b->m->lds_limit, b->m->lds_reported ? "reported by the runtime" : "assumed: the runtime reports the 64 KB default only");
      return why;
    }
  }
  return "";
}

// (Round 5, tried and dropped: a one-workgroup GATE kernel in front of the regular launch that waits until the launch's pollers are
// resident, and a higher priority for their stream. Launched first on their own stream the pollers lose the race for the chip in 7
// launches of 10 and start when the first regular workgroups retire, 4.4 ms into a HumanoidTorque launch; with the gate they are
// resident at once — and every poller then keeps one regular workgroup waiting for those 4.4 ms instead (the kernels' 512 registers
// allow one wave per SIMD, and 4096 environments are exactly one wave per SIMD): the step time is the same, 16.0 ms either way.
// profiles/r5_notes.md §4.)
template <bool FWD>
static void launch_variant(lm_batch* b, const KArgs& a, hipStream_t stream) {
  const int fam = b->m->family;
  if (fam < 0) { g_launch_err = "no kernel is compiled for this model"; return; }      // (lm_model_create refuses such a model: not reached)
  const LaunchCtx L = {stream, b->n_active, b->epb, b->m->lds_limit, &g_launch_err, nullptr, 0};
  if (b->n_active <= 0) return;            // an empty active list: nothing to run
  if (b->lds_ok[FWD] != b->epb) {          // (lm_batch_set_layout refuses such a layout; a model's default layout and the forward kernel are checked here, once)
    g_layout_err = layout_refusal(b, b->epb, FWD);
    if (!g_layout_err.empty()) { g_launch_err = g_layout_err.c_str(); return; }
    b->lds_ok[FWD] = b->epb;
  }
  if (!traits(b).specialised()) {
    if (b->dofprm) { g_launch_err = "per-environment joint parameters are not compiled for this model family"; return; }
    kFamilyTable[fam][b->m->P.integrator == LM_INT_RK4 ? 1 : 0](L, a, FWD ? lmk::LMK_FWD : lmk::LMK_REP1);      // (its parts: Euler | RK4)
    return;
  }
  const int kind = lmk::pick_kind(FWD, a.nfused > 1, b->nvar > 0, b->dofprm != nullptr, b->epb <= 4 && !replicas_off());
  const int big = lmk::find_kind(b->nvar > 0 ? 2 : (b->dofprm ? 1 : 0), lmk::kReplay, true);
  // (a policy launch, KArgs::pol: the same kinds from the parts that hold their POLICY instantiations, lm_step.h launch_family_policy)
  const bool policy = a.pol.d_params != nullptr;
  const lmk::family_fn launch = kFamilyTable[fam][policy ? 3 : lmk::kKinds[kind].part], launch_big = kFamilyTable[fam][policy ? 4 : lmk::kKinds[big].part];
  KArgs r = a;
  r.reg_grid = (b->n_active + b->epb - 1) / b->epb; r.epoch = b->epoch; r.host_hint = b->h_hint;
  const bool replay = !FWD && a.replay_list;
  bool pollers = false;
  if (replay) {
    // How many control steps did recent launches abandon? (h_hint: pinned host memory, written by the drain pass of a launch that
    // has completed by now — a hint, read without waiting for anything.) Launches that abandon some get pollers: replay workgroups on the second stream, launched
    // BEFORE the regular kernel, that take the abandoned environments over while the launch is still running (lm_step.h). A batch
    // whose robots stay inside the regular kernel (the quadruped's bench rollout) launches none.
    // (a rollout queues hundreds of launches before the first has run: no news = no change; news = the latest count, decaying slowly)
    const int last = b->h_hint[0], seen = b->h_hint[1];
    if (seen != b->hint_seen) { b->hint_seen = seen; b->hint = last > b->hint ? last : (b->hint > 0 ? b->hint - 1 : 0); }
    // how many: the abandoned steps of a launch scatter around the recent count like a Poisson variable (HumanoidTorque.run: 12.6 +- 3.5
    // per launch) — an entry without a poller of its own waits for one to finish a whole hard control step. pollers = kPollMul x
    // recent count + kPollAdd, at most kPollCap (round 5: profiles/r5_notes.md §4)
    static int poll_mul = lmk::kPollMul, poll_add = lmk::kPollAdd, poll_cap = lmk::kPollCap;
    static const bool poll_env = [] { if (const char* v = LM_PROBE_ENV("LM_POLLERS")) sscanf(v, "%d,%d,%d", &poll_mul, &poll_add, &poll_cap); return true; }();
    (void)poll_env;
    int want = a.replay_all ? lmk::kReplayGrid : (b->hint > 0 ? (poll_mul * b->hint) / 2 + poll_add : 0);
    if (want > poll_cap && !a.replay_all) want = poll_cap;
    if (want > lmk::kReplayGrid) want = lmk::kReplayGrid;
    if (b->replay >= 3) want = 0;
    if (b->h_hint[2] > 0) want = 0;        // a poller timed out once: they do not overlap with the regular kernel here (serialised kernels) — drain pass only from now on
    if (want > 0) {
      KArgs p = r;
      p.drain = 0; p.stats_off = b->stat_pre_off;
      // not further ahead than one launch: the pollers start once the launch BEFORE the previous one is complete (they are then resident
      // while the previous launch tails off and wait for its drain pass on the device). Without this a host that queues hundreds of
      // launches ahead of the device would start them long before their launch: they would wait out their time-out and leave
      if (b->epoch >= 2 && hipStreamWaitEvent(b->stream2, b->ev_done[b->epoch & 1], 0) != hipSuccess) { g_launch_err = "stream wait failed"; return; }
      const LaunchCtx L2 = {b->stream2, b->N, want, b->m->lds_limit, &g_launch_err, nullptr, 0};
      if (!launch_big(L2, p, big)) { g_launch_err = "no replay kernel in the family"; return; }
      if (g_launch_err) return;              // (launch_one refused: nothing is in flight)
      if (hipEventRecord(b->ev_join, b->stream2) != hipSuccess) { g_launch_err = "stream join failed"; return; }
      pollers = true;

    }
  }
  // A failure from here on leaves pollers in flight that wait for a regular launch which will not come: they give up after their
  // time-out. Wait for them, and put the control words back to "no launch in progress" (the epoch did not advance: nothing drained),
  // so that the batch can be launched again or destroyed safely.
  auto bail = [&](const char* msg) {
    g_launch_err = msg;
    if (pollers) {
      (void)hipStreamSynchronize(b->stream2);
      (void)hipStreamSynchronize(stream);
      (void)hipMemset(b->replay_ctl, 0, sizeof(int) * 4);
    }
  };
  if (!launch(L, r, kind)) { bail("no kernel of this kind in the family"); return; }
  if (g_launch_err) { bail(g_launch_err); return; }
  if (replay) {
    // the drain pass, behind the regular launch AND the pollers: whatever is still listed; resets the control words. An empty
    // list costs a few microseconds (its workgroups read a word and leave)
    if (pollers && hipStreamWaitEvent(stream, b->ev_join, 0) != hipSuccess) { bail("stream join failed"); return; }
    r.drain = 1; r.stats_off = 0;
    const LaunchCtx L3 = {stream, b->N, lmk::kReplayGrid, b->m->lds_limit, &g_launch_err, nullptr, 0};
    if (!launch_big(L3, r, big)) { bail("no replay kernel in the family"); return; }
    if (g_launch_err) { bail(g_launch_err); return; }
    if (hipEventRecord(b->ev_done[b->epoch & 1], stream) != hipSuccess) { bail("event record failed"); return; }
    b->epoch++;
  }
}

extern "C" {

const char* lm_last_error(void) { return g_err.c_str(); }

int lm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void lm_model_destroy(lm_model* m);

static int upload(const std::vector<float>& v, float** dev) {
  HIPCHK(hipMalloc(dev, sizeof(float) * v.size()));
  HIPCHK(hipMemcpy(*dev, v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice));
  return 0;
}

int lm_model_create(const double* cmod, size_t n, int device, lm_model** out) {
  lmp::ParsedModel pm; std::string why;
  if (!lmp::parse_model(cmod, n, &pm, &why)) return fail(why);      // (every check of the blob: lm_model_parse.h)
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<lm_model, void (*)(lm_model*)> guard(new lm_model(), lm_model_destroy);      // freed on every error path
  lm_model* m = guard.get(); m->device = device;
  // the LDS one workgroup may take. A runtime that reports no more than the 64 KB every launch gets without opting in says nothing
  // about the CU: then the 160 KB of a CDNA4 CU that lm_core.h's LaneMem budgets with
  int per_block = 0;
  if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) per_block = 0;
  m->lds_reported = per_block > 64 * 1024;
  m->lds_limit = m->lds_reported ? (size_t)per_block : kLdsAssumed;
  if (LM_PROBE_ENV("LM_NO_PAIRS")) for (int c = 0; c < LM_NCHAIN; c++) pm.cm[LM_CM_CHAINS + LM_C_NLPAIR * LM_NCHAIN + c] = 0.0f;      // A/B: self-collision broad phase off
  m->T = pm.T; m->root_limited = pm.root_limited; m->n_gpt_floats = pm.n_gpt_floats; m->nominal = std::move(pm.nominal);
  static const bool generic = LM_PROBE_ENV("LM_GENERIC_KERNELS") != nullptr;      // A/B: run-time cone for the humanoids
  const lmk::ModelFacts facts = {pm.T.max_links, pm.T.max_contacts, pm.integrator, pm.cone, pm.T.na, pm.T.npair, pm.T.all_pyr3 != 0, pm.root_xyz};
  m->family = lmk::pick_family(facts, generic);
  if (m->family < 0) return fail(lmk::no_family_reason(facts));      // refused HERE, not at the first launch
  for (auto [host, dev] : {std::make_pair(&pm.qobs, &m->d_qobs), std::make_pair(&pm.vobs, &m->d_vobs)}) {
    HIPCHK(hipMalloc(dev, sizeof(int) * (host->size() ? host->size() : 1)));
    HIPCHK(hipMemcpy(*dev, host->data(), sizeof(int) * host->size(), hipMemcpyHostToDevice));
  }
  if (upload(pm.cm, &m->d_cm) || upload(pm.gt, &m->d_gt) || (!pm.mt.empty() && upload(pm.mt, &m->d_mt)) || upload(pm.gpt, &m->d_gpt) ||
      upload(pm.meshv, &m->d_meshv) || upload(pm.meshn, &m->d_meshn) || upload(pm.bpt, &m->d_bpt) || upload(pm.meshadj, &m->d_meshadj)) return 1;
  lm::Params& P = m->P;
  P.h = pm.h; P.g = lm::V3{pm.g[0], pm.g[1], pm.g[2]}; P.iterations = pm.iterations; P.scale = pm.scale; P.nv = pm.T.nv;
  P.tolerance = 1e-6f;      // float32 stand-in for MuJoCo's 1e-8 (the gradient itself carries ~1e-6 relative noise)
  P.integrator = pm.integrator; P.cone = pm.cone; P.act_position = pm.act_position; P.off_runsup = pm.off_runsup; P.neq = pm.neq; P.off_eq = pm.off_eq;
  P.gt = m->d_gt; P.cmg = m->d_cm; P.gpt = m->d_gpt; P.meshv = m->d_meshv; P.meshn = m->d_meshn; P.bpt = m->d_bpt; P.meshadj = m->d_meshadj;
  P.ls_tol = 1e-2f; P.ls_iters = 12; P.ls_noise = 2e-6f; P.ablate = 0;
  P.root_limited = pm.root_limited ? 1 : 0; P.root_xyz = pm.root_xyz ? 1 : 0;
  P.ls_grid[0] = 0.25f; P.ls_grid[1] = 0.0625f; P.ls_grid[2] = 0.015625f;
  if (const char* v = LM_PROBE_ENV("LM_LS_GRID")) sscanf(v, "%f,%f,%f", &P.ls_grid[0], &P.ls_grid[1], &P.ls_grid[2]);   // A/B knob
  if (const char* v = LM_PROBE_ENV("LM_LS_NOISE")) P.ls_noise = (float)atof(v);
  if (const char* v = LM_PROBE_ENV("LM_ABLATE")) P.ablate = atoi(v);
  if (const char* v = LM_PROBE_ENV("LM_TOLERANCE")) P.tolerance = (float)atof(v);          // tuning knobs for A/B probes
  if (const char* v = LM_PROBE_ENV("LM_LS_TOL")) P.ls_tol = (float)atof(v);
  if (const char* v = LM_PROBE_ENV("LM_LS_ITERS")) P.ls_iters = atoi(v);
  *out = guard.release();
  return 0;
}

void lm_model_destroy(lm_model* m) {
  if (!m) return;
  for (float* p : {m->d_cm, m->d_gt, m->d_gpt, m->d_meshv, m->d_meshn, m->d_bpt, m->d_meshadj, m->d_mt}) if (p) (void)hipFree(p);
  for (int* p : {m->d_qobs, m->d_vobs}) if (p) (void)hipFree(p);
  delete m;
}

int lm_model_dims(const lm_model* m, lm_dims* out) {
  out->nq = m->T.nv; out->nv = m->T.nv; out->nu = m->T.nu; out->nobs = m->T.nobs; out->ngoal = m->T.ngoal;
  out->n_substeps = m->T.nsub; out->n_chains = m->T.n_chains; out->max_chain_dofs = m->T.max_links; out->na = m->T.na;
  return 0;
}

void lm_batch_destroy(lm_batch* b);

static int batch_alloc(lm_batch* b) {
  lm_model* m = b->m;
  const int N = b->N, nv = m->T.nv;
  const size_t nvN = (size_t)nv * N;
  b->stat_pre_off = b->nblocks; b->nstat = b->nblocks + lmk::kReplayGrid;      // the concurrent replay kernel adds into slots of its own
  if (batch_array(b, &b->qpos, nvN) || batch_array(b, &b->qvel, nvN) || batch_array(b, &b->warm, nvN) || batch_array(b, &b->goal, (size_t)4 * N) ||
      batch_array(b, &b->action, (size_t)m->T.nu * N) || batch_array(b, &b->obs, (size_t)m->T.nobs * N) || batch_array(b, &b->reward, N) ||
      batch_array(b, &b->done, N) || batch_array(b, &b->flags, N) || batch_array(b, &b->ep_step, N) || batch_array(b, &b->ep_count, N) ||
      (m->T.na > 0 && batch_array(b, &b->act, (size_t)m->T.na * N)) || batch_array(b, &b->stats, b->nstat) ||
      batch_array(b, &b->replay_list, N) || batch_array(b, &b->stall, N) || batch_array(b, &b->replay_ctl, 8) || batch_array(b, &b->replay_mark, N) ||
      batch_array(b, &b->hq, nvN) || batch_array(b, &b->hv, nvN) || batch_array(b, &b->hw, nvN) || batch_array(b, &b->hsub, N) ||
      batch_array(b, &b->premark, N) || batch_array(b, &b->slack, (size_t)12 * N) ||
      batch_array(b, &b->timers, 32 + 32 * (size_t)b->nblocks)) return 1;
#ifdef LM_TIMERS
  if (batch_array(b, &b->tline, 4 * (size_t)N + 2 * (size_t)b->nblocks)) return 1;
#endif
  HIPCHK(hipHostMalloc((void**)&b->h_hint, sizeof(int) * 4, hipHostMallocDefault)); b->h_hint[0] = 0; b->h_hint[1] = 0; b->h_hint[2] = 0; b->h_hint[3] = 0;
  // the convex collider's warm-start cache: one record per environment and geom-pair record of the models whose hull pairs run through
  // it in kernels with five or more links per chain (128 B each: HumanoidTorque 692 pairs -> 88 KB per environment, 363 MB at 4096)
  if (m->d_meshadj && m->n_gpt_floats > 0 && m->T.max_links > 3) {
    b->mprc_pairs = m->n_gpt_floats / LM_GPAIR_SIZE;
    if (batch_array(b, &b->mprc, lm::kMprCacheFloats * (size_t)b->mprc_pairs * (size_t)N)) return 1;
  }
  HIPCHK(hipStreamCreate(&b->stream)); HIPCHK(hipStreamCreate(&b->stream2));
  HIPCHK(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&b->ev_done[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&b->ev_done[1], hipEventDisableTiming));
  HIPCHK(hipEventCreate(&b->ev0)); HIPCHK(hipEventCreate(&b->ev1)); HIPCHK(hipEventCreateWithFlags(&b->ev_ext, hipEventDisableTiming));
  return 0;
}

int lm_batch_create(lm_model* m, int n_envs, lm_batch** out) {
  if (n_envs <= 0) return fail("n_envs must be positive");
  HIPCHK(hipSetDevice(m->device));
  lm_batch* b = new lm_batch();      // (value-initialised: every field starts as zero)
  b->m = m; b->N = n_envs; b->n_active = n_envs;
  // Four environments per workgroup: with the replicated layout that is one full wave (4 envs x 4 replicas x 4 chains).
  // Larger batches simply run more workgroups back to back (wider workgroups without replicas were 30-50 % slower at
  // every size, profiles/r1_ab_probes.md); lm_batch_set_layout selects the plain layout.
  {
    int epb = n_envs < 4 ? n_envs : 4;
    const char* ov = LM_PROBE_ENV("LM_ENVS_PER_BLOCK");
    if (ov && atoi(ov) >= 1 && atoi(ov) <= 16) epb = atoi(ov);
    b->epb = epb;
  }
  b->nblocks = (n_envs + b->epb - 1) / b->epb;
  b->replay = 1;
  {
    // a model with self-collision tables needs a kernel family with the pair pass: anything else would silently not simulate them
    if (m->T.npair > 0 && !traits(b).pairs()) {
      delete b;
      return fail("the model carries self-collision tables but its kernel family has no pair pass (RK4 with muscles, or a cone / condim the pair families are not compiled for)");
    }
    // the same for joint equality rows: compiled into the seven-link family only (lm_core.h EQ_ROWS)
    if (m->P.neq > 0 && !traits(b).eq_rows()) {
      delete b;
      return fail("the model carries joint equality rows but its kernel family has none (they are compiled into the seven-link family only)");
    }
  }
  if (batch_alloc(b)) { lm_batch_destroy(b); return 1; }     // g_err holds the failed call; nothing leaks
  *out = b;
  return 0;
}

/* speculate / replay (lm_step.h): on (default) = a control step that needs more contact slots, longer pair lists or — the
   quadruped — the convex collider is replayed by the family's big kernel instead of dropping contacts; off = the regular kernels
   alone (contacts beyond the slots are dropped and counted: the behaviour of rounds 1-3, kept for A/B measurements). */
int lm_batch_set_replay(lm_batch* b, int enabled) {
  if (!b) return fail("null batch");
  // 2 (tests): every control step goes through the replay kernel; 3 / 4 = 1 / 2 without pollers: the replay kernel only as the pass
  // behind the regular launch (profilers that run one kernel at a time would leave the pollers waiting for their time-out)
  if (!enabled && b->m->T.na == 0 && traits(b).specialised()) {
    // the regular kernels of the families without muscles have no limit rows for the root dofs: without the replay kernel a root dof
    // beyond its range would run without its row (flagged per step, but wrong physics) — refuse rather than offer that
    if (b->m->root_limited) return fail("this model has a limited root joint whose limit rows live in the replay kernel: replay cannot be switched off");
  }
  b->replay = (enabled >= 2 && enabled <= 4) ? enabled : (enabled ? 1 : 0);
  return 0;
}

/* launch geometry: environments per workgroup. 4 (the default) = the replicated layout, one wave = 4 environments x 4 replicas x 4
   chains; 8 or 16 = the plain layout, a workgroup of 8 / 16 quads without replicas (the only other layout the families are compiled
   for; slower at every batch size measured, profiles/r1_ab_probes.md, kept for very large batches and as a cross-check of the
   replicas' protocol). Statistics slots were allocated for the default: only coarser geometries are accepted. */
int lm_batch_set_layout(lm_batch* b, int envs_per_workgroup) {
  if (!b) return fail("null batch");
  const int def = b->N < 4 ? b->N : 4;
  if (envs_per_workgroup == 4) envs_per_workgroup = def;      // the advertised default, also for a batch of fewer than four environments
  if (envs_per_workgroup != def && envs_per_workgroup != 8 && envs_per_workgroup != 16) return fail("environments per workgroup: 4 (replicated layout), 8 or 16 (plain layout)");
  if (envs_per_workgroup > def && one_layout_only(b)) return fail("the generic kernel family has one layout only");
  // a layout whose kernels ask for more LDS than a CU has is refused HERE, with the byte counts, before anything is launched (the
  // muscle humanoid with pair tables at 16: 169 048 B against 163 840 B — launched, that ended in an illegal memory access)
  { const std::string why = layout_refusal(b, envs_per_workgroup, false); if (!why.empty()) return fail(why); }
  b->epb = envs_per_workgroup;
  b->nblocks = (b->N + b->epb - 1) / b->epb;
  return 0;
}

void lm_batch_destroy(lm_batch* b) {
  if (!b) return;
  hipSetDevice(b->m->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  for (const lm_batch::Owned& o : b->owned) batch_release(o.field, o.pinned);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->ev_ext) (void)hipEventDestroy(b->ev_ext);
  if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
  if (b->ev_join) (void)hipEventDestroy(b->ev_join);
  if (b->ev_done[0]) (void)hipEventDestroy(b->ev_done[0]);
  if (b->ev_done[1]) (void)hipEventDestroy(b->ev_done[1]);
  if (b->stream2) { (void)hipStreamSynchronize(b->stream2); (void)hipStreamDestroy(b->stream2); }
  if (b->h_hint) (void)hipHostFree(b->h_hint);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

// masked uploads move only the masked environments: compact rows + their indices go up, a small kernel scatters them into
// the [dim][N] arrays (reference counterpart: the per-environment reset of LocoEnv.reset, environments/base.py:344-373)
__global__ void scatter_rows(float* __restrict__ dst, const float* __restrict__ rows, const int* __restrict__ idx,
                             int n, int dim, int N) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * dim) return;
  const int k = t / dim, d = t - k * dim;
  dst[(size_t)d * N + idx[k]] = rows ? rows[t] : 0.0f;
}
__global__ void zero_ints(int* __restrict__ dst, const int* __restrict__ idx, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[idx[t]] = 0;
}

// indices of the masked environments, uploaded once per call into b->scr_idx; staging sized for `dim` floats per row
static int mask_indices(lm_batch* b, const uint8_t* mask, int dim, std::vector<int>& idx) {
  idx.clear();
  for (int e = 0; e < b->N; e++) if (mask[e]) idx.push_back(e);
  const size_t need = (size_t)std::max<size_t>(idx.size(), 1) * (size_t)std::max(dim, 1);
  if (need > b->scr_cap) {
    HIPCHK(hipStreamSynchronize(b->stream));
    b->scr_cap = 0;
    if (batch_array(b, &b->scr, need)) return 1;
    b->scr_cap = need;
  }
  if (!b->scr_idx && batch_array(b, &b->scr_idx, b->N)) return 1;
  if (!idx.empty()) HIPCHK(hipMemcpyAsync(b->scr_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// rows == nullptr: zero the masked rows
static int scatter_masked(lm_batch* b, float* dev, const float* host_aos, int dim, const std::vector<int>& idx) {
  const int n = (int)idx.size();
  if (n == 0 || dim == 0) return 0;
  if (host_aos) {
    std::vector<float> rows((size_t)n * dim);
    for (int k = 0; k < n; k++) memcpy(&rows[(size_t)k * dim], host_aos + (size_t)idx[k] * dim, sizeof(float) * dim);
    HIPCHK(hipMemcpyAsync(b->scr, rows.data(), sizeof(float) * n * dim, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));     // `rows` is pageable host memory that dies with this frame
  }
  const int threads = 256, blocks = (n * dim + threads - 1) / threads;
  hipLaunchKernelGGL(scatter_rows, dim3(blocks), dim3(threads), 0, b->stream, dev, host_aos ? b->scr : nullptr, b->scr_idx, n, dim, b->N);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

static int upload_soa(lm_batch* b, float* dev, const float* host_aos, int dim, const uint8_t* mask) {
  const int N = b->N;
  if (mask) {
    std::vector<int> idx;
    if (mask_indices(b, mask, dim, idx)) return 1;
    return scatter_masked(b, dev, host_aos, dim, idx);
  }
  std::vector<float> soa((size_t)dim * N);
  for (int e = 0; e < N; e++)
    for (int d = 0; d < dim; d++) soa[(size_t)d * N + e] = host_aos[(size_t)e * dim + d];
  HIPCHK(hipMemcpyAsync(dev, soa.data(), sizeof(float) * dim * N, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// the other direction, [dim][N] on the device -> [N][dim] on the host: wait for the library's stream, then a blocking copy
static int download_soa(lm_batch* b, const float* dev, float* host_aos, int dim) {
  const int N = b->N;
  std::vector<float> soa((size_t)dim * N);
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(soa.data(), dev, sizeof(float) * dim * N, hipMemcpyDeviceToHost));
  for (int e = 0; e < N; e++)
    for (int d = 0; d < dim; d++) host_aos[(size_t)e * dim + d] = soa[(size_t)d * N + e];
  return 0;
}

int lm_set_state(lm_batch* b, const float* qpos, const float* qvel, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  const int N = b->N, nv = b->m->T.nv, na = b->m->T.na;
  if (mask) {
    // positions, velocities, and the cleared warm start / activations / step counter of the masked environments only
    std::vector<int> idx;
    if (mask_indices(b, mask, nv, idx)) return 1;
    if (scatter_masked(b, b->qpos, qpos, nv, idx)) return 1;
    if (scatter_masked(b, b->qvel, qvel, nv, idx)) return 1;
    if (scatter_masked(b, b->warm, nullptr, nv, idx)) return 1;
    if (b->act && scatter_masked(b, b->act, nullptr, na, idx)) return 1;
    if (scatter_masked(b, b->slack, nullptr, 12, idx)) return 1;           // new positions: the self-collision detection is due
    if (!idx.empty()) {
      const int n = (int)idx.size();
      hipLaunchKernelGGL(zero_ints, dim3((n + 255) / 256), dim3(256), 0, b->stream, b->ep_step, b->scr_idx, n);
      hipLaunchKernelGGL(zero_ints, dim3((n + 255) / 256), dim3(256), 0, b->stream, b->premark, b->scr_idx, n);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(b->stream));
    }
    return 0;
  }
  if (upload_soa(b, b->qpos, qpos, nv, nullptr)) return 1;
  if (upload_soa(b, b->qvel, qvel, nv, nullptr)) return 1;
  if (b->act) HIPCHK(hipMemsetAsync(b->act, 0, sizeof(float) * na * N, b->stream));
  HIPCHK(hipMemsetAsync(b->warm, 0, sizeof(float) * nv * N, b->stream));
  HIPCHK(hipMemsetAsync(b->ep_step, 0, sizeof(int) * N, b->stream));
  HIPCHK(hipMemsetAsync(b->premark, 0, sizeof(int) * N, b->stream));
  HIPCHK(hipMemsetAsync(b->slack, 0, sizeof(float) * 12 * N, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_get_state(lm_batch* b, float* qpos, float* qvel) {
  HIPCHK(hipSetDevice(b->m->device));
  const int nv = b->m->T.nv;
  if (qpos && download_soa(b, b->qpos, qpos, nv)) return 1;
  if (qvel && download_soa(b, b->qvel, qvel, nv)) return 1;
  return 0;
}

int lm_set_dof_params(lm_batch* b, const float* damping, const float* stiffness, const float* frictionloss, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  const int N = b->N, nv = b->m->T.nv;
  if (!b->dofprm) {
    // fail HERE, not at the first launch: the generic kernels (and six-link RK4 models, which have no kernel at all) are not
    // compiled for per-environment joint parameters / model variants
    if (!traits(b).env_params())
      return fail("per-environment joint parameters and model variants are not compiled for this model's kernel family (generic kernels)");
    std::vector<float> init((size_t)3 * nv * N);
    for (int p = 0; p < 3; p++) for (int d = 0; d < nv; d++) for (int e = 0; e < N; e++) init[((size_t)p * nv + d) * N + e] = b->m->nominal[(size_t)p * nv + d];
    if (batch_array(b, &b->dofprm, (size_t)3 * nv * N)) return 1;
    HIPCHK(hipMemcpy(b->dofprm, init.data(), sizeof(float) * 3 * nv * N, hipMemcpyHostToDevice));
  }
  const float* src[3] = {damping, stiffness, frictionloss};
  if (damping || stiffness || frictionloss) b->dofprm_of_variants = false;      // the caller's own values: they outlive the variant pool
  for (int p = 0; p < 3; p++) {
    if (!src[p]) continue;
    for (size_t i = 0; i < (size_t)N * nv; i++) if (!(src[p][i] >= 0.0f) && (!mask || mask[i / nv])) return fail("joint parameters must be non-negative");
    if (upload_soa(b, b->dofprm + (size_t)p * nv * N, src[p], nv, mask)) return 1;
  }
  return 0;
}

int lm_get_dof_params(lm_batch* b, float* damping, float* stiffness, float* frictionloss) {
  HIPCHK(hipSetDevice(b->m->device));
  const int N = b->N, nv = b->m->T.nv;
  float* dst[3] = {damping, stiffness, frictionloss};
  for (int p = 0; p < 3; p++) {
    if (!dst[p]) continue;
    if (b->dofprm) { if (download_soa(b, b->dofprm + (size_t)p * nv * N, dst[p], nv)) return 1; continue; }
    for (int e = 0; e < N; e++) for (int d = 0; d < nv; d++) dst[p][(size_t)e * nv + d] = b->m->nominal[(size_t)p * nv + d];
  }
  return 0;
}

int lm_set_dof_randomization(lm_batch* b, const float* spec) {
  HIPCHK(hipSetDevice(b->m->device));
  const int nv = b->m->T.nv;
  if (!spec) { batch_release(&b->drspec); return 0; }
  for (int i = 0; i < 3 * nv; i++) { const int k = (int)spec[3 * i]; if (k < 0 || k > 3) return fail("bad randomisation kind"); }
  if (!b->dofprm && lm_set_dof_params(b, nullptr, nullptr, nullptr, nullptr)) return 1;
  if (!b->drspec && batch_array(b, &b->drspec, (size_t)9 * nv)) return 1;
  HIPCHK(hipMemcpy(b->drspec, spec, sizeof(float) * 9 * nv, hipMemcpyHostToDevice));
  return 0;
}

static void compile_models(lm_batch* b, const unsigned char* mask, int all, hipStream_t stream);

int lm_set_model_variants(lm_batch* b, const float* records, const float* geom_tables, const float* pair_tables,
                          int pair_floats, int n_variants) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (float** p : {&b->vrec, &b->vgt, &b->vgpt}) batch_release(p);
  b->nvar = 0; b->gpt_floats = 0;
  batch_release(&b->mc_ib); batch_release(&b->mc_db);      // a pool replaces the compiler
  if (n_variants <= 0) {       // pool removed: the joint-parameter rows go with it when this call had created them
    if (b->dofprm_of_variants && !b->drspec) batch_release(&b->dofprm);
    b->dofprm_of_variants = false;
    return 0;
  }
  if (!records || !geom_tables) return fail("model variants need inertial records and geom tables");
  if ((pair_tables != nullptr) != (b->m->n_gpt_floats > 0) || (pair_tables && pair_floats != b->m->n_gpt_floats))
    return fail("geom-pair tables of the variants do not match the model's");
  if (!b->dofprm) {                                  // the kernels with per-environment parameters
    if (lm_set_dof_params(b, nullptr, nullptr, nullptr, nullptr)) return 1;
    b->dofprm_of_variants = true;
  }
  const size_t nr = (size_t)n_variants * LM_IR_SIZE * LM_NCHAIN, ng = (size_t)n_variants * LM_GT_SIZE, np_ = (size_t)n_variants * pair_floats;
  if (batch_array(b, &b->vrec, nr) || batch_array(b, &b->vgt, ng) || (pair_tables && batch_array(b, &b->vgpt, np_))) return 1;
  HIPCHK(hipMemcpy(b->vrec, records, sizeof(float) * nr, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->vgt, geom_tables, sizeof(float) * ng, hipMemcpyHostToDevice));
  if (pair_tables) HIPCHK(hipMemcpy(b->vgpt, pair_tables, sizeof(float) * np_, hipMemcpyHostToDevice));
  if (!b->var && batch_array(b, &b->var, b->N)) return 1;
  HIPCHK(hipMemset(b->var, 0, sizeof(int) * b->N));
  HIPCHK(hipMemset(b->slack, 0, sizeof(float) * 12 * b->N));
  b->nvar = n_variants; b->gpt_floats = pair_floats;
  return 0;
}

int lm_set_variant_index(lm_batch* b, const int32_t* index, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  if (b->nvar <= 0) return fail("the batch has no model variants");
  if (b->mc_ib) return fail("the model compiler is on: every environment owns its slot (lm_compile_models draws a new model)");
  std::vector<int> cur(b->N);
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(cur.data(), b->var, sizeof(int) * b->N, hipMemcpyDeviceToHost));
  for (int e = 0; e < b->N; e++) {
    if (mask && !mask[e]) continue;
    if (index[e] < 0 || index[e] >= b->nvar) return fail("variant index out of range");
    cur[e] = index[e];
  }
  HIPCHK(hipMemcpy(b->var, cur.data(), sizeof(int) * b->N, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b->slack, 0, sizeof(float) * 12 * b->N));       // another model: whatever the pair pass knew is void
  return 0;
}

int lm_set_variant_rows(lm_batch* b, int rows_per_variant) {
  if (rows_per_variant < 0) return fail("rows_per_variant must be >= 0");
  if (rows_per_variant > 0 && b->mc_ib) return fail("the model compiler is on: the model does not follow the reset-table row");
  if (rows_per_variant > 0 && (b->nvar <= 0 || b->table_rows != b->nvar * rows_per_variant))
    return fail("the reset table must hold n_variants blocks of rows_per_variant rows (set the variants and the table first)");
  b->var_rows = rows_per_variant;
  return 0;
}

int lm_get_variant_index(lm_batch* b, int32_t* index) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->nvar <= 0) { for (int e = 0; e < b->N; e++) index[e] = 0; return 0; }
  HIPCHK(hipMemcpy(index, b->var, sizeof(int) * b->N, hipMemcpyDeviceToHost));
  return 0;
}

int lm_set_model_compiler(lm_batch* b, const int32_t* index, long long n_index, const double* data, long long n_data,
                          const float* record, const float* geom_table, const float* pair_table, int pair_floats, uint64_t seed) {
  HIPCHK(hipSetDevice(b->m->device));
  if (!index || !data || n_index < lmc::kIntHead || n_data < lmc::kDblHead) return fail("the model compiler needs its program");
  if ((unsigned)index[0] != lmc::kMagic) return fail("not a model-compiler program (lowering.model_compiler_tables)");
  const int nv = index[1], nrb = index[2], ngs = index[3], nd = index[4], nslot = index[5], nrec = index[6], ncon = index[7], nbody = index[8];
  if (nv != b->m->T.nv) return fail("the model-compiler program is of another model (nv)");
  if (nv > lmc::kMaxNv || nrb > lmc::kMaxRbody || ngs > lmc::kMaxGslot || nd > lmc::kMaxDraw || nslot > lmc::kMaxSlot || nbody > lmc::kMaxBody || nd < 1)
    return fail("the model-compiler program is beyond the device compiler's tables (lm_compile.h)");
  const long long want_i = lmc::kIntHead + (long long)nd * lmc::kDrawInts + (long long)nrb * lmc::kRbInts + 2ll * nrec + (long long)ncon * lmc::kConInts;
  const long long want_d = lmc::kDblHead + (long long)nd * lmc::kDrawDbls + (long long)nrb * lmc::kRbDbls + (long long)nbody * 6 * nv + (long long)nv * nv + 2ll * nv +
                           (long long)nslot * 10 + 3ll * ngs;
  if (want_i != n_index || want_d != n_data) return fail("the model-compiler program has the wrong size");
  const int* recops = index + lmc::kIntHead + nd * lmc::kDrawInts + nrb * lmc::kRbInts;
  for (int i = 0; i < nrec; i++)
    if (recops[2 * i] < 0 || recops[2 * i] >= LM_IR_SIZE * LM_NCHAIN || recops[2 * i + 1] < 0 || recops[2 * i + 1] >= 3 * nv + 1 + nslot * 10)
      return fail("the model-compiler program writes outside the inertial record");
  const int* conops = recops + 2 * nrec;
  for (int i = 0; i < ncon; i++) {
    const int* op = conops + i * lmc::kConInts;
    const long long last = (long long)op[1] + 12ll * op[2], cap = op[0] == 0 ? (long long)LM_GT_SIZE : (long long)pair_floats;
    if (op[0] < 0 || op[0] > 1 || op[1] < 0 || op[2] < 1 || last >= cap || op[4] < 0 || op[4] >= ngs || op[5] < 0 || op[5] >= ngs ||
        op[6] < 0 || op[6] >= nbody || op[7] < 0 || op[7] >= nbody)
      return fail("the model-compiler program writes outside the contact tables");
  }
  // what the draws and the drawn bodies index (the kernel sizes its LDS tables by the header's counts and indexes the body Jacobians by
  // these numbers: a malformed program must not get past this point — round-5 advisor; the Python binding checks the same)
  const int* draws = index + lmc::kIntHead;
  for (int i = 0; i < nd; i++) {
    const int kind = draws[4 * i], target = draws[4 * i + 1], idx = draws[4 * i + 2], comp = draws[4 * i + 3];
    const int lim_i = target == 0 ? nv : (target >= 1 && target <= 3 ? nrb : (target == 4 ? ngs : -1)), lim_c = (target == 0 || target == 1) ? 1 : 3;
    if (kind < 1 || kind > 3 || lim_i < 0 || idx < 0 || idx >= lim_i || comp < 0 || comp >= lim_c) return fail("the model-compiler program has a draw outside its table");
  }
  const int* rbody = draws + nd * lmc::kDrawInts;
  for (int i = 0; i < nrb; i++) {
    const int body = rbody[4 * i], kind = rbody[4 * i + 1], slot = rbody[4 * i + 2], has_sv = rbody[4 * i + 3];
    if (body <= 0 || body >= nbody || kind < 1 || kind > 2 || slot < 0 || slot >= nslot || has_sv < 0 || has_sv > 1) return fail("the model-compiler program has a drawn body outside the model");
  }
  // ... and the nominal tables, BEFORE anything of the batch's current variant state is torn down
  if (!record || !geom_table) return fail("the model compiler needs the nominal inertial record and geom table");
  if ((pair_table != nullptr) != (b->m->n_gpt_floats > 0) || (pair_table && pair_floats != b->m->n_gpt_floats))
    return fail("the geom-pair table does not match the model's");
  // the tables: one slot per environment, every slot starts as the nominal model
  if (lm_set_model_variants(b, nullptr, nullptr, nullptr, 0, 0)) return 1;
  if (!b->dofprm) {
    if (lm_set_dof_params(b, nullptr, nullptr, nullptr, nullptr)) return 1;
    b->dofprm_of_variants = true;
  }
  const int N = b->N;
  const size_t nr = (size_t)LM_IR_SIZE * LM_NCHAIN, ng = (size_t)LM_GT_SIZE, np_ = (size_t)(pair_table ? pair_floats : 0);
  dev_temp<float> nominal_tmp;      // the nominal tables on the device, for this call
  if (dev_temp_alloc(&nominal_tmp, nr + ng + np_)) return 1;
  float* nominal = nominal_tmp.get();
  HIPCHK(hipMemcpy(nominal, record, sizeof(float) * nr, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(nominal + nr, geom_table, sizeof(float) * ng, hipMemcpyHostToDevice));
  if (np_) HIPCHK(hipMemcpy(nominal + nr + ng, pair_table, sizeof(float) * np_, hipMemcpyHostToDevice));
  if (batch_array(b, &b->vrec, nr * N) || batch_array(b, &b->vgt, ng * N) || (np_ && batch_array(b, &b->vgpt, np_ * N))) return 1;
  lmc::replicate(b->vrec, nominal, (long long)nr, N, b->stream);
  lmc::replicate(b->vgt, nominal + nr, (long long)ng, N, b->stream);
  if (np_) lmc::replicate(b->vgpt, nominal + nr + ng, (long long)np_, N, b->stream);
  if (!b->var && batch_array(b, &b->var, N)) return 1;
  lmc::iota(b->var, N, b->stream);
  if (batch_array(b, &b->mc_ib, (size_t)n_index) || batch_array(b, &b->mc_db, (size_t)n_data) || batch_array(b, &b->vdirty, N) ||
      batch_array(b, &b->mc_mask, N) || batch_array(b, &b->vgen, N) || batch_array(b, &b->vdraws, (size_t)N * nd)) return 1;
  HIPCHK(hipMemcpy(b->mc_ib, index, sizeof(int) * n_index, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->mc_db, data, sizeof(double) * n_data, hipMemcpyHostToDevice));
  b->mc_ndraw = nd; b->mc_seed = seed; b->nvar = N; b->gpt_floats = (int)np_; b->var_rows = 0;
  compile_models(b, nullptr, 1, b->stream);            // every environment starts on a model of its own
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_compile_models(lm_batch* b, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  if (!b->mc_ib) return fail("the batch has no model compiler (lm_set_model_compiler)");
  if (mask) HIPCHK(hipMemcpyAsync(b->mc_mask, mask, b->N, hipMemcpyHostToDevice, b->stream));
  compile_models(b, mask ? b->mc_mask : nullptr, mask ? 0 : 1, b->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_get_model_draws(lm_batch* b, double* draws, uint32_t* generation) {
  HIPCHK(hipSetDevice(b->m->device));
  if (!b->mc_ib) return fail("the batch has no model compiler (lm_set_model_compiler)");
  HIPCHK(hipStreamSynchronize(b->stream));
  if (draws) HIPCHK(hipMemcpy(draws, b->vdraws, sizeof(double) * (size_t)b->N * b->mc_ndraw, hipMemcpyDeviceToHost));
  if (generation) HIPCHK(hipMemcpy(generation, b->vgen, sizeof(unsigned) * b->N, hipMemcpyDeviceToHost));
  return 0;
}

int lm_get_model_tables(lm_batch* b, int env, float* record, float* geom_table, float* pair_table) {
  HIPCHK(hipSetDevice(b->m->device));
  if (b->nvar <= 0) return fail("the batch has no model variants");
  if (env < 0 || env >= b->N) return fail("environment out of range");
  HIPCHK(hipStreamSynchronize(b->stream));
  int var = 0;
  HIPCHK(hipMemcpy(&var, b->var + env, sizeof(int), hipMemcpyDeviceToHost));
  if (record) HIPCHK(hipMemcpy(record, b->vrec + (size_t)var * LM_IR_SIZE * LM_NCHAIN, sizeof(float) * LM_IR_SIZE * LM_NCHAIN, hipMemcpyDeviceToHost));
  if (geom_table) HIPCHK(hipMemcpy(geom_table, b->vgt + (size_t)var * LM_GT_SIZE, sizeof(float) * LM_GT_SIZE, hipMemcpyDeviceToHost));
  if (pair_table && b->vgpt) HIPCHK(hipMemcpy(pair_table, b->vgpt + (size_t)var * b->gpt_floats, sizeof(float) * b->gpt_floats, hipMemcpyDeviceToHost));
  return 0;
}

int lm_set_activation(lm_batch* b, const float* act, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  if (!b->act) return fail("model has no activation states");
  return upload_soa(b, b->act, act, b->m->T.na, mask);
}

int lm_get_activation(lm_batch* b, float* act) {
  HIPCHK(hipSetDevice(b->m->device));
  if (!b->act) return fail("model has no activation states");
  return download_soa(b, b->act, act, b->m->T.na);
}

int lm_set_goal(lm_batch* b, const float* goal, const uint8_t* mask) {
  HIPCHK(hipSetDevice(b->m->device));
  if (b->m->T.ngoal == 0) return 0;
  return upload_soa(b, b->goal, goal, b->m->T.ngoal, mask);
}

static KArgs make_args(lm_batch* b) {
  KArgs a;
  memset(&a, 0, sizeof(a));
  a.cm = b->m->d_cm; a.mt = b->m->d_mt; a.act = b->act; a.dofprm = b->dofprm; a.drspec = b->drspec;
  a.vrec = b->nvar > 0 ? b->vrec : nullptr; a.vgt = b->vgt; a.vgpt = b->vgpt; a.var = b->var; a.nvar = b->nvar; a.gpt_floats = b->gpt_floats; a.var_rows = b->var_rows; a.vdirty = b->mc_ib ? b->vdirty : nullptr; a.qpos = b->qpos; a.qvel = b->qvel; a.warm = b->warm; a.goal = b->goal;
  a.term_obs = b->term_obs;
  a.ep_step = b->ep_step; a.ep_count = b->ep_count; a.flags = b->flags; a.slack = b->slack; a.mprc = b->mprc; a.mprc_pairs = b->mprc_pairs; a.env_map = b->env_map; a.n_active = b->n_active;
  a.table = b->table; a.table_rows = b->table_rows; a.seed = b->seed; a.env_offset = b->env_offset;
  a.auto_reset = b->auto_reset; a.horizon = b->horizon; a.step_index = b->step_index;
  a.N = b->N; a.P = b->m->P; a.T = b->m->T; a.stats = b->stats;
  a.epb = b->epb; a.timers = b->timers; a.tline = b->tline; a.nfused = 1;
  // speculate / replay: every family but the generic one has a replay kernel
  if (b->replay && traits(b).specialised()) { a.replay_list = b->replay_list; a.replay_ctl = b->replay_ctl; a.stall = b->stall; a.replay_mark = b->replay_mark;
    static const bool no_resume = LM_PROBE_ENV("LM_NO_RESUME") != nullptr;       // A/B: restart abandoned control steps from their own state (round 4)
    if (!no_resume) { a.hq = b->hq; a.hv = b->hv; a.hw = b->hw; }
    a.hsub = b->hsub;
    static const bool no_premark = LM_PROBE_ENV("LM_NO_PREMARK") != nullptr;       // A/B: every control step starts in the regular kernel (round 4)
    if (!no_premark) {
      a.premark = b->premark;
      // the regular kernels' capacity per chain (lm_families.h / lm_core.h LaneMem: contact slots, queued convex pairs, pair results)
      const Task& T = b->m->T;
      a.reg_ns = traits(b).NS; a.reg_q = T.max_links >= 5 ? 24 : 8; a.reg_r = a.reg_ns < 8 ? a.reg_ns : 8;
    } a.replay_all = b->replay == 2 || b->replay == 4; }
  static const bool no_xcd_map = LM_PROBE_ENV("LM_NO_XCD_MAP") != nullptr;
  a.xcd_map = no_xcd_map ? 0 : 1;
  return a;
}

static void compile_models(lm_batch* b, const unsigned char* mask, int all, hipStream_t stream) {
  lmc::Args c;
  c.ib = b->mc_ib; c.db = b->mc_db; c.N = b->N; c.seed = b->mc_seed; c.env_offset = b->env_offset; c.dirty = b->vdirty; c.mask = mask; c.all = all;
  c.gen = b->vgen; c.vrec = b->vrec; c.vgt = b->vgt; c.vgpt = b->vgpt; c.gpt_floats = b->gpt_floats; c.slack = b->slack; c.draws = b->vdraws;
  lmc::launch(c, stream);
}

// The stream an entry point works on: the caller's (e.g. torch's current stream) or, for null, the library's own. enter() orders it
// behind everything the batch has in flight: the library's stream (ev_ext), and the last launch with a replay pass wherever it ran — its
// drain pass waits for the pollers of stream2 (ev_join) and is followed by ev_done, so that event also covers a launch that another
// caller's stream still holds. leave() orders the library's stream behind the stream in use, so that whatever the library queues next
// (lm_get_state, lm_get_stats, lm_rollout ...) waits for this call's work; an entry point that returns early leaves through the destructor
struct StreamScope {
  lm_batch* b; hipStream_t used; bool entered = false;
  StreamScope(lm_batch* b_, void* stream) : b(b_), used(stream ? (hipStream_t)stream : b_->stream) {}
  StreamScope(const StreamScope&) = delete;
  int enter() {
    if (b->epoch > 0) HIPCHK(hipStreamWaitEvent(used, b->ev_done[(b->epoch - 1) & 1], 0));
    if (used != b->stream) { HIPCHK(hipEventRecord(b->ev_ext, b->stream)); HIPCHK(hipStreamWaitEvent(used, b->ev_ext, 0)); }
    entered = true;
    return 0;
  }
  int leave() {
    if (!entered) return 0;
    entered = false;
    if (used != b->stream) { HIPCHK(hipEventRecord(b->ev_ext, used)); HIPCHK(hipStreamWaitEvent(b->stream, b->ev_ext, 0)); }
    return 0;
  }
  ~StreamScope() { (void)leave(); }
};
// `queue(stream)` inside a scope: enter, queue, leave, and wait for the stream if asked. The per-thread HIP error state is shared with
// whoever else uses HIP in this process: what they left behind is dropped, so that the check after `queue` reports OUR launches
extern "C++" template <class Queue> static int on_stream(lm_batch* b, void* stream, int sync, Queue queue) {
  StreamScope scope(b, stream);
  if (scope.enter()) return 1;
  (void)hipGetLastError();
  if (queue(scope.used)) return 1;
  HIPCHK(hipGetLastError());
  if (scope.leave()) return 1;
  if (sync) HIPCHK(hipStreamSynchronize(scope.used));
  return 0;
}

// Where the control steps of one call take their actions and leave their results: the first step's pointer and the stride from one
// control step to the next, in elements (0: every step at the same rows). `action_mode` is the kernels' (0: `action`, 1: zero, 2:
// uniform random); `seed` keys the random actions and the restarts; `term` null: the buffer of lm_set_terminal_obs, if any
struct StepIO {
  int action_mode; unsigned long long seed;
  const float* action; long long action_stride;
  float* obs; long long obs_stride;
  float* reward; long long reward_stride;
  unsigned char* done; long long done_stride;
  float* term; long long term_stride;
};
// the batch's own rows, overwritten by every control step: what lm_step* and the policy-free rollouts write
static StepIO own_rows(lm_batch* b, int action_mode, const float* action) {
  return {action_mode, b->seed, action, 0, b->obs, 0, b->reward, 0, b->done, 0, nullptr, 0};
}
// the tapes of lm_rollout_tape / lm_rollout_policy, one row set per control step. A tape that is not given: the batch's own rows as in
// lm_step_device, stride 0 — every control step overwrites them
static void record_on_tapes(StepIO* io, const lm_batch* b, float* d_obs, float* d_reward, uint8_t* d_done, float* d_term) {
  const long long N = b->N, nobs = b->m->T.nobs;
  if (d_obs) { io->obs = d_obs; io->obs_stride = N * nobs; }
  if (d_reward) { io->reward = d_reward; io->reward_stride = N; }
  if (d_done) { io->done = d_done; io->done_stride = N; }
  if (d_term) { io->term = d_term; io->term_stride = N * nobs; }
}

// THE launch path of lm_step*, lm_rollout_fused and lm_rollout_tape: queues `n_steps` control steps on `stream`, `steps_per_launch` of
// them per launch. b->step_index, the count that keys the random actions, advances by the launches that were accepted and by no
// other: a refused call leaves it where it was. `timed`: ev0 / ev1 around the span
// `pol` (lm_rollout_policy): the control steps take their actions from a policy, evaluated from the observation the step before left
// (pol->obs0 for the call's first step). A launch of several control steps: the POLICY instantiation of the fused kernel does it at the
// top of every step (lm_step.h KArgs::pol). A launch of ONE control step (the layouts and families without a fused kernel, the model
// compiler, a ragged last launch): policy_kernel (lm_policy.h) writes the step's row of the action tape in front of the ordinary
// launch, on the same stream. Both run lmp::policy_row: the actions are bitwise the same either way
struct PolicyCall { lm_mlp_policy p; const float* obs0; unsigned long long noise_seed; };
static int queue_steps(lm_batch* b, hipStream_t stream, const StepIO& io, int n_steps, int steps_per_launch, bool timed, const PolicyCall* pol = nullptr) {
  // one control step per launch where there is no fused kernel (the full-wave layout, the generic family), and with the model compiler:
  // a restart inside a launch needs its fresh model before the episode's first step. The launch's pointers then carry the offsets
  if (b->epb > 4 || replicas_off() || one_layout_only(b) || b->mc_ib) steps_per_launch = 1;
#ifdef LM_NO_POLICY_KERNELS
  if (pol) steps_per_launch = 1;      // a library built without the POLICY instantiations (lm_step.h): policy_kernel in front of every step
#endif
  KArgs a = make_args(b);
  a.action_mode = io.action_mode; a.seed = io.seed;
  a.tape_action = io.action_stride; a.tape_obs = io.obs_stride; a.tape_reward = io.reward_stride; a.tape_done = io.done_stride; a.tape_term = io.term_stride;
  if (timed) HIPCHK(hipEventRecord(b->ev0, stream));
  for (int s = 0; s < n_steps; s += steps_per_launch) {
    a.nfused = (n_steps - s < steps_per_launch) ? n_steps - s : steps_per_launch;
    a.step_index = b->step_index;
    a.action = io.action ? io.action + s * io.action_stride : nullptr;
    a.obs = io.obs + s * io.obs_stride; a.reward = io.reward + s * io.reward_stride; a.done = io.done + s * io.done_stride;
    if (io.term) a.term_obs = io.term + s * io.term_stride;
    // the per-thread HIP error state is shared with whoever else uses HIP in this process (PyTorch probes peers, pointer
    // attributes ...): drop what they left behind so that the check after the launch reports OUR launch
    (void)hipGetLastError();
    g_launch_err = nullptr;
    if (pol) {
      const float* prev = s == 0 ? pol->obs0 : io.obs + (s - 1) * io.obs_stride;
      a.pol.d_params = nullptr;
      if (a.nfused > 1) {
        a.pol = pol->p; a.pol_obs0 = prev; a.pol_seed = pol->noise_seed; a.pol_hand = b->pol_hand; a.pol_norm = b->pol_norm;
        if (!a.term_obs) a.term_obs = b->pol_sink;
      } else {
        if (!io.term) a.term_obs = b->term_obs;        // (not the sink of an earlier fused launch of this call)
        lmp::PolicyArgs pa = {pol->p, b->pol_norm, prev, const_cast<float*>(a.action), b->env_map, b->n_active, pol->noise_seed, b->env_offset, b->step_index};
        lmp::launch_policy(pa, stream);
      }
    }
    launch_variant<false>(b, a, stream);
    if (g_launch_err) return fail(g_launch_err);
    // the environments that restarted an episode in this launch get their fresh model before the next one (stream order)
    if (b->mc_ib && b->auto_reset && b->table_rows > 0) compile_models(b, nullptr, 0, stream);
    HIPCHK(hipGetLastError());
    b->step_index += (unsigned)a.nfused;
  }
  if (timed) HIPCHK(hipEventRecord(b->ev1, stream));
  return 0;
}

static int drain_stats(lm_batch* b) {
  std::vector<DevStats> s(b->nstat);
  HIPCHK(hipMemcpyAsync(s.data(), b->stats, sizeof(DevStats) * b->nstat, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipMemsetAsync(b->stats, 0, sizeof(DevStats) * b->nstat, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (const DevStats& x : s) {
    b->acc.env_steps += x.env_steps; b->acc.episodes += x.episodes; b->acc.reward_sum += x.reward_sum;
    b->acc.nan_resets += x.nan_resets; b->acc.solver_iters += x.solver_iters; b->acc.overflow_contacts += x.overflow;
    b->acc.unhandled_geoms += x.unhandled; b->acc.linesearch_evals += x.ls_evals; b->acc.linesearch_capped += x.ls_capped; b->acc.steps_with_8plus_iters += x.it_ge8;
    b->acc.self_proximity += x.selfprox; b->acc.self_contacts += x.selfcon; b->acc.replayed_env_steps += x.replayed; b->acc.own_manifold_contacts += x.natown;
  }
  return 0;
}

// the end of a rollout behind queue_steps(..., timed = true): wait for the span (`wait` false: the call returns with the steps queued),
// add its time to the batch's and, with `drain`, the device's counters; `stats`: the totals, with this span's time
static int finish_rollout(lm_batch* b, bool wait, bool drain, lm_stats* stats) {
  if (!wait) return 0;
  HIPCHK(hipEventSynchronize(b->ev1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->acc.kernel_ms += ms;
  if (drain && drain_stats(b)) return 1;
  if (stats) { *stats = b->acc; stats->kernel_ms = ms; }
  return 0;
}

int lm_batch_set_active(lm_batch* b, const int32_t* env_ids, int count) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!env_ids) { b->n_active = b->N; batch_release(&b->env_map); return 0; }
  if (traits(b).no_active_lists()) return fail("active lists are not compiled into the quadruped's kernels (lm_step.h: the indirection costs the bench kernel 0.9 %)");
  if (count < 0 || count > b->N) return fail("active list: more entries than environments");
  std::vector<char> seen((size_t)b->N, 0);
  for (int i = 0; i < count; i++) {
    if (env_ids[i] < 0 || env_ids[i] >= b->N) return fail("active list: environment id out of range");
    if (seen[env_ids[i]]) return fail("active list: an environment is listed twice");
    seen[env_ids[i]] = 1;
  }
  if (!b->env_map && batch_array(b, &b->env_map, (size_t)b->N)) return 1;
  if (count > 0) HIPCHK(hipMemcpy(b->env_map, env_ids, sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
  b->n_active = count;
  return 0;
}

#ifndef LM_TOOLCHAIN
#define LM_TOOLCHAIN "unknown (built outside csrc/Makefile)"
#endif
const char* lm_toolchain(void) { return LM_TOOLCHAIN; }

int lm_lds_bytes(int family, int kind, int envs_per_workgroup, int cm_used_floats, int* static_bytes, int* dynamic_bytes) {
  lmk::LdsUse u;
  if (kind < 0 || kind >= lmk::LMK_NKINDS || cm_used_floats < 0 || !lds_of(family, kind, envs_per_workgroup, cm_used_floats, LM_MAXC, &u)) return fail("no kernel of that family and kind");
  if (static_bytes) *static_bytes = (int)u.stat;
  if (dynamic_bytes) *dynamic_bytes = (int)u.dyn;
  return 0;
}

int lm_step(lm_batch* b, const float* action, float* obs, float* reward, uint8_t* done) {
  HIPCHK(hipSetDevice(b->m->device));
  const int N = b->N; const Task& T = b->m->T;
  if (action) HIPCHK(hipMemcpyAsync(b->action, action, sizeof(float) * T.nu * N, hipMemcpyHostToDevice, b->stream));
  if (queue_steps(b, b->stream, own_rows(b, action ? 0 : 1, action ? b->action : nullptr), 1, 1, false)) return 1;
  if (obs) HIPCHK(hipMemcpyAsync(obs, b->obs, sizeof(float) * T.nobs * N, hipMemcpyDeviceToHost, b->stream));
  if (reward) HIPCHK(hipMemcpyAsync(reward, b->reward, sizeof(float) * N, hipMemcpyDeviceToHost, b->stream));
  if (done) HIPCHK(hipMemcpyAsync(done, b->done, N, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// ---- the float64 host surface (include/locohip.h lm_step_pinned)
__global__ void pack_out64_kernel(const float* __restrict__ obs, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                  const int* __restrict__ perm, int N, int nobs, double* __restrict__ o64, double* __restrict__ r64,
                                  unsigned char* __restrict__ d8) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, total = N * nobs;
  if (i < total) {
    const int e = i / nobs, j = i - e * nobs;
    o64[i] = (double)obs[e * nobs + (perm ? perm[j] : j)];
  }
  if (i < N) { r64[i] = (double)reward[i]; d8[i] = done[i]; }
}

// the same conversion with the terminal observations as the result set's fourth array: only the rows of the environments whose
// episode ended in this step (done byte, bit 1) are converted — the others keep what the slot held. Under an active list the done
// byte of an INACTIVE environment is the one of its last step: if that one had bit 1, its (unchanged) terminal row is converted
// again every step — the slot then holds that environment's last episode end, as the device buffer does.
__global__ void pack_out64_term_kernel(const float* __restrict__ obs, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                       const float* __restrict__ term, const int* __restrict__ perm, int N, int nobs, double* __restrict__ o64,
                                       double* __restrict__ r64, unsigned char* __restrict__ d8, double* __restrict__ t64) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, total = N * nobs;
  if (i < total) {
    const int e = i / nobs, j = i - e * nobs, src = e * nobs + (perm ? perm[j] : j);
    o64[i] = (double)obs[src];
    if (done[e] & 2) t64[i] = (double)term[src];
  }
  if (i < N) { r64[i] = (double)reward[i]; d8[i] = done[i]; }
}

// the fourth array of the pinned result sets (allocated when both the ring and the terminal observations are in use)
static int pinned_term_alloc(lm_batch* b) {
  if (b->h_term64[0]) return 0;
  for (int i = 0; i < LM_PINNED_SLOTS; i++) if (batch_array(b, &b->h_term64[i], (size_t)b->N * (size_t)b->m->T.nobs, true)) return 1;
  return 0;
}

static int pinned_alloc(lm_batch* b) {
  if (b->h_act) return 0;
  const size_t N = (size_t)b->N, nobs = (size_t)b->m->T.nobs;
  b->out64_bytes = sizeof(double) * (N * nobs + N) + N;
  if (batch_array(b, &b->h_act, N * (size_t)b->m->T.nu, true)) return 1;
  for (int i = 0; i < LM_PINNED_SLOTS; i++) if (batch_array(b, &b->h_out64[i], b->out64_bytes, true)) return 1;
  return 0;
}

int lm_pinned_slot(lm_batch* b, int slot, double** obs, double** reward, uint8_t** done) {
  HIPCHK(hipSetDevice(b->m->device));
  if (slot < 0 || slot >= LM_PINNED_SLOTS) return fail("pinned slot out of range");
  if (pinned_alloc(b)) return 1;
  const size_t N = (size_t)b->N, nobs = (size_t)b->m->T.nobs;
  double* base = reinterpret_cast<double*>(b->h_out64[slot]);
  if (obs) *obs = base;
  if (reward) *reward = base + N * nobs;
  if (done) *done = reinterpret_cast<uint8_t*>(base + N * nobs + N);
  return 0;
}

int lm_set_terminal_obs(lm_batch* b, int enabled, float* d_out) {
  if (!b) return fail("null batch");
  HIPCHK(hipSetDevice(b->m->device));
  // no launch in flight still writes the buffer that is being replaced: the library's stream waits (ev_ext) for every launch that
  // lm_step_device put on a caller's stream, so this wait covers those too
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!enabled) { b->term_obs = nullptr; return 0; }
  // the caller's device buffer (the batch's own, if any, is kept for later). Like the pointers of lm_step_device it is taken as given:
  // [n_envs][nobs] float32 on this batch's device is the caller's promise, the library cannot check it
  if (d_out) { b->term_obs = d_out; return 0; }
  const size_t bytes = sizeof(float) * (size_t)b->N * (size_t)b->m->T.nobs;
  if (!b->term_own && batch_array(b, &b->term_own, (size_t)b->N * (size_t)b->m->T.nobs)) return 1;
  HIPCHK(hipMemsetAsync(b->term_own, 0, bytes, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->term_obs = b->term_own;
  return 0;
}

int lm_set_policy_obs_norm(lm_batch* b, const float* d_mean, const float* d_inv_std, float clip) {
  if (!b) return fail("null batch");
  // every argument is checked before anything changes: a refused call leaves the setting as it was
  if ((d_mean == nullptr) != (d_inv_std == nullptr)) return fail("lm_set_policy_obs_norm: d_mean and d_inv_std go together (both NULL: off)");
  if (!std::isfinite(clip) || clip < 0.0f) return fail("lm_set_policy_obs_norm: clip must be finite and >= 0 (0: no clamp)");
  HIPCHK(hipSetDevice(b->m->device));
  // no launch in flight still reads the tensors that are being replaced (as lm_set_terminal_obs: the library's stream is ordered behind
  // every launch on a caller's stream). Like d_params the pointers are taken as given: [nobs] float32 on the batch's device
  HIPCHK(hipStreamSynchronize(b->stream));
  b->pol_norm.mean = d_mean; b->pol_norm.inv_std = d_inv_std; b->pol_norm.clip = d_mean ? clip : 0.0f;
  return 0;
}

int lm_get_terminal_obs(lm_batch* b, float* out) {
  if (!b) return fail("null batch");
  if (!b->term_obs) return fail("terminal observations are not enabled (lm_set_terminal_obs)");
  if (!out) return fail("lm_get_terminal_obs needs a host buffer [n_envs][nobs]");
  HIPCHK(hipSetDevice(b->m->device));
  // on the library's stream: behind every launch (one on a caller's stream included: ev_ext) and behind the replay kernel's pollers
  HIPCHK(hipMemcpyAsync(out, b->term_obs, sizeof(float) * (size_t)b->N * (size_t)b->m->T.nobs, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_pinned_terminal_obs(lm_batch* b, int slot, double** term_obs) {
  if (!b) return fail("null batch");
  HIPCHK(hipSetDevice(b->m->device));
  if (slot < 0 || slot >= LM_PINNED_SLOTS) return fail("pinned slot out of range");
  if (!b->term_obs) return fail("terminal observations are not enabled (lm_set_terminal_obs)");
  if (pinned_alloc(b) || pinned_term_alloc(b)) return 1;
  if (term_obs) *term_obs = b->h_term64[slot];
  return 0;
}

int lm_set_obs_order(lm_batch* b, const int32_t* perm, int n) {
  HIPCHK(hipSetDevice(b->m->device));
  if (b->d_perm) { HIPCHK(hipStreamSynchronize(b->stream)); batch_release(&b->d_perm); }
  if (!perm) return 0;
  const int nobs = b->m->T.nobs;
  if (n != nobs) return fail("observation order: one entry per observation column");
  for (int j = 0; j < n; j++) if (perm[j] < 0 || perm[j] >= nobs) return fail("observation order: column out of range");
  if (batch_array(b, &b->d_perm, (size_t)n)) return 1;
  HIPCHK(hipMemcpy(b->d_perm, perm, sizeof(int) * n, hipMemcpyHostToDevice));
  return 0;
}

int lm_step_pinned(lm_batch* b, const double* action, int slot) {
  HIPCHK(hipSetDevice(b->m->device));
  if (slot < 0 || slot >= LM_PINNED_SLOTS) return fail("pinned slot out of range");
  if (!action) return fail("lm_step_pinned needs an action (policy-free rollouts: lm_rollout)");
  if (pinned_alloc(b)) return 1;
  if (b->term_obs && pinned_term_alloc(b)) return 1;
  const int N = b->N; const Task& T = b->m->T;
  const size_t na = (size_t)N * T.nu;
  for (size_t i = 0; i < na; i++) b->h_act[i] = (float)action[i];
  // the step kernel reads the action out of the pinned staging buffer itself and the conversion kernel writes the pinned slot itself
  // (both mapped into the device's address space): no copy is queued on either side of the launch. Measured on one box against an
  // H2D copy in front and a D2H copy behind (tools/probes/r6/surface.py, 4096 quadrupeds): 1.258 against 1.274 ms per LocoEnv.step()
  if (queue_steps(b, b->stream, own_rows(b, 0, b->h_act), 1, 1, false)) return 1;
  double* o64 = reinterpret_cast<double*>(b->h_out64[slot]);
  const int total = N * T.nobs, threads = 256;
  if (b->term_obs)
    hipLaunchKernelGGL(pack_out64_term_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, b->stream, b->obs, b->reward, b->done, b->term_obs,
                       b->d_perm, N, T.nobs, o64, o64 + (size_t)N * T.nobs, reinterpret_cast<unsigned char*>(o64 + (size_t)N * T.nobs + N), b->h_term64[slot]);
  else
  hipLaunchKernelGGL(pack_out64_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, b->stream, b->obs, b->reward, b->done,
                     b->d_perm, N, T.nobs, o64, o64 + (size_t)N * T.nobs, reinterpret_cast<unsigned char*>(o64 + (size_t)N * T.nobs + N));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_step_device(lm_batch* b, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, void* stream, int sync) {
  HIPCHK(hipSetDevice(b->m->device));
  StepIO io = own_rows(b, d_action ? 0 : 1, d_action);
  if (d_obs) io.obs = d_obs;
  if (d_reward) io.reward = d_reward;
  if (d_done) io.done = d_done;
  return on_stream(b, stream, sync, [&](hipStream_t s) { return queue_steps(b, s, io, 1, 1, false); });
}

int lm_set_reset_table(lm_batch* b, const float* rows, int n_rows, uint64_t seed, int64_t global_env_offset) {
  HIPCHK(hipSetDevice(b->m->device));
  const Task& T = b->m->T;
  const size_t w = 2 * T.nv + T.ngoal;
  if (n_rows <= 0) return fail("empty reset table");
  if (batch_array(b, &b->table, w * n_rows)) return 1;
  HIPCHK(hipMemcpy(b->table, rows, sizeof(float) * w * n_rows, hipMemcpyHostToDevice));
  b->table_rows = n_rows; b->seed = seed; b->env_offset = global_env_offset;
  b->var_rows = 0;                 // a new table: the variant no longer follows the row until lm_set_variant_rows says so
  return 0;
}

// ---- state on device buffers (include/locostate.h ls_get_state_device, ls_set_state_device, ls_restart_device; the kernels: lm_state_io.h)
static lmio::State io_state(const lm_batch* b) {
  const Task& T = b->m->T;
  return {b->N, T.nv, T.na, T.ngoal, T.nobs, T.ngrf, b->qpos, b->qvel, b->warm, b->act, b->goal, b->slack, b->ep_step, b->ep_count, b->premark,
          b->m->d_qobs, b->m->d_vobs};
}

int ls_get_state_device(lm_batch* b, float* d_qpos, float* d_qvel, float* d_act, float* d_goal, int32_t* d_ep_step, uint32_t* d_ep_count,
                        void* stream, int sync) {
  if (!b) return fail("null batch");
  // every argument is checked before the launch: a refused call launches nothing
  if (!d_qpos && !d_qvel && !d_act && !d_goal && !d_ep_step && !d_ep_count) return fail("ls_get_state_device: every output is null (nothing to read)");
  if (d_act && !b->act) return fail("ls_get_state_device: d_act given, but the model has no activation states");
  HIPCHK(hipSetDevice(b->m->device));
  const lmio::GatherArgs a = {io_state(b), d_qpos, d_qvel, d_act, d_goal, d_ep_step, d_ep_count};
  return on_stream(b, stream, sync, [&](hipStream_t s) { lmio::launch_gather(a, s); return 0; });
}

int ls_set_state_device(lm_batch* b, const float* d_qpos, const float* d_qvel, const float* d_act, const float* d_goal, const uint8_t* d_mask,
                        float* d_obs, void* stream, int sync) {
  if (!b) return fail("null batch");
  if (!d_qpos || !d_qvel) return fail("ls_set_state_device: d_qpos and d_qvel are both needed (a state is positions and velocities)");
  if (d_act && !b->act) return fail("ls_set_state_device: d_act given, but the model has no activation states");
  HIPCHK(hipSetDevice(b->m->device));
  const lmio::ScatterArgs a = {io_state(b), d_qpos, d_qvel, d_act, b->m->T.ngoal > 0 ? d_goal : nullptr, d_mask, d_obs ? d_obs : b->obs};
  return on_stream(b, stream, sync, [&](hipStream_t s) { lmio::launch_scatter(a, s); return 0; });
}

int ls_restart_device(lm_batch* b, const uint8_t* d_mask, float* d_obs, void* stream, int sync) {
  if (!b) return fail("null batch");
  if (b->table_rows <= 0 || !b->table) return fail("ls_restart_device needs a reset table (lm_set_reset_table)");
  HIPCHK(hipSetDevice(b->m->device));
  const lmio::RestartArgs a = {io_state(b), b->table, b->table_rows, b->seed, b->env_offset, b->mc_ib ? b->vdirty : nullptr, b->var, b->nvar, b->var_rows,
                               b->dofprm, b->dofprm ? b->drspec : nullptr, d_mask, d_obs ? d_obs : b->obs};
  return on_stream(b, stream, sync, [&](hipStream_t s) {
    lmio::launch_restart(a, s);
    // the restarted environments get their fresh model before the next launch (stream order), as behind a step launch (queue_steps)
    if (b->mc_ib) compile_models(b, nullptr, 0, s);
    return 0;
  });
}

int lm_set_auto_reset(lm_batch* b, int enabled, int horizon) {
  if (enabled && b->table_rows <= 0) return fail("auto reset needs a reset table (lm_set_reset_table)");
  b->auto_reset = enabled; b->horizon = horizon;
  return 0;
}

int lm_rollout_fused(lm_batch* b, int n_steps, int steps_per_launch, int action_mode, uint64_t seed, lm_stats* stats) {
  HIPCHK(hipSetDevice(b->m->device));
  if (action_mode != 0 && action_mode != 1) return fail("action_mode must be 0 (zero) or 1 (uniform random)");
  if (steps_per_launch < 1) return fail("steps_per_launch must be >= 1");
  StepIO io = own_rows(b, action_mode == 0 ? 1 : 2, nullptr);   // kernel: 1 = zero action, 2 = random
  io.seed = b->seed ^ (seed * 0x9E3779B97F4A7C15ull);
  if (queue_steps(b, b->stream, io, n_steps, steps_per_launch, true)) return 1;
  return finish_rollout(b, true, true, stats);
}

int lm_rollout_tape(lm_batch* b, int n_steps, int steps_per_launch, const float* d_actions, long long action_step_stride,
                    float* d_obs, float* d_reward, uint8_t* d_done, float* d_term, void* stream, int sync, lm_stats* stats) {
  if (!b) return fail("null batch");
  HIPCHK(hipSetDevice(b->m->device));
  const long long N = b->N; const Task& T = b->m->T;
  // every argument is checked before the first launch: a refused call leaves the batch as it was
  if (n_steps < 0) return fail("lm_rollout_tape: n_steps must be >= 0");
  if (steps_per_launch < 1) return fail("lm_rollout_tape: steps_per_launch must be >= 1");
  if (!d_actions) return fail("lm_rollout_tape: d_actions is null (policy-free rollouts: lm_rollout_fused)");
  if (action_step_stride != 0 && action_step_stride != N * T.nu) return fail("lm_rollout_tape: action_step_stride must be n_envs * nu (a tape) or 0 (action repeat)");
  if (d_term && !b->term_obs) return fail("lm_rollout_tape: d_term needs terminal observations enabled (lm_set_terminal_obs)");
  // the batch's own seed: a tape launch restarts episodes exactly like lm_step*
  StepIO io = own_rows(b, 0, d_actions);
  io.action_stride = action_step_stride;
  record_on_tapes(&io, b, d_obs, d_reward, d_done, d_term);
  if (on_stream(b, stream, 0, [&](hipStream_t s) { return queue_steps(b, s, io, n_steps, steps_per_launch, true); })) return 1;
  return finish_rollout(b, sync, stats != nullptr, stats);
}

int lm_rollout_policy(lm_batch* b, const lm_mlp_policy* p, int n_steps, int steps_per_launch, uint64_t noise_seed,
                      const float* d_obs0, float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done,
                      float* d_term, void* stream, int sync, lm_stats* stats) {
  if (!b) return fail("null batch");
  HIPCHK(hipSetDevice(b->m->device));
  const long long N = b->N; const Task& T = b->m->T;
  // every argument is checked before the first launch: a refused call leaves the batch as it was
  if (!p) return fail("lm_rollout_policy: the policy is null");
  if (n_steps < 0) return fail("lm_rollout_policy: n_steps must be >= 0");
  if (steps_per_launch < 1) return fail("lm_rollout_policy: steps_per_launch must be >= 1");
  if (p->n_layers < 1 || p->n_layers > lmp::kPolicyMaxLayers) return fail("lm_rollout_policy: n_layers must be 1..3");
  if (p->sizes[0] != T.nobs) return fail("lm_rollout_policy: sizes[0] = " + std::to_string(p->sizes[0]) + ", the model's nobs = " + std::to_string(T.nobs));
  if (p->sizes[p->n_layers] != T.nu) return fail("lm_rollout_policy: sizes[n_layers] = " + std::to_string(p->sizes[p->n_layers]) + ", the model's nu = " + std::to_string(T.nu));
  for (int l = 1; l < p->n_layers; l++)
    if (p->sizes[l] < 1 || p->sizes[l] > lmp::kPolicyMaxWidth) return fail("lm_rollout_policy: hidden width " + std::to_string(p->sizes[l]) + " is outside 1..256");
  if (T.nobs > lmp::kPolicyMaxWidth || T.nu > lmp::kPolicyMaxWidth) return fail("lm_rollout_policy: nobs and nu must be at most 256");
  if (p->activation != 0 && p->activation != 1) return fail("lm_rollout_policy: activation must be 0 (tanh) or 1 (relu)");
  if (!p->d_params) return fail("lm_rollout_policy: d_params is null");
  if (!d_actions) return fail("lm_rollout_policy: d_actions is null (the action tape is the output and what the steps read)");
  if (d_term && !b->term_obs) return fail("lm_rollout_policy: d_term needs terminal observations enabled (lm_set_terminal_obs)");
  if (b->lds_ok[0] != b->epb) {          // (what the first launch would refuse, before the policy's kernel is queued)
    const std::string why = layout_refusal(b, b->epb, false);
    if (!why.empty()) return fail(why);
  }
  if (!b->pol_hand && batch_array(b, &b->pol_hand, (size_t)N * 2 * lmp::kPolicyMaxWidth)) return 1;
  if (!b->pol_sink && batch_array(b, &b->pol_sink, (size_t)N * T.nobs)) return 1;
  StepIO io = own_rows(b, 0, d_actions);
  io.action_stride = N * T.nu;
  record_on_tapes(&io, b, d_obs, d_reward, d_done, d_term);
  const PolicyCall pol = {*p, d_obs0 ? d_obs0 : b->obs, noise_seed};
  if (on_stream(b, stream, 0, [&](hipStream_t s) { return queue_steps(b, s, io, n_steps, steps_per_launch, true, &pol); })) return 1;
  return finish_rollout(b, sync, stats != nullptr, stats);
}

// Generalised advantage estimation over the tapes (locohip.h lm_tape_gae): one environment per lane, so that every row [t][.] of a tape
// is read and written coalesced; t runs from T-1 down with adv[t+1] and V[t+1] kept in registers. No step kernel: no LDS, no family.
// Every line is spelled out in single operations and explicit fmaf calls (-ffp-contract has nothing to decide), and what a cut makes
// unreachable is chosen away by selects, never multiplied by a mask: a NaN there does not reach the output.
namespace lmg {
struct GaeArgs {
  const float *reward, *value, *last_value, *term_value; const unsigned char* done;
  float gamma, lam; float *adv, *ret; int T; long long N;
};
constexpr int kGaeBlock = 256;

__global__ __launch_bounds__(kGaeBlock) void gae_kernel(GaeArgs a) {
  const long long e = (long long)blockIdx.x * kGaeBlock + threadIdx.x;
  if (e >= a.N) return;
  const float gl = a.gamma * a.lam;
  float adv_next = 0.0f, v_next = 0.0f;
  for (int t = a.T - 1; t >= 0; t--) {
    const long long at = (long long)t * a.N + e;
    const unsigned char d = a.done[at];
    const bool last = t == a.T - 1;
    const float r = a.reward[at], v = a.value[at];
    float next_v;
    if (d & 1) next_v = 0.0f;
    else if (d & 2) next_v = a.term_value ? a.term_value[at] : 0.0f;
    else next_v = last ? a.last_value[e] : v_next;
    const float delta = fmaf(a.gamma, next_v, r) - v;
    const float adv = (d != 0 || last) ? delta : fmaf(gl, adv_next, delta);
    if (a.adv) a.adv[at] = adv;
    if (a.ret) a.ret[at] = adv + v;
    adv_next = adv; v_next = v;
  }
}
}  // namespace lmg

int lm_tape_gae(lm_batch* b, int n_steps, const float* d_reward, const uint8_t* d_done, const float* d_value, const float* d_last_value,
                const float* d_term_value, float gamma, float lam, float* d_adv, float* d_ret, void* stream, int sync) {
  if (!b) return fail("null batch");
  // every argument is checked before the launch: a refused call launches nothing
  if (n_steps < 1) return fail("lm_tape_gae: n_steps must be >= 1");
  if (!d_reward) return fail("lm_tape_gae: d_reward is null");
  if (!d_done) return fail("lm_tape_gae: d_done is null");
  if (!d_value) return fail("lm_tape_gae: d_value is null");
  if (!d_last_value) return fail("lm_tape_gae: d_last_value is null");
  if (!d_adv && !d_ret) return fail("lm_tape_gae: d_adv and d_ret are both null (nothing to compute)");
  if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail("lm_tape_gae: gamma must be in [0, 1]");
  if (!(lam >= 0.0f && lam <= 1.0f)) return fail("lm_tape_gae: lam must be in [0, 1]");
  HIPCHK(hipSetDevice(b->m->device));
  const lmg::GaeArgs a = {d_reward, d_value, d_last_value, d_term_value, d_done, gamma, lam, d_adv, d_ret, n_steps, (long long)b->N};
  // on the given stream behind everything the batch has in flight (the rollout that fills the tapes), as the snapshot copy is
  return on_stream(b, stream, sync, [&](hipStream_t s) {
    hipLaunchKernelGGL(lmg::gae_kernel, dim3((unsigned)((a.N + lmg::kGaeBlock - 1) / lmg::kGaeBlock)), dim3(lmg::kGaeBlock), 0, s, a);
    return 0;
  });
}

int lm_rollout(lm_batch* b, int n_steps, int action_mode, uint64_t seed, lm_stats* stats) {
  return lm_rollout_fused(b, n_steps, 1, action_mode, seed, stats);
}

int lm_forward_debug(lm_batch* b, const float* action, lm_forward_out* out) {
  HIPCHK(hipSetDevice(b->m->device));
  const int N = b->N; const Task& T = b->m->T; const int nv = T.nv;
  KArgs a = make_args(b);
  a.stats = nullptr; a.replay_list = nullptr;
  if (action) { HIPCHK(hipMemcpy(b->action, action, sizeof(float) * T.nu * N, hipMemcpyHostToDevice)); a.action = b->action; a.action_mode = 0; }
  else a.action_mode = 1;
  const size_t per = (size_t)nv * nv + 5 * nv;
  dev_temp<float> buf_tmp; dev_temp<int> ibuf_tmp;      // the stage outputs on the device, for this call
  if (dev_temp_alloc(&buf_tmp, per * N) || dev_temp_alloc(&ibuf_tmp, (size_t)2 * N)) return 1;
  float* buf = buf_tmp.get(); int* ibuf = ibuf_tmp.get();
  HIPCHK(hipMemset(buf, 0, sizeof(float) * per * N));
  a.dM = buf; a.dbias = buf + (size_t)nv * nv * N; a.dsmooth = a.dbias + (size_t)nv * N; a.dqacc_smooth = a.dsmooth + (size_t)nv * N;
  a.dqacc = a.dqacc_smooth + (size_t)nv * N; a.dqfrc = a.dqacc + (size_t)nv * N; a.dncon = ibuf; a.diter = ibuf + N;
  (void)hipGetLastError();
  g_launch_err = nullptr;
  launch_variant<true>(b, a, b->stream);
  if (g_launch_err) return fail(g_launch_err);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->stream));
  auto get = [&](float* dst, const float* src, size_t n) -> int { if (dst) HIPCHK(hipMemcpy(dst, src, sizeof(float) * n, hipMemcpyDeviceToHost)); return 0; };
  if (get(out->M, a.dM, (size_t)nv * nv * N) || get(out->qfrc_bias, a.dbias, (size_t)nv * N) || get(out->qfrc_smooth, a.dsmooth, (size_t)nv * N) ||
      get(out->qacc_smooth, a.dqacc_smooth, (size_t)nv * N) || get(out->qacc, a.dqacc, (size_t)nv * N) || get(out->qfrc_constraint, a.dqfrc, (size_t)nv * N)) return 1;
  if (out->ncon) HIPCHK(hipMemcpy(out->ncon, a.dncon, sizeof(int) * N, hipMemcpyDeviceToHost));
  if (out->solver_iter) HIPCHK(hipMemcpy(out->solver_iter, a.diter, sizeof(int) * N, hipMemcpyDeviceToHost));
  return 0;
}

int lm_get_flags(lm_batch* b, uint8_t* out) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(out, b->flags, b->N, hipMemcpyDeviceToHost));
  return 0;
}

int lm_get_replay_marks(lm_batch* b, uint8_t* out, int reset) {
  if (!b) return fail("null batch");
  HIPCHK(hipSetDevice(b->m->device));
  // copy and clear ON the library's stream: it is ordered behind every launch (also one on a caller's stream: ev_ext) and behind the
  // replay kernel's pollers (ev_join), which write the marks
  if (out) HIPCHK(hipMemcpyAsync(out, b->replay_mark, b->N, hipMemcpyDeviceToHost, b->stream));
  if (reset) HIPCHK(hipMemsetAsync(b->replay_mark, 0, b->N, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int lm_get_stats(lm_batch* b, lm_stats* out, int reset) {
  HIPCHK(hipSetDevice(b->m->device));
  if (drain_stats(b)) return 1;
  if (out) *out = b->acc;
  if (reset) memset(&b->acc, 0, sizeof(b->acc));
  return 0;
}

#ifdef LM_TIMERS      // (the shipped library exports nothing that include/locohip.h does not declare: tests/test_abi_exports.py)
/* profiling builds (-DLM_TIMERS): cycles spent per solver region, summed over workgroups (not part of the ABI header) */
int lm_debug_timers(lm_batch* b, unsigned long long* out16) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(out16, b->timers, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->timers, 0, sizeof(unsigned long long) * 16));
  return 0;
}

/* profiling builds: per workgroup of the LAST launch [nblocks][16] = cycles, then per environment (4) solver iterations,
   contact slots (summed over passes), line-search evaluations */
int lm_debug_wg_records(lm_batch* b, unsigned long long* out, int nblocks) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (nblocks != b->nblocks) return fail("nblocks mismatch");
  HIPCHK(hipMemcpy(out, b->timers + 16, sizeof(unsigned long long) * 16 * (size_t)nblocks, hipMemcpyDeviceToHost));
  return 0;
}

/* profiling builds: per workgroup of the LAST launch [nblocks][16] = cycles per solver region */
int lm_debug_wg_regions(lm_batch* b, unsigned long long* out, int nblocks) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (nblocks != b->nblocks) return fail("nblocks mismatch");
  HIPCHK(hipMemcpy(out, b->timers + 16 + 16 * (size_t)nblocks, sizeof(unsigned long long) * 16 * (size_t)nblocks, hipMemcpyDeviceToHost));
  return 0;
}

/* profiling builds: wall-clock time line of the last launch(es) since the last call: [N][4] + [nblocks][2] (lm_step.h KArgs::tline), cleared */
int lm_debug_timeline(lm_batch* b, unsigned long long* out) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  const size_t n = 4 * (size_t)b->N + 2 * (size_t)b->nblocks;
  HIPCHK(hipMemcpy(out, b->tline, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->tline, 0, sizeof(unsigned long long) * n));
  return 0;
}

/* profiling builds: counters of the pair pass and the convex collider since the last call (16 values, summed over all lanes) */
int lm_debug_mpr_counters(lm_batch* b, unsigned long long* out8 /* 16 values */) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(out8, b->timers + 16 + 32 * (size_t)b->nblocks, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->timers + 16 + 32 * (size_t)b->nblocks, 0, sizeof(unsigned long long) * 16));
  return 0;
}

#endif

// ---- snapshots (include/locohip.h lm_snapshot_*; the table, the walks and the kernel: lm_snapshot.h)
}  // extern "C"

struct lm_snapshot {
  int sig[10];               // the configuration it was created for (kSnapSigNames)
  int flags;                 // bit 0: no collider cache
  int device;
  long long bytes;           // device storage
  unsigned char* data;
  unsigned step_index;       // the batch's count of control steps at the save
  bool saved;
};

static const char* const kSnapSigNames[10] = {"n_envs", "nv", "na", "nobs", "mprc_pairs", "dof_params", "n_variants", "gpt_floats", "model_compiler", "n_model_draws"};
constexpr uint32_t kSnapMagic = 0x50534d4cu /* "LMSP" */, kSnapVersion = 1;
struct SnapBlobHead { uint32_t magic, version; int32_t sig[10]; int32_t flags; uint32_t step_index; int64_t bytes; };

static void snap_signature(const lm_batch* b, int* sig) {
  const Task& T = b->m->T;
  const int v[10] = {b->N, T.nv, T.na, T.nobs, b->mprc_pairs, b->dofprm ? 1 : 0, b->nvar, b->gpt_floats, b->mc_ib ? 1 : 0, b->mc_ib ? b->mc_ndraw : 0};
  for (int i = 0; i < 10; i++) sig[i] = v[i];
}

// the batch's state arrays in the snapshot's order: a function of the signature and the flags alone, so that a snapshot created for
// one batch fits every batch of the same signature (lm_snapshot_import into a fresh batch)
static bool snap_table(const lm_batch* b, int flags, lms::Table* t) {
  const Task& T = b->m->T;
  const int N = b->N;
  lms::table_init(t, N);
  bool ok = lms::table_add_soa(t, b->qpos, T.nv, 4) && lms::table_add_soa(t, b->qvel, T.nv, 4) && lms::table_add_soa(t, b->warm, T.nv, 4) &&
            lms::table_add_soa(t, b->goal, 4, 4) && lms::table_add_soa(t, b->slack, 12, 4) && lms::table_add_soa(t, b->ep_step, 1, 4) &&
            lms::table_add_soa(t, b->ep_count, 1, 4) && lms::table_add_soa(t, b->premark, 1, 4) && lms::table_add_soa(t, b->reward, 1, 4) &&
            lms::table_add_soa(t, b->done, 1, 1) && lms::table_add_soa(t, b->flags, 1, 1) && lms::table_add_aos(t, b->obs, 4ll * T.nobs);
  if (ok && b->act) ok = lms::table_add_soa(t, b->act, T.na, 4);
  if (ok && b->dofprm) ok = lms::table_add_soa(t, b->dofprm, 3 * T.nv, 4);
  if (ok && b->nvar > 0 && !b->mc_ib) ok = lms::table_add_soa(t, b->var, 1, 4);      // a pool: the index is the state, the pool a setting
  if (ok && b->mc_ib) {
    // the model compiler: slot e IS environment e's model (var stays the identity), with its restart flag, draw counter and draws
    ok = lms::table_add_soa(t, b->vdirty, 1, 1) && lms::table_add_soa(t, b->vgen, 1, 4) && lms::table_add_aos(t, b->vdraws, 8ll * b->mc_ndraw) &&
         lms::table_add_aos(t, b->vrec, 4ll * LM_IR_SIZE * LM_NCHAIN) && lms::table_add_aos(t, b->vgt, 4ll * LM_GT_SIZE);
    if (ok && b->vgpt) ok = lms::table_add_aos(t, b->vgpt, 4ll * b->gpt_floats);
  }
  if (ok && b->mprc && !(flags & 1)) ok = lms::table_add_aos(t, b->mprc, 4ll * lm::kMprCacheFloats * b->mprc_pairs);
  return ok;
}

static int snap_check(const lm_batch* b, const int* sig, const char* who, const char* what) {
  int now[10];
  snap_signature(b, now);
  for (int i = 0; i < 10; i++)
    if (now[i] != sig[i]) {
      char why[200];
      snprintf(why, sizeof(why), "%s: the %s is of another configuration: %s = %d, the batch has %d", who, what, kSnapSigNames[i], sig[i], now[i]);
      return fail(why);
    }
  return 0;
}

extern "C" {

int lm_snapshot_create(lm_batch* b, int flags, lm_snapshot** out) {
  if (!b || !out) return fail("lm_snapshot_create: null batch");
  if (flags & ~1) return fail("lm_snapshot_create: unknown flag bits (bit 0: leave the collider cache out)");
  HIPCHK(hipSetDevice(b->m->device));
  lms::Table t;
  if (!snap_table(b, flags, &t)) return fail("lm_snapshot_create: more state arrays than the segment table holds");
  std::unique_ptr<lm_snapshot, void (*)(lm_snapshot*)> s(new lm_snapshot(), lm_snapshot_destroy);      // freed on every error path
  memset(s.get(), 0, sizeof(lm_snapshot));
  snap_signature(b, s->sig);
  s->flags = flags; s->device = b->m->device; s->bytes = t.bytes;
  HIPCHK(hipMalloc(&s->data, (size_t)t.bytes));
  // (the gaps between segments travel in lm_snapshot_export's blob.) Complete before this returns: the first save may run on a
  // caller's stream that knows nothing of this one
  HIPCHK(hipMemsetAsync(s->data, 0, (size_t)t.bytes, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  *out = s.release();
  return 0;
}

void lm_snapshot_destroy(lm_snapshot* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->data) (void)hipFree(s->data);         // (hipFree waits for the device: no copy still runs on it)
  delete s;
}

long long lm_snapshot_bytes(const lm_snapshot* s) { return s ? s->bytes : 0; }

int lm_snapshot_save(lm_batch* b, lm_snapshot* s, void* stream, int sync) {
  if (!b || !s) return fail("lm_snapshot_save: null batch or snapshot");
  if (snap_check(b, s->sig, "lm_snapshot_save", "snapshot")) return 1;
  HIPCHK(hipSetDevice(b->m->device));
  lms::Table t;
  if (!snap_table(b, s->flags, &t) || t.bytes != s->bytes) return fail("lm_snapshot_save: the snapshot's layout does not match the batch");
  return on_stream(b, stream, sync, [&](hipStream_t on) {
    lms::launch_copy(t, s->data, nullptr, 0, on);
    s->step_index = b->step_index; s->saved = true;
    return 0;
  });
}

int lm_snapshot_restore(lm_batch* b, const lm_snapshot* s, const int32_t* d_src, void* stream, int sync) {
  if (!b || !s) return fail("lm_snapshot_restore: null batch or snapshot");
  if (!s->saved) return fail("lm_snapshot_restore: nothing was saved into this snapshot");
  if (snap_check(b, s->sig, "lm_snapshot_restore", "snapshot")) return 1;
  HIPCHK(hipSetDevice(b->m->device));
  lms::Table t;
  if (!snap_table(b, s->flags, &t) || t.bytes != s->bytes) return fail("lm_snapshot_restore: the snapshot's layout does not match the batch");
  return on_stream(b, stream, sync, [&](hipStream_t on) {
    lms::launch_copy(t, s->data, d_src, 1, on);
    if (!d_src) b->step_index = s->step_index;      // every environment is back at the save: so is the count that keys the random actions
    return 0;
  });
}

int lm_snapshot_export(lm_batch* b, const lm_snapshot* s, void* host, long long n) {
  if (!b || !s || !host) return fail("lm_snapshot_export: null argument");
  if (!s->saved) return fail("lm_snapshot_export: nothing was saved into this snapshot");
  if (n < (long long)sizeof(SnapBlobHead) + s->bytes) return fail("lm_snapshot_export: the buffer is shorter than the blob (header + lm_snapshot_bytes)");
  HIPCHK(hipSetDevice(b->m->device));
  SnapBlobHead h;
  memset(&h, 0, sizeof(h));
  h.magic = kSnapMagic; h.version = kSnapVersion; h.flags = s->flags; h.step_index = s->step_index; h.bytes = s->bytes;
  for (int i = 0; i < 10; i++) h.sig[i] = s->sig[i];
  memcpy(host, &h, sizeof(h));
  StreamScope scope(b, nullptr);
  if (scope.enter()) return 1;
  HIPCHK(hipMemcpyAsync(static_cast<unsigned char*>(host) + sizeof(h), s->data, (size_t)s->bytes, hipMemcpyDeviceToHost, scope.used));
  HIPCHK(hipStreamSynchronize(scope.used));
  return 0;
}

int lm_snapshot_import(lm_batch* b, lm_snapshot* s, const void* host, long long n) {
  if (!b || !s || !host) return fail("lm_snapshot_import: null argument");
  SnapBlobHead h;
  if (n < (long long)sizeof(h)) return fail("lm_snapshot_import: the blob is shorter than its header");
  memcpy(&h, host, sizeof(h));
  if (h.magic != kSnapMagic) return fail("lm_snapshot_import: not a snapshot blob (magic word)");
  if (h.version != kSnapVersion) return fail("lm_snapshot_import: a blob of another version");
  if (snap_check(b, h.sig, "lm_snapshot_import", "blob") || snap_check(b, s->sig, "lm_snapshot_import", "snapshot")) return 1;
  if (h.flags != s->flags) return fail("lm_snapshot_import: blob and snapshot differ in flag bit 0 (the collider cache)");
  if (h.bytes != s->bytes) return fail("lm_snapshot_import: the blob's payload is not of this snapshot's size");
  if (n < (long long)sizeof(h) + h.bytes) return fail("lm_snapshot_import: the blob is cut short");
  HIPCHK(hipSetDevice(b->m->device));
  StreamScope scope(b, nullptr);
  if (scope.enter()) return 1;
  HIPCHK(hipMemcpyAsync(s->data, static_cast<const unsigned char*>(host) + sizeof(h), (size_t)s->bytes, hipMemcpyHostToDevice, scope.used));
  HIPCHK(hipStreamSynchronize(scope.used));
  s->step_index = h.step_index; s->saved = true;
  return 0;
}

int lm_sync(lm_batch* b) {
  HIPCHK(hipSetDevice(b->m->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

}  // extern "C"
