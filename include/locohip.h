/*
 * locohip.h — C-ABI of the MI355X batched locomotion step ("liblocohip.so").
 *
 * The reference has no C boundary on this path: LocoEnv.step() is mushroom-rl's MuJoCo.step, which
 * calls into the MuJoCo C library through its pybind module. The entry points
 * below are what a loco-mujoco maintainer would bind with ctypes to replace, for
 * a whole batch of environments at once:
 *
 *   lm_model_create     <- MjModel.from_xml_string + MultiMuJoCo.__init__ bookkeeping (model upload)
 *                          (/root/reference/loco_mujoco/environments/base.py:109-126;
 *                           obs/action spec unitreeA1.py:778-854)
 *   lm_batch_create     <- mujoco.MjData(model), one per environment (base.py:185)
 *   lm_set_state        <- LocoEnv.set_sim_state: data.joint(name).qpos/qvel = value (base.py:478-497)
 *                          after mj_resetData (base.py:180): also clears the solver warm start
 *   lm_get_state        <- data.qpos / data.qvel reads (ObservationHelper._build_obs, base.py:202)
 *   lm_set_dof_params / lm_set_dof_randomization / lm_set_model_variants <- DomainRandomizationHandler.get_randomized_model
 *                          (utils/domain_randomization.py:219-227): joint damping/stiffness/frictionloss per environment
 *   lm_set_model_compiler / lm_compile_models / lm_get_model_draws / lm_get_model_tables <- the reference's re-compile of a
 *                          randomised XML at every reset (base.py:183-185, utils/domain_randomization.py:219-227,386-514: armature,
 *                          Inertial mass / diaginertia / fullinertia, Geoms friction), drawn and compiled on the device
 *   lm_set/get_activation <- data.act (muscle activation state, humanoids.py:320 HumanoidMuscle; integrated by mj_step)
 *   lm_set_goal         <- per-episode goal written into the observation
 *                          (unitreeA1.py:288-291 set_goal, :454-476 _create_observation)
 *   lm_step             <- MuJoCo.step: _preprocess_action (base.py:606-621) -> ctrl ->
 *                          mujoco.mj_step(model, data, n_substeps) -> _create_observation
 *                          (base.py:584-604, unitreeA1.py:454-476) -> is_absorbing/_has_fallen
 *                          (base.py:243-255, unitreeA1.py:503-536) -> reward (base.py:170-176,
 *                          utils/reward.py:66-117, evaluated on the previous observation)
 *   lm_set_reset_table  <- Trajectory.reset_trajectory + set_sim_state for finished episodes
 *                          (utils/trajectory.py:236-273, base.py:178-203), done on the device
 *   lm_set_terminal_obs / lm_get_terminal_obs / lm_pinned_terminal_obs <- the observation an episode ENDED in: the reference's
 *                          step() returns it itself, because its reset() is a call of its own (base.py:344-373); with device-side
 *                          restarts the step's observation is already the new episode's, and the terminal one lands in a buffer
 *                          [n_envs][nobs] of its own (device memory, the batch's or the caller's; off by default)
 *   lm_rollout          <- the user's `for step in range(n): env.step(a)` loop
 *                          (tests/test_environments.py:15-38), kept on the device for benchmarking
 *   lm_rollout_fused    <- the same loop with several control steps per kernel launch (zero or in-kernel random actions)
 *   lm_rollout_tape     <- the same loop over a GIVEN action sequence, `for a in actions: env.step(a)` with no policy decision
 *                          inside (action repeat / frame skip, K-step action chunks, sampling planners, open-loop replay of
 *                          recorded actions), with every step's observation, reward and done byte recorded
 *   lm_rollout_policy   <- the same loop with a policy inside, `a = policy(obs); obs, r, absorbing, _ = env.step(a)`: a small MLP evaluated
 *                          on the device at the top of every control step, its actions recorded as a tape
 *   lm_set_policy_obs_norm <- the Standardizer in front of the reference's actor and critic (examples/imitation_learning/utils.py):
 *                          the policy of lm_rollout_policy reads the clipped, standardised observation
 *   lm_tape_gae         <- mushroom-rl's compute_gae over the dataset of one Core.learn epoch (the reference's PPO / TRPO baselines),
 *                          over the tapes and with the done byte's bits told apart, one launch
 *   lm_forward_debug    <- mujoco.mj_forward (base.py:362) with intermediate results, for parity tests
 *   lm_snapshot_create / _save / _restore / _export / _import <- copy.copy(data) / mujoco.mj_copyData of every environment's MjData
 *                          (the reference keeps one MjData per environment on the host, base.py:185; it has no call of its own for
 *                          this): save, rewind and fork environments on the device, for sampling planners and checkpoints
 *
 * All arrays at the boundary are caller-owned HOST buffers, row-major [n_envs][dim], float32.
 * Device memory lives behind the opaque handles. Functions return 0 on success, non-zero on error;
 * lm_last_error() returns a message for the calling thread. One handle = one GPU; handles are not
 * thread-safe (one host thread per handle), calls on a handle are stream-ordered.
 */
#ifndef LOCOHIP_H
#define LOCOHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lm_model lm_model;
typedef struct lm_batch lm_batch;

typedef struct {
  int nq, nv, nu, nobs, ngoal, n_substeps, n_chains, max_chain_dofs;
  int na;                  /* activation states per environment (muscles); 0 for torque-driven models */
} lm_dims;

typedef struct {
  double env_steps;        /* control steps executed, summed over environments */
  double episodes;         /* episodes finished (absorbing or horizon) */
  double reward_sum;       /* sum of rewards */
  double nan_resets;       /* environments reset because their state became non-finite */
  double solver_iters;     /* Newton iterations, summed over environments and substeps */
  double overflow_contacts;/* contacts dropped because a per-chain contact slot budget was exceeded */
  double unhandled_geoms;  /* substeps in which a geom without a device collider came within margin */
  double linesearch_evals; /* line-search function evaluations after the first, summed like solver_iters */
  double linesearch_capped;/* line searches that ran into the iteration cap */
  double steps_with_8plus_iters; /* env-steps in which some substep needed >= 8 Newton iterations */
  double kernel_ms;        /* HIP-event time of the step kernels of this call (rollout only) */
  double self_proximity;   /* forward passes x geom pairs WITHOUT a collider (a box / cylinder against another geom of the robot)
                              within the contact margin: the state was outside the validated collision domain */
  double self_contacts;    /* self-contacts simulated (sphere / capsule pairs in closed form, the engine's native box / cylinder colliders,
                              convex pairs of two links through MPR), summed over the forward passes */
  double replayed_env_steps; /* env-steps that left the regular kernel's capacity (contact slots, pair lists, convex collider) and were
                              run by the family's replay kernel instead (lm_batch_set_replay); part of env_steps */
  double own_manifold_contacts; /* of self_contacts: contacts of box-box and capsule-box pairs. Their manifold construction is this
                              library's own (the engine's mjc_BoxBox / mjc_CapsuleBox case analysis is not restated: csrc/lm_core.h nat_*):
                              exact where the geometry leaves no choice (pinned edge-edge case), approximate for face contacts */
} lm_stats;

typedef struct {
  /* all optional (NULL = skip); [n_envs][...] row-major float32 */
  float* M;            /* [nv*nv]  joint-space inertia */
  float* qfrc_bias;    /* [nv] */
  float* qfrc_smooth;  /* [nv]  passive - bias + actuator */
  float* qacc_smooth;  /* [nv] */
  float* qacc;         /* [nv]  after the constraint solve */
  float* qfrc_constraint; /* [nv] */
  int* ncon;           /* [1] active contacts */
  int* solver_iter;    /* [1] */
} lm_forward_out;

int lm_device_count(void);
const char* lm_last_error(void);

/* chain_model: float64 array laid out as in lm_layout.h (header H_* + constant table), produced by the
   host-side mini-compiler + lowering (loco_mujoco_amd/mjcf.py, lowering.py) from the MJCF model and the
   task description (observation/action spec, termination bounds, reward). Refused, with the reason, where no kernel
   is compiled for the model: six- and seven-link chains outside their families, and a muscle model that no muscle
   family fits (the generic kernels that serve other cones and integrators have no muscles). */
int lm_model_create(const double* chain_model, size_t n, int device, lm_model** out);
void lm_model_destroy(lm_model* m);
int lm_model_dims(const lm_model* m, lm_dims* out);

int lm_batch_create(lm_model* m, int n_envs, lm_batch** out);
void lm_batch_destroy(lm_batch* b);
/* Launch geometry (no counterpart in the reference: its step is one MjData at a time, base.py:185). envs_per_workgroup = 4: one wave
   per 4 environments, each replicated over 4 quads (default); 8 or 16: plain layout without replicas. Same physics either way.
   Refused, with the byte counts, where a kernel of the layout needs more LDS than a compute unit has (lm_lds_bytes). */
int lm_batch_set_layout(lm_batch* b, int envs_per_workgroup);
/* Speculate / replay (no counterpart in the reference: the engine it calls sizes its contact buffers for everything,
   environments/data/humanoid/humanoid_torque.xml:19 njmax 1000 / nconmax 400, data/atlas/atlas.xml:23). The regular step kernels hold a few
   contact slots per chain; a control step that needs more is abandoned unstored and run by the family's replay kernel (a slot for
   every contact, long pair lists, the convex collider): as a few polling workgroups beside the regular launch (second stream; only
   when recent launches abandoned steps) and as a pass behind it. enabled = 1 (default); 0 = regular kernels only: contacts beyond
   the slots are dropped and counted in overflow_contacts, and what the regular kernels leave to the replay kernel altogether (the
   quadruped's convex pairs and capsule-box pairs, root-joint limits of the muscle humanoid) is not simulated: flag bit 2 and
   self_proximity say when (A/B measurements); 2 = every control step through the replay kernel
   (tests); 3 / 4 = 1 / 2 without the pollers (for profilers that run one kernel at a time: pollers would wait out their 0.5 s). */
int lm_batch_set_replay(lm_batch* b, int enabled);
/* one byte per environment: 1 = the replay kernel ran at least one control step of this environment since the marks were last
   cleared (reset = 1 clears them after the copy; out may be NULL). Diagnostics of THIS path, like lm_get_flags. */
int lm_get_replay_marks(lm_batch* b, uint8_t* out, int reset);

/* mask: [n_envs] bytes, NULL = all environments. Setting a state clears that env's warm start. */
int lm_set_state(lm_batch* b, const float* qpos, const float* qvel, const uint8_t* mask);
int lm_get_state(lm_batch* b, float* qpos, float* qvel);
int lm_set_goal(lm_batch* b, const float* goal, const uint8_t* mask);
/* muscle activations [n_envs][na] (data.act of the reference: mj_resetData zeroes it, base.py:180, so lm_set_state
   and device-side episode restarts zero it too; these two exist for parity tests and for single arrays; a CHECKPOINT is lm_snapshot_save / lm_snapshot_export) */
/* per-environment joint damping / stiffness / frictionloss [n_envs][nv] (NULL = leave as is) — what the reference's
   domain randomisation changes per episode by re-compiling the model (utils/domain_randomization.py:299-383,
   base.py:183-185). The first call allocates the arrays (initialised with the model's values) and switches the batch
   to the kernel variant that reads them. */
int lm_set_dof_params(lm_batch* b, const float* damping, const float* stiffness, const float* frictionloss,
                      const uint8_t* mask);
int lm_get_dof_params(lm_batch* b, float* damping, float* stiffness, float* frictionloss);
/* redraw rule used when the device restarts an episode (lm_set_auto_reset): spec[3][nv][3] = (kind, a, b) per parameter
   (damping, stiffness, frictionloss) and dof; kind 0 keep, 1 max(N(a,b),0), 2 U(a,b), 3 max(N(a,b),0) as well (both normal
   kinds are clipped at 0: a joint parameter cannot be negative, utils/domain_randomization.py:335-337). NULL disables. */
int lm_set_dof_randomization(lm_batch* b, const float* spec);
/* model variants: what the reference's domain randomisation changes by re-compiling the model with other inertial / armature /
   geom-friction numbers (utils/domain_randomization.py:386-514 set_geom_conf / set_inertial_conf, base.py:183-185). The host
   lowers n_variants randomised models (lowering.variant_tables) and hands over, per variant, the inertial record
   [LM_IR_SIZE][4], the geom table [LM_GT_SIZE] and the geom-pair table [pair_floats] (NULL when the model has none). Every
   environment holds the index of its variant (0 after this call); a device-side restart redraws it uniformly. Switches the
   batch to the kernel variant with per-environment parameters, like lm_set_dof_params. n_variants = 0 removes the pool. */
int lm_set_model_variants(lm_batch* b, const float* records, const float* geom_tables, const float* pair_tables,
                          int pair_floats, int n_variants);
int lm_set_variant_index(lm_batch* b, const int32_t* index, const uint8_t* mask);
int lm_get_variant_index(lm_batch* b, int32_t* index);
/* several MODELS of one environment as variants (the reference's MultiMuJoCo draws a model per episode, base.py:186-190): the
   reset table holds n_variants blocks of rows_per_variant rows (each block with its model's constants in the goal columns);
   a device-side restart from row i then puts the environment on variant i / rows_per_variant. 0 = independent uniform redraw. */
int lm_set_variant_rows(lm_batch* b, int rows_per_variant);
/* the model compiler on the device: a FRESHLY randomised model per environment and episode, like the reference's re-compile at
   every reset() (base.py:183-185, utils/domain_randomization.py:219-227,386-514). `index` / `data` = the program of
   lowering.model_compiler_tables (the draws of the randomisation rules, the model's Jacobians at qpos0, where every derived
   value lands); `record` / `geom_table` / `pair_table` = the nominal model's tables (lm_set_model_variants' layout, ONE set).
   The batch then holds one slot per environment; this call and lm_compile_models (the host-side reset; mask NULL = everyone)
   draw and compile on the device, and so does every device-side restart (lm_set_auto_reset) before the episode's first step:
   armature / mass / diaginertia / fullinertia / geom friction drawn with a counter-based generator keyed by (seed, global
   environment id, models this environment has had), M(qpos0) -> dof_invweight0 / body_invweight0 / meaninertia in float64.
   Fused launches fall back to one control step per launch. lm_set_model_variants replaces the compiler by a pool again. */
int lm_set_model_compiler(lm_batch* b, const int32_t* index, long long n_index, const double* data, long long n_data,
                          const float* record, const float* geom_table, const float* pair_table, int pair_floats, uint64_t seed);
int lm_compile_models(lm_batch* b, const uint8_t* mask);
/* what the compiler drew for the CURRENT model of every environment, [N][n_draw] in the order of the program's draws, and how
   many models each environment has had (either may be NULL): the host (and the oracle) rebuild that model from these */
int lm_get_model_draws(lm_batch* b, double* draws, uint32_t* generation);
/* the tables environment `env` runs on (its variant's slot; any of the three may be NULL) */
int lm_get_model_tables(lm_batch* b, int env, float* record, float* geom_table, float* pair_table);
int lm_set_activation(lm_batch* b, const float* act, const uint8_t* mask);
int lm_get_activation(lm_batch* b, float* act);

/* one control step for every environment. action in [-1,1] (normalised, base.py:606-621).
   obs [n_envs][nobs], reward [n_envs], done [n_envs] may each be NULL. Synchronous.
   The done byte: bit 0 (value 1) = absorbing state (the reference's `absorbing`: is_absorbing(obs), base.py:274-282);
   bit 1 (value 2) = the episode ended in this step on the device's side — it was restarted from the reset table (the
   observation written is then the first of the NEW episode; the one it ended in is written to the terminal-observation
   buffer, lm_set_terminal_obs), or, without device-side restarts, this is the step that reached the horizon (the terminal
   buffer then receives a copy of that step's observation). `done & 1` is what the reference's step() returns; `done != 0` mixes truncation into it. */
int lm_step(lm_batch* b, const float* action, float* obs, float* reward, uint8_t* done);

/* the same step with DEVICE pointers (action [n_envs][nu], obs [n_envs][nobs], reward [n_envs], done [n_envs]; any may be
   NULL) for training loops that keep policy inputs/outputs on the GPU: no PCIe traffic. `stream` = a hipStream_t to run
   on (NULL: the library's own stream); with sync = 0 the call returns after the launch. The caller orders its own work
   against that stream. */
int lm_step_device(lm_batch* b, const float* d_action, float* d_obs, float* d_reward, uint8_t* d_done, void* stream, int sync);

/* TERMINAL OBSERVATIONS (off by default). Every control step whose done byte gets bit 1 writes the observation of the state the
   step REACHED — the state the episode ended in — into row e of a device buffer [n_envs][nobs] float32, row-major like `obs`,
   before the restart replaces state and goal: the goal columns hold the old episode's goal, the foot-force columns this step's mean
   force (the fresh episode's observation reports zeros there). Rows of environments whose episode did not end are not written (an
   inactive environment's neither): after lm_rollout / lm_rollout_fused a row holds the LAST episode end of its environment. A state
   that ended because it became non-finite is stored as computed, NaN / Inf included (lm_stats.nan_resets counts those steps).
     lm_set_terminal_obs    enabled = 1, d_out NULL: the batch allocates and owns the buffer, zero-filled by every such call;
                            d_out non-NULL: a caller-owned DEVICE buffer (for users of lm_step_device; never freed by the library,
                            and taken as given: at least [n_envs][nobs] float32 on the batch's device — size and device are NOT checked);
                            enabled = 0: off again. Waits for every launch of this batch still in flight, those that lm_step_device
                            queued on a caller's stream with sync = 0 included (the library's stream is ordered behind them).
     lm_get_terminal_obs    the buffer -> host [n_envs][nobs] float32, stream-ordered behind the last step; an error when off
     lm_pinned_terminal_obs with the feature on, every result set of lm_step_pinned's ring carries a fourth array, [n_envs][nobs]
                            float64 in the column order of lm_set_obs_order: lm_step_pinned's conversion kernel fills the rows whose
                            done byte has bit 1 (no extra copy is queued), the other rows keep what the slot held; an error when off.
                            (Under an active list an inactive environment keeps the done byte of its last step: while that has bit 1
                            its unchanged row is converted again, so the slot shows that environment's last episode end.) */
int lm_set_terminal_obs(lm_batch* b, int enabled, float* d_out);
int lm_get_terminal_obs(lm_batch* b, float* out);
int lm_pinned_terminal_obs(lm_batch* b, int slot, double** term_obs);

/* ACTIVE LIST: from now on every step / rollout of this batch runs only the listed environments (ids in [0, n_envs), each at most
   once; count 0: nothing runs), in one launch of ceil(count / environments per workgroup) workgroups; the others keep their state, and
   what the step writes for them (observation, reward, done) is left as it was. NULL: all environments again. Host buffers keep their
   [n_envs][...] shape — an environment keeps its row. For environments that share ids across several models and change model per
   episode (the reference's MultiMuJoCo with models that differ in geometry, base.py:186-190: HumanoidTorque4Ages "all"): one batch per
   model, each stepping the environments currently of its size. Random numbers stay keyed by the global environment id. Compiled into every
   kernel family but the quadruped's (one model per batch there; the indirection costs its bench kernel 0.9 %): refused for it. */
int lm_batch_set_active(lm_batch* b, const int32_t* env_ids, int count);

/* LocoEnv.step()'s host surface in ONE call (reference gymnasium.py:47-65 -> base.py step(): numpy float64 action in, float64
   observation / reward and the absorbing flag out — the library's counterpart of the dtype conversions and copies the Python
   layer did around lm_step, environments/base.py). The results land in PINNED host memory owned by the batch: a ring of
   LM_PINNED_SLOTS result sets, so that what step t returned stays intact while steps t+1 .. t+LM_PINNED_SLOTS-1 run.
     lm_pinned_slot   pointers to result set `slot` (allocated at the first call): obs [n_envs][nobs] float64 in the column order of
                      lm_set_obs_order, reward [n_envs] float64, done [n_envs] (the done byte of lm_step)
     lm_set_obs_order column j of the float64 observation = column perm[j] of the kernel's (the reference's observation order where
                      it differs from the device's, base.py _obs_perm); NULL: the kernel's order
     lm_step_pinned   one control step: the action (float64, pageable or not) is converted into a pinned staging buffer, which the step
                      kernel reads itself; a small kernel behind it converts observation / reward to float64 (applying the order)
                      straight into the pinned slot — no copy is queued on either side of the launch; synchronous */
#define LM_PINNED_SLOTS 4
int lm_pinned_slot(lm_batch* b, int slot, double** obs, double** reward, uint8_t** done);
int lm_set_obs_order(lm_batch* b, const int32_t* perm, int n);
int lm_step_pinned(lm_batch* b, const double* action, int slot);

/* device-side episode handling: rows = [qpos(nq) | qvel(nv) | goal(ngoal)]; when enabled, an
   environment whose step ended absorbing (or reached `horizon` control steps, 0 = never) restarts
   from a row drawn with a counter-based RNG keyed by (seed, global env id, episode count) and the
   observation returned for that step is the fresh one. */
int lm_set_reset_table(lm_batch* b, const float* rows, int n_rows, uint64_t seed, int64_t global_env_offset);
int lm_set_auto_reset(lm_batch* b, int enabled, int horizon);
/* Setting, reading and restarting environments from DEVICE memory, on a stream: include/locostate.h (the ls_ names, served by this
   library; a restart on request is the restart described above, for the environments of a mask). */

/* n_steps control steps entirely on the device. action_mode 0: zero action; 1: a ~ U(-1,1)^nu from
   the counter-based RNG, keyed by (seed, global env id, the batch's count of control steps so far, action index).
   The call runs under the batch's seed (lm_set_reset_table; 0 without a table) xor `seed` * 0x9E3779B97F4A7C15:
   that seed keys the actions AND the restart draws of these steps, so seed 0 restarts like lm_step does and
   another seed draws other restart rows too. Accumulates into *stats (may be NULL). */
int lm_rollout(lm_batch* b, int n_steps, int action_mode, uint64_t seed, lm_stats* stats);

/* The same rollout with `steps_per_launch` control steps per kernel launch: every environment advances on its own, without
   the device-wide join that ends each single-step launch with its slowest environment. Bitwise the same states,
   observations and statistics as lm_rollout (which is steps_per_launch = 1). It keeps the LAST step's observation, reward and done
   byte; actions that are known ahead for several steps go through lm_rollout_tape, a small MLP policy that decides every step
   through lm_rollout_policy; any other policy needs lm_step / lm_step_device. */
int lm_rollout_fused(lm_batch* b, int n_steps, int steps_per_launch, int action_mode, uint64_t seed, lm_stats* stats);

/* ACTION TAPES: n_steps control steps under given actions, `steps_per_launch` of them per kernel launch, every step recorded.
     d_actions            DEVICE float32 [n_steps][n_envs][nu] with action_step_stride = n_envs * nu (floats from one step's actions to
                          the next), or [n_envs][nu] with action_step_stride = 0: the same action in every step (action repeat).
                          NULL and any other stride are errors.
     d_obs, d_reward, d_done, d_term
                          DEVICE tapes [n_steps][n_envs][nobs] float32, [n_steps][n_envs] float32, [n_steps][n_envs] bytes and
                          [n_steps][n_envs][nobs] float32; each may be NULL. Step t writes row t. A NULL d_obs / d_reward / d_done
                          means what it means in lm_step_device: the batch's own [n_envs] rows, which then hold the last step's.
                          d_term receives the terminal observation of exactly the steps whose done byte has bit 1, at [t][e] (the
                          other rows are not touched); it needs lm_set_terminal_obs enabled — otherwise the call fails and launches
                          nothing. While d_term is given those rows go to the tape and NOT to the buffer of lm_set_terminal_obs;
                          with d_term NULL that buffer is written as by lm_step_device.
   The final state, every tape row and the statistics' event counters are bitwise what n_steps calls of lm_step_device fed
   d_actions[t] produce, whatever steps_per_launch is, a ragged last launch included. Two statistics are not event counters and
   follow the launches instead. lm_stats.reward_sum is a float32 sum per workgroup, and a fused launch adds up its own steps'
   rewards first: it agrees to rounding, while every single reward in the tape is bitwise. replayed_env_steps counts where a step
   ran: an environment handed to the replay kernel finishes its launch there, so the figure grows with steps_per_launch, as under
   lm_rollout_fused. The call runs under the batch's own seed and advances its count of control steps by n_steps, so episodes
   restart exactly as under lm_step.
   Layouts of more than 4 environments per workgroup, families without replicas and batches with the model compiler run one step
   per launch (as in lm_rollout_fused), with the same results. Under an active list the rows of inactive environments are left as
   they were in every tape. `stream`, `sync`: as in lm_step_device. With sync != 0 and stats != NULL the statistics are drained
   into *stats (kernel_ms: this call's, by HIP events); with sync = 0 *stats is not written. */
int lm_rollout_tape(lm_batch* b, int n_steps, int steps_per_launch, const float* d_actions, long long action_step_stride,
                    float* d_obs, float* d_reward, uint8_t* d_done, float* d_term, void* stream, int sync, lm_stats* stats);

/* CLOSED-LOOP POLICY ROLLOUTS: lm_rollout_tape with the actions computed on the device by a small MLP policy, step by step, from the
   observation the previous step wrote — the reference's `for t in range(K): a = policy(obs); obs, r, absorbing, _ = env.step(a)`
   (examples/reinforcement_learning: mushroom-rl's Core.learn loop around LocoEnv.step, base.py:344-373) without a host round trip
   or a torch launch per step. The policy is a plain description, read in place at every step; the library keeps nothing of it:
     n_layers, sizes      1..3 linear layers; sizes[0] = the model's nobs, sizes[n_layers] = its nu, the widths between 1..256
     activation           after every layer but the last (the output layer is linear; the actuator's clamp bounds the control as it
                          does for any tape action): 0 tanh, 1 relu
     d_params             DEVICE float32, per layer W [out][in] row-major, then b [out] — torch.nn.utils.parameters_to_vector of a
                          Sequential(Linear, act, Linear, act, Linear)
     d_log_std            DEVICE float32 [nu], or NULL: the action is the MLP's output (deterministic). Otherwise
                          a[k] = mean[k] + exp(d_log_std[k]) * z, z ~ N(0, 1) by Box-Muller on the counter-based generator, keyed by
                          (noise_seed, GLOBAL environment id, the batch's count of control steps at that step, k) under a salt of its
                          own: neither the uniform actions of lm_rollout nor the restart draws share numbers with it.
   Every unit accumulates in float32 in one fixed order (bias, then the inputs in index order, fused multiply-adds): an action does not
   depend on the launch split, the batch size or the environment's place in the batch. */
typedef struct {
  int n_layers;            /* 1..3 linear layers */
  int sizes[4];            /* sizes[0] == nobs, sizes[n_layers] == nu, hidden widths 1..256 (any value, not only multiples of 16) */
  int activation;          /* after every layer but the last: 0 tanh, 1 relu */
  const float* d_params;   /* DEVICE, float32, per layer: W [out][in] row-major, then b [out] */
  const float* d_log_std;  /* DEVICE [nu] or NULL (deterministic) */
} lm_mlp_policy;
/*   d_obs0               DEVICE [n_envs][nobs]: the observation the FIRST action is computed from, in the kernel's column order (the
                          one lm_step_device writes, not lm_set_obs_order's). NULL: the batch's own last-step row — valid after any
                          step of this batch, NOT after lm_set_state (which leaves that row as it was: pass the reset observation).
     d_actions            DEVICE [n_steps][n_envs][nu], required: step t's action is written to row t (the raw a, before the actuator's
                          clamp) and read from there by the step — the recorded tape fed to lm_rollout_tape repeats the rollout bitwise.
     d_obs, d_reward, d_done, d_term, steps_per_launch, stream, sync, stats
                          as in lm_rollout_tape (d_obs NULL: the batch's own row; the policy then reads that row).
   Every argument is checked before the first launch (the sizes against the model's nobs / nu, layer count, widths, null pointers): a
   refused call launches nothing and leaves the count of control steps where it was. Under an active list the rows of inactive
   environments are left as they were, the action tape's included.
   A launch of several control steps evaluates the policy inside the fused step kernel, at the top of every step; a launch of one
   control step (steps_per_launch = 1, a ragged last launch, and wherever lm_rollout_tape runs one step per launch: layouts of more than
   4 environments per workgroup, families without replicas, the model compiler) runs a small kernel of its own in front of the ordinary
   step kernel, on the same stream and without a host wait. Both run the same device function: the action tape is bitwise the same
   whatever steps_per_launch is. */
int lm_rollout_policy(lm_batch* b, const lm_mlp_policy* p, int n_steps, int steps_per_launch, uint64_t noise_seed,
                      const float* d_obs0, float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done,
                      float* d_term, void* stream, int sync, lm_stats* stats);

/* POLICY INPUT NORMALISATION (off by default): the policy of lm_rollout_policy reads clamp((obs - mean) * inv_std, -clip, clip) in place
   of the raw observation row — the running standardiser in front of the reference's actors (examples/imitation_learning/utils.py
   Standardizer) and of practically every locomotion PPO.
   d_mean, d_inv_std: DEVICE float32 [nobs] in the KERNEL's column order (that of lm_step_device / d_obs0, not lm_set_obs_order's);
   caller-owned, read in place at every policy evaluation like lm_mlp_policy.d_params (an update between two calls is seen by the next).
   clip > 0: the normalised input is clamped to [-clip, clip]; clip == 0: no clamp. Both pointers NULL: off (the default).
   One NULL and one not, clip < 0 or not finite: refused, nothing changes. Waits for the batch's launches in flight (as lm_set_terminal_obs).
   Per input: one subtraction, one multiplication, two selects, each rounded on its own — torch's ((x - mean) * inv_std).clamp(-clip, clip)
   bit for bit, a NaN staying NaN; both launch paths of lm_rollout_policy run it. Only what the policy reads is normalised: the observation
   rows and tapes the steps write, the terminal rows and d_obs0 stay raw. With the setting off the actions are bitwise what they were. */
int lm_set_policy_obs_norm(lm_batch* b, const float* d_mean, const float* d_inv_std, float clip);

/* Generalised advantage estimation over the tapes of lm_rollout_tape / lm_rollout_policy, with the done byte's meaning built in
   (the reference's training loop: mushroom-rl compute_gae with absorbing = done & 1, last = done != 0 or t == n_steps - 1).
     d_reward [T][n] f32, d_done [T][n] bytes        the tapes
     d_value  [T][n] f32                             V(the observation step t's action was computed from: obs0, then obs[t-1])
     d_last_value [n] f32                            V(obs[T-1]): the successor of the last step where that step ended no episode
     d_term_value [T][n] f32 or NULL                 V(terminal tape row), READ ONLY where done has bit 1 and not bit 0 (a truncation);
                                                     NULL: such steps bootstrap with 0
   next_v = 0 if done & 1; else d_term_value[t][e] if done & 2; else (t == T-1 ? d_last_value[e] : d_value[t+1][e])
   delta  = r + gamma * next_v - v;  adv[t] = delta + (done != 0 || t == T-1 ? 0 : gamma * lam * adv[t+1]);  ret[t] = adv[t] + v
   float32, one environment per lane, t from T-1 down, each line above one fmaf chain in the order written — delta = fmaf(gamma, next_v, r)
   - v, adv[t] = fmaf(gamma * lam, adv[t+1], delta) with the product gamma * lam rounded once: the result does not depend on n, the
   launch shape or the environment's place. What a cut makes unreachable (d_value[t+1], d_last_value, adv[t+1]) is selected away, not
   multiplied by zero: a NaN there stays out. d_adv, d_ret [T][n] f32, either may be NULL (not both). All n_envs rows are computed,
   active list or not. One launch on `stream`, ordered behind everything the batch has in flight as the snapshot copy is; stream, sync:
   as lm_rollout_tape. Checked before the launch: null pointers, n_steps < 1, gamma / lam outside [0, 1] or not finite — a refused call
   launches nothing. */
int lm_tape_gae(lm_batch* b, int n_steps, const float* d_reward, const uint8_t* d_done, const float* d_value, const float* d_last_value,
                const float* d_term_value, float gamma, float lam, float* d_adv, float* d_ret, void* stream, int sync);

/* SNAPSHOTS: the state of every environment of a batch, kept in device memory — save, rewind, fork (environment e continues from
   the state environment w reached), and a self-describing blob for files. A restored batch continues BIT FOR BIT as the batch that
   was saved would have (lm_set_state cannot do that: it carries qpos / qvel only and clears the rest).
   A snapshot holds everything a later control step reads, per environment: qpos, qvel, the solver warm start, the goal, the muscle
   activations, the episode's step and the episode count, the replay prediction mark, the self-collision slack, the convex collider's
   warm-start cache, the per-environment joint parameters (when allocated), the model-variant index — with the model compiler instead
   the environment's own slot of the inertial record / geom table / geom-pair table, its restart flag, draw counter and draws — the
   batch's last-step rows (observation, reward, done byte, validity flags), and the batch's count of control steps.
   It does NOT hold settings (the reset table, seed and horizon, the active list, the layout, the replay mode, the randomisation
   spec, the variant pool, the compiler program, the policy's input normalisation of lm_set_policy_obs_norm), accumulators and diagnostics (lm_stats, replay marks, the pollers' hint, timers),
   output buffers (the pinned ring, terminal-observation buffers of the library or the caller) or the scratch of a launch (the
   replay list and its control words, the resume states): every launch leaves those consumed.
     lm_snapshot_create   device storage sized for b's configuration NOW: n_envs, nv, na, nobs, the collider cache's pairs, whether
                          joint parameters exist, the number of variants and their pair floats, the model compiler and its draws.
                          Save, restore and import refuse a batch whose configuration differs, naming the field; nothing is launched.
                          flags bit 0: leave the convex collider's warm-start cache out (HumanoidTorque: 88 KB per environment,
                          363 MB at 4096). Restore then leaves the batch's cache rows as they are. The cache is meant to decide how
                          fast the collider answers, not what; equal supports on flat hull faces may break that, so only the default
                          (cache kept) is promised bitwise.
     lm_snapshot_save     one kernel launch copies every state array into the snapshot (again: into the same storage).
     lm_snapshot_restore  one launch back. d_src NULL: every environment takes its own saved state, and the batch's count of control
                          steps is rewound to the saved one. Otherwise d_src is a DEVICE int32 [n_envs]: environment e takes the saved
                          state of environment d_src[e]; an entry outside [0, n_envs) means "e keeps what it has" (nothing is read or
                          written for e), and the count of control steps is left alone.
                          FORK: the copy includes the episode's step and the episode count, while every random number stays keyed by the
                          global environment id. A forked environment equals its source until one of them restarts on the device; from
                          then on each draws its own reset row (and model).
     lm_snapshot_bytes    device bytes of the snapshot
     lm_snapshot_export / _import  the snapshot <-> a host blob of `n` bytes: a header (magic word, version, the configuration, the
                          flags, the count of control steps; 64 bytes) and lm_snapshot_bytes of payload. Import refuses a blob that is
                          short, foreign or of another configuration and leaves snapshot and batch as they were. Synchronous.
   `stream`, `sync`: as in lm_rollout_tape. The copy is ordered behind everything the batch has in flight — the library's stream, the
   replay kernel's pollers, a launch that lm_step_device queued on a caller's stream with sync = 0 — and the library's stream behind
   the copy. With sync = 0 nothing waits on the host: a planner saves, rolls a tape, picks winners on the device and restores with
   d_src without a synchronisation. The snapshot must outlive the work queued on it (lm_snapshot_destroy waits for the device). */
typedef struct lm_snapshot lm_snapshot;
int lm_snapshot_create(lm_batch* b, int flags, lm_snapshot** out);
void lm_snapshot_destroy(lm_snapshot* s);
int lm_snapshot_save(lm_batch* b, lm_snapshot* s, void* stream, int sync);
int lm_snapshot_restore(lm_batch* b, const lm_snapshot* s, const int32_t* d_src, void* stream, int sync);
long long lm_snapshot_bytes(const lm_snapshot* s);
int lm_snapshot_export(lm_batch* b, const lm_snapshot* s, void* host, long long n);
int lm_snapshot_import(lm_batch* b, lm_snapshot* s, const void* host, long long n);

/* Validity flags of the LAST control step, one byte per environment: 1 = a contact was dropped (the chain's contact slots were
 * full), 2 = two geoms of the robot WITHOUT a pair collider (a box or cylinder against another geom) came within the contact
 * margin, 4 = a geom without a floor collider (mesh without hull) reached the floor. 0 = the step stayed inside the collision model
 * that the parity tests validate. No counterpart in the reference (MuJoCo collides everything): statistics of THIS path. */
int lm_get_flags(lm_batch* b, uint8_t* out);

/* one forward-dynamics pass at the current state with `action`, without advancing it */
int lm_forward_debug(lm_batch* b, const float* action, lm_forward_out* out);

/* the compiler the library was built with and its optimisation level ("HIP version: ...;AMD clang version ... | -Os"), recorded by
   csrc/Makefile: no counterpart in the reference; the kernels sit at the 512-register ceiling, where one code-generation defect of the
   toolchain was met (csrc/Makefile) — a library built by another compiler should be re-validated (tests/test_abi_exports.py) */
const char* lm_toolchain(void);
/* LDS per workgroup, in bytes, of one step kernel: what it declares itself (static: the muscle table of the muscle families, the statistics
   block) and what its launch asks for (dynamic: the model's constant table of cm_used_floats floats + lane memory). Host arithmetic from the
   constants the launches use; no device is touched, nothing is launched. family: 0 quadruped, 2 / 4 five-link humanoids RK4 / Euler, 5
   muscles, 6 generic, 7 six-link chains, 8 / 9 / 10 five-link chains with self-collisions RK4 / Euler / muscles, 11 seven-link chains.
   kind: 0 forward (lm_forward_debug), 1 / 2 replicated / plain, 3 / 4 the same with joint parameters, 5 / 6 fused, 7 / 8 replicated /
   plain with model variants, 9 fused with model variants, 10 / 11 / 12 the replay kernels. Non-zero: the family has no such kernel.
   lm_batch_set_layout refuses a layout whose step kernels exceed a compute unit's LDS (160 KB on gfx950), lm_forward_debug its own kernel
   (no counterpart in the reference: it has no launch geometry). */
int lm_lds_bytes(int family, int kind, int envs_per_workgroup, int cm_used_floats, int* static_bytes, int* dynamic_bytes);

int lm_get_stats(lm_batch* b, lm_stats* out, int reset);
int lm_sync(lm_batch* b);

#ifdef __cplusplus
}
#endif
#endif
