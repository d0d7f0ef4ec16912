/*
 * locotape.h — C-ABI of the learner's side of the tapes ("liblocotape.so"): episode returns and lengths from the reward and done
 * tapes of lm_rollout_tape / lm_rollout_policy (include/locohip.h), carried across rollouts.
 *
 * The reference measures its policies with mushroom-rl's dataset helpers, once per epoch
 * (the reference's examples/imitation_learning/experiment.py:51-58):
 *
 *   lt_tape_episodes         <- compute_J(dataset) (R_mean), compute_J(dataset, gamma) (J_mean) and compute_episodes_length(dataset) (L)
 *                               (experiment.py:51-53), over the tapes and per environment, with the running discounted return that
 *                               reward normalisation divides by (VecNormalize-style) from the same scan
 *   lt_episode_carry_reset   <- the fresh dataset of the next epoch after a host-side reset() (base.py:344-373): running episodes dropped
 *
 * One difference, on purpose: mushroom-rl appends the trailing PARTIAL episode of a dataset to its lists (compute_J and
 * compute_episodes_length count whatever is left after the last `last` flag). Here an unfinished episode is never counted: it stays in
 * the carry, and the next call continues it — episodes run across rollout boundaries.
 *
 * This library knows no lm_batch, no model and no step kernel: it reads tapes. All pointers are DEVICE pointers. Functions return 0 on
 * success, non-zero on error; lt_last_error() returns a message for the calling thread. The launches go to the calling thread's current
 * device (hipSetDevice), which must be the one the buffers and the stream live on.
 */
#ifndef LOCOTAPE_H
#define LOCOTAPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per calling thread, as lm_last_error */
const char* lt_last_error(void);

/* THE CARRY: what an environment's running episode has accumulated so far, float32 [LT_CARRY_ROWS][n_envs] — row 0 ret (the undiscounted
   return), row 1 disc (the discounted return), row 2 w (gamma ^ steps of the episode, the weight of the next reward), row 3 g (the running
   discounted return of the reward normaliser, g = gamma * g + r) — and its length in steps, int32 [n_envs]. Caller-owned: saving or forking
   it beside a snapshot (lm_snapshot_save / lm_snapshot_restore with d_src) is a copy / a gather by the same d_src. */
#define LT_CARRY_ROWS 4
/* THE SUMMARY: float64 [LT_SUMMARY_FIELDS] — 0 episodes, 1 sum R, 2 sum R*R, 3 min R, 4 max R, 5 sum J, 6 sum L, 7 min L, 8 max L,
   9 absorbing (episodes whose last done byte has bit 0), R = ret, J = disc, L = len of the finished episodes. With no episode: count 0, sums
   0, min +inf, max -inf. Sums are plain per process: they all-reduce across shards as they are (min / max by min / max). A NaN return
   makes the sums NaN and is passed over by min / max. */
#define LT_SUMMARY_FIELDS 10

/* size of d_work in doubles for n_envs environments (LT_SUMMARY_FIELDS per workgroup of 256 lanes); host arithmetic, no device.
   0 for n_envs < 1. */
long long lt_episode_work_doubles(long long n_envs);

/* A fresh carry — ret = disc = g = 0, w = 1, len = 0 — for every environment (d_mask NULL) or where the mask byte is set: after a
   host-side reset() / lm_set_state that drops running episodes. Refused before the first HIP call: n_envs < 1, null d_carry / d_len. */
int lt_episode_carry_reset(long long n_envs, float* d_carry, int32_t* d_len, const uint8_t* d_mask, void* stream, int sync);

/* Episode returns and lengths over n_steps rows of the tapes, continuing the carry.
     d_reward [n_steps][n_envs] f32, d_done [n_steps][n_envs] bytes    the tapes, row-major, as the rollouts write them
     d_mask   [n_envs] bytes or NULL   an environment whose mask byte is 0 is skipped: nothing is read, written or counted for it, and its
                                       carry stays. Under an active list (lm_batch_set_active) the tape rows of inactive environments are
                                       stale by contract of lm_rollout_tape: pass the list as a mask.
     d_carry, d_len                    the carry (above): loaded at the start, stored at the end
     d_ep_return, d_ep_disc_return [n_steps][n_envs] f32, d_ep_length [n_steps][n_envs] int32, each may be NULL
                                       written at [t][e] where an episode ENDED (done != 0); rows with done == 0 are NOT written
     d_return_trace [n_steps][n_envs] f32 or NULL   g at every step, including that step's reward
     d_summary [LT_SUMMARY_FIELDS] f64 or NULL; accumulate = 0 overwrites it, accumulate = 1 merges into what it holds (a logger reads once
                                       per interval); needs d_work, lt_episode_work_doubles(n_envs) doubles of scratch (not otherwise)
   One lane per environment, t ascending, float32, every operation rounded once (fmaf where written):
     r = reward[t][e]; d = done[t][e]
     ret = ret + r;  disc = fmaf(w, r, disc);  w = w * gamma;  g = fmaf(gamma, g, r);  len = len + 1
     trace[t][e] = g
     if d != 0:      the episode ended in this step — absorbing (bit 0), restarted on the device or at the horizon (bit 1): `done != 0`, NOT
                     `done & 1`; the reward of the ending step belongs to the old episode
         ep_return[t][e] = ret; ep_disc_return[t][e] = disc; ep_length[t][e] = len; the lane's float64 partial of the summary takes them
         ret = 0; disc = 0; w = 1; g = 0; len = 0      by ASSIGNMENT, never by multiplying with a mask: a NaN does not cross an episode end
   A value does not depend on n_envs, on the environment's place or on how the steps are split over calls. The lanes' float64 partials
   are combined without floating-point atomics in an order that depends on n_envs only — a fixed tree in LDS per workgroup of 256 lanes,
   the workgroups' partials in d_work, and a one-workgroup kernel behind it that adds them in index order: the same call twice gives
   the same bits.
   `stream`, `sync`: as in lm_step_device, with NULL = the device's null stream (there is no library stream here). The caller orders the
   call behind whatever filled the tapes, exactly as for a torch op on them.
   Every argument is checked before the first HIP call, so a refusal works on a machine without a GPU, and a refused call launches
   nothing: null d_reward / d_done / d_carry / d_len, n_steps < 1, n_envs < 1, gamma outside [0, 1] or not finite, d_summary without d_work. */
int lt_tape_episodes(int n_steps, long long n_envs, const float* d_reward, const uint8_t* d_done, const uint8_t* d_mask, float gamma,
                     float* d_carry, int32_t* d_len,
                     float* d_ep_return, float* d_ep_disc_return, int32_t* d_ep_length, float* d_return_trace,
                     double* d_summary, int accumulate, double* d_work, void* stream, int sync);

#ifdef __cplusplus
}
#endif
#endif
